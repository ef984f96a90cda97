// kb_shared_plus_batch.hip -- chip-wide passes for shared dictionaries that still grow under the margin rule:
// kb_set_shared_plus_batch / kb_get_shared_plus_batch / kb_shared_plus_batch_info (ranslice.h).  #included by
// rs_api.hip after kb_shared_plus.hip.
//
// Between two insertions the landmarks and Kinv of a dictionary are fixed, so a merged list is taken in SEGMENTS: for the
// proposals that remain, KF, d* = Kinv KF, F0 and the Gram block are formed by kernels as wide as the chip -- the bodies of
// shared_cols_kernel, shared_matvec_kernel / shared_matvec_mfma_kernel and shared_gram_kernel (kb_kbrl.hip), copied so that those
// kernels stay what they were, every value summed as they sum it, rows and columns counted from the segment's first proposal --
// and one wave walks them by apply_full_batch<true>'s rule until a mistake asks for an insertion (max(1 - A[p][p], 0) > eta below
// the capacity).  That sample goes through kernel_column_full and apply_update_plus, which decide for themselves; the next segment
// starts behind it.  Per-slice state on the device (the next proposal, whether the list is engaged and not done) lets every kernel
// of a round return at once, so launch_shared_plus_batch enqueues a fixed number of rounds and a finishing kernel whose workgroup
// runs the same device functions for what is left: the result does not depend on the number of rounds.

namespace kb {

struct SpbArgs {
    KbDev D;
    KbState K;
    const double* props;
    const int32_t* counts;
    int budget;
    int32_t* st;               // [S][4]: the first proposal of the next segment, 1 while the list is engaged and not done
    unsigned long long* info;  // [8] kb_shared_plus_batch_info
    int32_t* rest;             // [S] the counts the parent's kernels see: 0 for an engaged list
    uint64_t* gstats;
    int min_m;
    int mfma;
};

// which lists are engaged: min_landmarks <= m < capacity, not KBRL_SERIAL_APPLY, at least one proposal
__global__ __launch_bounds__(64) void spb_begin_kernel(SpbArgs a) {
    const int s = threadIdx.x;
    if (s >= a.D.S) return;
    const int m = a.K.m[s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    const bool eng = np > 0 && m >= a.min_m && m < a.D.cap && !a.D.serial_apply;
    a.st[4 * s] = 0;
    a.st[4 * s + 1] = eng ? 1 : 0;
    a.rest[s] = eng ? 0 : a.counts[s];
    if (eng) atomicAdd(&a.info[0], 1ull);
}

// ---- the stages of a segment.  pr: the segment's first proposal; n proposals; thread tid of nt / wave w of nw of the launch (a
// wide kernel) or of the workgroup (the finishing kernel): which thread forms a value does not enter the value.

// shared_cols_kernel's body
__device__ __forceinline__ void spb_cols(const KbDev& D, const KbState& K, int s, int m, const double* pr, int n, int budget, int tid, int nt) {
    const int d = D.dims[s] + 1, capr = kb_capr(D.cap);
    const uint64_t* sh = shells_of(D, K, s);
    double* KF = K.workb + (size_t)s * 2 * budget * capr;
    for (int e = tid; e < n * m; e += nt) {
        const int p = e / m, j = e - p * m;
        const double* x = pr + (size_t)p * KB_PROP_W + 2;
        const double* P = vec_page(K, sh, j >> 6);
        const int l = j & 63;
        double d0 = 0.0;
        for (int q = 0; q < d - 1; ++q) {
            const double t = P[q * KB_CH + l] - x[q];
            d0 += t * t;
        }
        const int c = ((int)pr[(size_t)p * KB_PROP_W + 1]) >> 2;
        const double dl = P[(d - 1) * KB_CH + l] - (double)c / (double)D.n_prbs;
        KF[(size_t)p * capr + j] = rs_exp(-D.gamma * (d0 + dl * dl));
    }
}

// shared_matvec_kernel's body: matvec_colsum's sums
__device__ __forceinline__ void spb_matvec_col(const KbDev& D, const KbState& K, int s, int m, int n, int budget, int wave, int nw) {
    const int capr = kb_capr(D.cap);
    const uint64_t* sh = shells_of(D, K, s);
    const int lane = threadIdx.x & 63;
    const int nb = (m + 63) >> 6;
    const double* KF = K.workb + (size_t)s * 2 * budget * capr;
    double* DS = K.workb + (size_t)s * 2 * budget * capr + (size_t)budget * capr;
    const int nwork = nb * ((n + 3) >> 2);
    for (int wk = wave; wk < nwork; wk += nw) {
        const int bi = wk % nb, p0 = (wk / nb) * 4;
        double a[8][4];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) a[u][r] = 0.0;
        for (int bj = 0; bj < nb; ++bj) {
            const int rows = m - 64 * bj < 64 ? m - 64 * bj : 64;
            const double* tp = kinv_tile(K, sh, bj, bi) + lane;
            double kfv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) kfv[r] = KF[(size_t)(p0 + r < n ? p0 + r : p0) * capr + 64 * bj + lane];
            for (int r0 = 0; r0 < rows; r0 += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int rr = r0 + u;
                    if (rr < rows) {
                        const double kv = tp[rr * 64];
#pragma unroll
                        for (int r = 0; r < 4; ++r) a[u][r] = __builtin_fma(kv, readlane_f64(kfv[r], rr), a[u][r]);
                    }
                }
            }
        }
        const int i = 64 * bi + lane;
        if (i < m) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (p0 + r < n)
                    DS[(size_t)(p0 + r) * capr + i] = ((a[0][r] + a[1][r]) + (a[2][r] + a[3][r])) + ((a[4][r] + a[5][r]) + (a[6][r] + a[7][r]));
        }
    }
}

// shared_matvec_mfma_kernel's body (m a multiple of 64): the same sums on the matrix cores
__device__ __forceinline__ void spb_matvec_mfma(const KbDev& D, const KbState& K, int s, int m, int n, int budget, int wave, int nw) {
    const int capr = kb_capr(D.cap);
    const uint64_t* sh = shells_of(D, K, s);
    const int lane = threadIdx.x & 63, li = lane & 15, kq = lane >> 4;
    const int nb = m >> 6;
    const double* KF = K.workb + (size_t)s * 2 * budget * capr;
    double* DS = K.workb + (size_t)s * 2 * budget * capr + (size_t)budget * capr;
    const int npt = (n + 15) >> 4, nct = m >> 4;
    const int nwork = npt * nct;
    for (int wk = wave; wk < nwork; wk += nw) {
        const int ct = wk / npt, pt = wk - ct * npt;
        const int p = 16 * pt + li;
        const int bi = ct >> 2, ci = 16 * (ct & 3) + li;
        const double* ar = KF + (size_t)(p < n ? p : 0) * capr + 8 * kq;
        kb_f64x4 acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = (kb_f64x4){0.0, 0.0, 0.0, 0.0};
        for (int bj = 0; bj < nb; ++bj) {
            const double* tp = kinv_tile(K, sh, bj, bi) + (size_t)(8 * kq) * 64 + ci;
            double a[2][8], b[2][8];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    a[h][c] = p < n ? ar[64 * bj + 32 * h + c] : 0.0;
                    b[h][c] = tp[(size_t)(32 * h + c) * 64];
                }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[h][c], b[h][c], acc[c], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int po = 16 * pt + kq + 4 * r;
            if (po < n)
                DS[(size_t)po * capr + 64 * bi + ci] =
                    ((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + ((acc[4][r] + acc[5][r]) + (acc[6][r] + acc[7][r]));
        }
    }
}

// shared_gram_kernel's body: the lower block triangle of A[p][q] = KF_p . DS_q (stored by column) and F0_p = KF_p . coeff
__device__ __forceinline__ void spb_gram(const KbDev& D, const KbState& K, int s, int m, int n, int budget, int wave, int nw) {
    const int capr = kb_capr(D.cap);
    const int lane = threadIdx.x & 63, kq = lane >> 4, li = lane & 15;
    const double* KF = K.workb + (size_t)s * 2 * budget * capr;
    const double* DS = KF + (size_t)budget * capr;
    double* A = K.workg + (size_t)s * budget * budget;
    double* F0 = K.workf + (size_t)s * budget;
    const int nt = (n + 15) >> 4, ntile = nt * (nt + 1) / 2;
    for (int wk = wave; wk < ntile + n; wk += nw) {
        if (wk >= ntile) {
            const int p = wk - ntile;
            const uint64_t* sh = shells_of(D, K, s);
            double part[4];
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                part[v] = 0.0;
                for (int j = 64 * v + lane; j < m; j += 256) part[v] += KF[(size_t)p * capr + j] * vec_page(K, sh, j >> 6)[KB_ROW_CO * KB_CH + lane];
            }
            for (int dd = 32; dd >= 1; dd >>= 1) {
#pragma unroll
                for (int v = 0; v < 4; ++v) part[v] += __shfl_xor(part[v], dd);
            }
            double t = 0.0;
#pragma unroll
            for (int v = 0; v < 4; ++v) t += __shfl(part[v], 0);
            if (lane == 0) F0[p] = t;
            continue;
        }
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= wk) ++ti;
        const int tj = wk - ti * (ti + 1) / 2;
        const int pa = 16 * ti + li, qb = 16 * tj + li;
        const double* ar = KF + (size_t)(pa < n ? pa : 0) * capr;
        const double* br = DS + (size_t)(qb < n ? qb : 0) * capr;
        kb_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < m; k0 += 32) {
            double a[8], b[8];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = k0 + 16 * h + 4 * kq + u;
                    a[4 * h + u] = (pa < n && k < m) ? ar[k] : 0.0;
                    b[4 * h + u] = (qb < n && k < m) ? br[k] : 0.0;
                }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int p = 16 * ti + kq + 4 * r, q = 16 * tj + li;
            if (p < n && q < n) A[(size_t)q * budget + p] = acc[r];
        }
    }
}

// The ordered part of a segment, by the slice's own workgroup: apply_full_batch<true>'s walk over the n remaining proposals (one
// wave; g starts at 0) with one addition -- a mistake with max(1 - A[p][p], 0) > eta below the capacity stops the walk BEFORE it is
// applied -- and its tail, the coefficients taking the applied d* in list order.  co: the coefficient column, wl: 4 x budget
// doubles, in LDS.  Left in wl + 2 budget: [1] the proposal the walk stopped at (-1: none), [2] its f_p, [3] the samples that changed
// the coefficients, [4] those that formed delta (the stopping one is counted by its own update).
__device__ void spb_walk(const KbDev& D, const KbState& K, int s, int m, const double* pr, int np, int budget, double* co, double* wl) {
    const int capr = kb_capr(D.cap);
    const uint64_t* sh = shells_of(D, K, s);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double* DS = K.workb + (size_t)s * 2 * budget * capr + (size_t)budget * capr;
    const double* A = K.workg + (size_t)s * budget * budget;
    const double* F0 = K.workf + (size_t)s * budget;
    double* wq = wl;
    double* lst = wl + budget;
    double* cnt = wl + 2 * budget;
    for (int j = threadIdx.x; j < m; j += blockDim.x) co[j] = *vec_at(K, sh, KB_ROW_CO, j);
    for (int q = threadIdx.x; q < budget; q += blockDim.x) wq[q] = 0.0;
    __syncthreads();
    if (wave == 0) {
        bool sat = false;
        int napp = 0, stop = -1;
        double fstop = 0.0;
        uint64_t work = 0;
        const int nq = (np + 63) >> 6;
        double g[4] = {0.0, 0.0, 0.0, 0.0}, f0v[4];
        int yv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int q = lane + 64 * k;
            yv[k] = q < np ? ((((int)pr[(size_t)q * KB_PROP_W + 1]) & 1) ? 1 : -1) : 1;
            f0v[k] = q < np ? F0[q] : 0.0;
        }
        double nxt[2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < 4; ++k) nxt[h][k] = (h < np && k < nq && lane + 64 * k < np) ? A[(size_t)h * budget + lane + 64 * k] : 0.0;
        for (int p = 0; p < np; ++p) {
            double col[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                col[k] = nxt[p & 1][k];
                nxt[p & 1][k] = (p + 2 < np && k < nq && lane + 64 * k < np) ? A[(size_t)(p + 2) * budget + lane + 64 * k] : 0.0;
            }
            const int pk = p >> 6, pl = p & 63;
            const int y = __builtin_amdgcn_readlane(pk == 0 ? yv[0] : (pk == 1 ? yv[1] : (pk == 2 ? yv[2] : yv[3])), pl);
            const double f = readlane_f64(pk == 0 ? f0v[0] + g[0] : (pk == 1 ? f0v[1] + g[1] : (pk == 2 ? f0v[2] + g[2] : f0v[3] + g[3])), pl);
            const double margin = (double)y * f;
            if (margin >= 1.0) continue;
            const double dg = readlane_f64(pk == 0 ? col[0] : (pk == 1 ? col[1] : (pk == 2 ? col[2] : col[3])), pl);
            double delta = 1.0 - dg;
            delta = delta > 0.0 ? delta : 0.0;
            double w = (double)y;
            if (margin <= 0.0) {
                if (delta > D.eta) {
                    if (m < D.cap) {  // the dictionary would grow: apply_update_plus takes the sample, the next segment follows it
                        stop = p;
                        fstop = f;
                        break;
                    }
                    sat = true;
                }
                work += 1;
            } else {  // margin_update's statements on the Gram block's diagonal
                work += 1;
                double norm = 1.0 - delta;
                norm = norm > 0.0 ? norm : 0.0;
                const double loss = 1.0 - margin;
                const double slack = loss - delta / D.eta;
                if (!(slack > 0.0)) continue;  // branch 4
                double alpha = loss / norm;
                alpha = 1.0 < alpha ? 1.0 : alpha;
                const double by_slack = 2.0 * slack / norm;
                alpha = by_slack < alpha ? by_slack : alpha;
                w = alpha * (double)y;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (lane + 64 * k > p) g[k] = __builtin_fma(w, col[k], g[k]);
            if (lane == 0) {
                wq[p] = w;
                lst[napp] = (double)p;
            }
            napp += 1;
        }
        if (lane == 0) {
            cnt[0] = (double)napp;
            cnt[1] = (double)stop;
            cnt[2] = fstop;
            cnt[3] = (double)napp;
            cnt[4] = (double)work;
        }
        if (sat && lane == 0) atomicOr(&K.err[0], 8);
    }
    __syncthreads();
    const int napp = (int)cnt[0];
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        double c = co[j];
        for (int a0 = 0; a0 < napp; a0 += 4) {
            double v[4], yy[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = (int)lst[a0 + u < napp ? a0 + u : a0];
                v[u] = DS[(size_t)q * capr + j];
                yy[u] = wq[q];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (a0 + u < napp) c = c + yy[u] * v[u];
        }
        *vec_at(K, sh, KB_ROW_CO, j) = c;
    }
    __syncthreads();
}

// One segment's end, by the whole workgroup: the walk, then the sample it stopped at through kernel_column_full and
// apply_update_plus (authoritative: its own residual_delta decides, its capacity and pool rules apply).  Updates m and from; returns
// whether proposals are left.  finishing: the segment is run by the finishing kernel (info[4]).
__device__ bool spb_segment_end(const SpbArgs& a, int s, int& m, int& from, int np, Lds& sm, double* dyn, int finishing) {
    const KbDev& D = a.D;
    const KbState& K = a.K;
    const int budget = a.budget;
    const double* pr = a.props + ((size_t)s * budget + from) * KB_PROP_W;
    double* wl = dyn + kb_capr(D.cap);
    spb_walk(D, K, s, m, pr, np - from, budget, dyn, wl);
    const double* cnt = wl + 2 * budget;
    const int stop = (int)cnt[1];
    const double fstop = cnt[2];
    unsigned long long n_changed = (unsigned long long)cnt[3], n_work = (unsigned long long)cnt[4], n_grow = 0;
    const int covered = np - from;
    __syncthreads();
    int m_new = m;
    if (stop >= 0) {
        const double* p = pr + (size_t)stop * KB_PROP_W;
        const int packed = (int)p[1];
        const int c = packed >> 2, y = (packed & 1) ? 1 : -1;
        const int d = D.dims[s] + 1;
        const uint64_t* sh = shells_of(D, K, s);
        if ((int)threadIdx.x < d - 1) sm.x[threadIdx.x] = p[2 + threadIdx.x];
        __syncthreads();
        const double t = (double)c / (double)D.n_prbs;
        kernel_column_full(D, K, sh, m, d, sm.x, t);
        int branch;
        double delta;
        m_new = apply_update_plus(D, K, s, 0, m, d, sm.x, t, c, y, fstop, sm, &branch, &delta);
        n_work += 1;
        n_changed += branch != 4;
        n_grow += (branch == 2 && m_new > m) ? 1 : 0;
        from += stop + 1;
    } else {
        from = np;
    }
    m = m_new;
    const bool left = from < np;
    if (threadIdx.x == 0) {
        K.m[s] = m;
        K.kf_owner[s] = -1;
        a.st[4 * s] = from;
        a.st[4 * s + 1] = left ? 1 : 0;
        atomicAdd(&a.info[1], 1ull);
        atomicAdd(&a.info[2], (unsigned long long)covered);
        if (stop >= 0) atomicAdd(&a.info[3], 1ull);
        if (finishing) atomicAdd(&a.info[4], 1ull);
        if (n_work) atomicAdd((unsigned long long*)&K.hv_work[6], n_work);
        atomicAdd((unsigned long long*)&a.gstats[1], n_changed);
        atomicAdd((unsigned long long*)&a.gstats[2], n_grow);
        atomicAdd((unsigned long long*)&a.gstats[16 + s], n_changed);
        atomicAdd((unsigned long long*)&a.gstats[24 + s], (unsigned long long)(stop >= 0 ? stop + 1 : covered));
    }
    __syncthreads();
    return left;
}

// ---- a round: three wide kernels and the walk.  Each returns at once for a list that is not engaged or is done.
#define KB_SPB_COLS_BLOCKS 64
#define KB_SPB_MATVEC_BLOCKS 256
#define KB_SPB_GRAM_BLOCKS 128

__global__ __launch_bounds__(256) void spb_cols_kernel(SpbArgs a) {
    const int s = blockIdx.x;
    if (!a.st[4 * s + 1]) return;
    const int from = a.st[4 * s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    spb_cols(a.D, a.K, s, a.K.m[s], a.props + ((size_t)s * a.budget + from) * KB_PROP_W, np - from, a.budget,
             blockIdx.y * blockDim.x + threadIdx.x, gridDim.y * blockDim.x);
}

__global__ __launch_bounds__(256) void spb_matvec_kernel(SpbArgs a) {
    const int s = blockIdx.x;
    if (!a.st[4 * s + 1]) return;
    const int from = a.st[4 * s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    const int m = a.K.m[s];
    const int wave = blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), nw = gridDim.y * (blockDim.x >> 6);
    if (a.mfma && !(m & 63))
        spb_matvec_mfma(a.D, a.K, s, m, np - from, a.budget, wave, nw);
    else
        spb_matvec_col(a.D, a.K, s, m, np - from, a.budget, wave, nw);
}

__global__ __launch_bounds__(256) void spb_gram_kernel(SpbArgs a) {
    const int s = blockIdx.x;
    if (!a.st[4 * s + 1]) return;
    const int from = a.st[4 * s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    spb_gram(a.D, a.K, s, a.K.m[s], np - from, a.budget, blockIdx.y * (blockDim.x >> 6) + (threadIdx.x >> 6), gridDim.y * (blockDim.x >> 6));
}

// dynamic LDS: kb_apply_lds_doubles()
__global__ __launch_bounds__(1024) void spb_walk_kernel(SpbArgs a) {
    extern __shared__ double spb_dyn_lds[];
    __shared__ Lds sm;
    const int s = blockIdx.x;
    if (!a.st[4 * s + 1]) return;
    int from = a.st[4 * s], m = a.K.m[s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    (void)spb_segment_end(a, s, m, from, np, sm, spb_dyn_lds, 0);
}

// what the rounds left: the same segments, the stages by the slice's own workgroup.  d* by the column walk whatever m is: its sums
// are the matrix cores' bit for bit (shared_matvec_mfma_kernel), and its registers leave room for sixteen waves, which one CU
// streaming Kinv needs more than it needs the matrix cores
__global__ __launch_bounds__(1024) void spb_finish_kernel(SpbArgs a) {
    extern __shared__ double spb_dyn_lds[];
    __shared__ Lds sm;
    const int s = blockIdx.x;
    if (!a.st[4 * s + 1]) return;
    int from = a.st[4 * s], m = a.K.m[s];
    const int np = a.counts[s] < a.budget ? a.counts[s] : a.budget;
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    bool left = true;
    while (left) {
        const int n = np - from;
        spb_cols(a.D, a.K, s, m, a.props + ((size_t)s * a.budget + from) * KB_PROP_W, n, a.budget, threadIdx.x, blockDim.x);
        __syncthreads();
        spb_matvec_col(a.D, a.K, s, m, n, a.budget, wave, nw);
        __syncthreads();
        spb_gram(a.D, a.K, s, m, n, a.budget, wave, nw);
        __syncthreads();
        left = spb_segment_end(a, s, m, from, np, sm, spb_dyn_lds, 1);
    }
}

}  // namespace kb

#define KB_SPB_BYTES(S) (64 + 16 * (size_t)(S) + 4 * (size_t)(S))  // info[8], the per-slice state, the parent kernels' counts

static void kb_shared_plus_batch_release(kb_handle* k) {
    if (k->d_spb) (void)hipFree(k->d_spb);
    k->d_spb = nullptr;
}

// the counters since kb_reset start over (kb_restart_counters)
static void kb_shared_plus_batch_restart(kb_handle* k) {
    if (k->d_spb) (void)hipMemsetAsync(k->d_spb, 0, 64, k->stream);
}

static bool kb_shared_plus_batch_on(const kb_handle* k) { return k->shared_plus && k->spb_min > 0 && k->d_spb; }

// launch_shared_apply with both switches on.  The parent's kernels go first and see a count of 0 for every engaged list, so they
// take the lists of dictionaries below min_landmarks and at their capacity exactly as they did and decide from K.m before any segment
// changes it; then the rounds, then the finishing kernel.  Plain launches; nothing waits on the host.
static void launch_shared_plus_batch(kb_handle* k, const double* props, const int32_t* counts, int budget) {
    const unsigned S = (unsigned)k->cfg.n_slices;
    static const bool mfma_on = !(dev_env("KBRL_MATVEC_MFMA") && atoi(dev_env("KBRL_MATVEC_MFMA")) == 0);
    kb::SpbArgs a;
    a.D = k->D;
    a.K = k->K;
    a.props = props;
    a.counts = counts;
    a.budget = budget;
    a.info = (unsigned long long*)k->d_spb;
    a.st = (int32_t*)(k->d_spb + 64);
    a.rest = (int32_t*)(k->d_spb + 64 + 16 * (size_t)S);
    a.gstats = k->d_gstats;
    a.min_m = k->spb_min;
    a.mfma = mfma_on ? 1 : 0;
    hipLaunchKernelGGL(kb::spb_begin_kernel, dim3(1), dim3(64), 0, k->stream, a);
    hipLaunchKernelGGL(kb::shared_cols_kernel, dim3(S, KB_COLS_BLOCKS), dim3(256), 0, k->stream, k->D, k->K, props, a.rest, budget);
    if (mfma_on && k->cfg.capacity % 64 == 0)
        hipLaunchKernelGGL(kb::shared_matvec_mfma_kernel, dim3(S, KB_MATVEC_BLOCKS), dim3(256), 0, k->stream, k->D, k->K, a.rest, budget);
    else
        hipLaunchKernelGGL(kb::shared_matvec_kernel, dim3(S, KB_MATVEC_BLOCKS), dim3(256), 0, k->stream, k->D, k->K, a.rest, budget, 0);
    hipLaunchKernelGGL(kb::shared_gram_kernel, dim3(S, 128), dim3(256), 0, k->stream, k->D, k->K, a.rest, budget);
    const size_t lds = sizeof(double) * kb::kb_apply_lds_doubles(k->cfg.capacity, k->budget_cap);
    hipLaunchKernelGGL(kb::shared_apply_plus_kernel, dim3(S), dim3(1024), lds, k->stream, k->D, k->K, props, a.rest, budget, k->d_gstats);
    for (int r = 0; r < k->spb_segments; ++r) {
        hipLaunchKernelGGL(kb::spb_cols_kernel, dim3(S, KB_SPB_COLS_BLOCKS), dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::spb_matvec_kernel, dim3(S, KB_SPB_MATVEC_BLOCKS), dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::spb_gram_kernel, dim3(S, KB_SPB_GRAM_BLOCKS), dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::spb_walk_kernel, dim3(S), dim3(1024), lds, k->stream, a);
    }
    hipLaunchKernelGGL(kb::spb_finish_kernel, dim3(S), dim3(1024), lds, k->stream, a);
}

/* Host state of the handle like kb_set_shared_plus: off by default, in no kb_save_state blob, left alone by kb_share, kb_unshare
   and kb_shared_prune; remembered, but it acts only while kb_set_shared_plus is on.  The per-slice state and the counters are
   allocated here: the first launch may be inside a stream capture. */
extern "C" int kb_set_shared_plus_batch(kb_handle* k, int32_t min_landmarks, int32_t segments) {
    if (!k) return RS_EINVAL;
    if (min_landmarks != 0 && (min_landmarks < 2 || min_landmarks > k->D.cap)) {
        k->err = "kb_set_shared_plus_batch: min_landmarks = " + std::to_string(min_landmarks) +
                 " (0 turns the segments off, the default; else 2 .. the handle's capacity, " + std::to_string(k->D.cap) +
                 ": a single landmark's float32 regime stays one by one)";
        return RS_EINVAL;
    }
    if (segments < 0 || segments > 16) {
        k->err = "kb_set_shared_plus_batch: segments = " + std::to_string(segments) +
                 " (0 .. 16 segment rounds enqueued per apply; the finishing launch takes what they leave)";
        return RS_EINVAL;
    }
    if (!k->D.shared) {
        k->err = "kb_set_shared_plus_batch: not a shared-dictionary handle";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_set_shared_plus_batch: a round is open between kb_shared_scan and kb_shared_commit; the switch changes between steps only";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    if (k->spb_min != min_landmarks || k->spb_segments != segments) {
        const int rc = kb_retire_graph(k);
        if (rc != RS_OK) return rc;
    }
    if (min_landmarks && !k->d_spb) {
        const size_t bytes = KB_SPB_BYTES(k->cfg.n_slices);
        HIPCHK(k, hipMalloc((void**)&k->d_spb, bytes));
        HIPCHK(k, hipMemsetAsync(k->d_spb, 0, bytes, k->stream));
        const size_t lds = sizeof(double) * kb::kb_apply_lds_doubles(k->cfg.capacity, k->budget_cap);
        if (lds > 48 * 1024) {
            HIPCHK(k, hipFuncSetAttribute((const void*)kb::spb_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            HIPCHK(k, hipFuncSetAttribute((const void*)kb::spb_finish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
    }
    k->spb_min = min_landmarks;
    k->spb_segments = segments;
    return RS_OK;
}

extern "C" int kb_get_shared_plus_batch(kb_handle* k, int32_t* min_landmarks, int32_t* segments) {
    if (!k || !min_landmarks || !segments) return RS_EINVAL;
    *min_landmarks = k->spb_min;
    *segments = k->spb_segments;
    return RS_OK;
}

extern "C" int kb_shared_plus_batch_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    return kb_read_words(k, k->d_spb, 8, work);
}
