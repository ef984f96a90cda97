// kb_control_plus_batch.hip -- the closed control loop in Projectron++ mode with ONE pass over Kinv for a group of candidates,
// behind kb_set_control_plus_batch.  #included by rs_api.hip after kb_control_plus.hip: it is control_plus_kernel's
// row with another walk over the candidates, and it changes none of that file's, kb_fit's, kb_fit_steps's or kb_kbrl.hip's kernels.
//
// The candidates of a step differ in their last coordinate only.  K_f(a) depends on the landmarks alone and d*(a) = Kinv K_f(a) on
// the landmarks and Kinv alone, and of the rule's branches only an insertion (finish_update, branch 2) changes either: branches 1
// and 3 move coefficients, 0 and 4 write nothing.  So the d* of the next `width` candidates are formed together from one read of
// the stored triangle, and the walk then goes on in order with the coefficients as they are: every candidate's f is formed from
// its K_f column and the current coefficients in predict_column_steps's order, its d* is the one the parent would have formed at
// that point (same Kinv, same K_f, same order of sums), and the rule's tail -- residual_delta, margin_update, finish_update --
// runs unmodified on the candidate's two columns, copied into the page's KB_ROW_KF / KB_ROW_DS rows.  An insertion ends the
// group behind itself.  Landmarks, coefficients, all of Kinv, the control state and every counter are bit for bit the parent's.
//
// Scratch.  The group's K_f and d* columns live in an ARENA of 2 x width x max_landmarks doubles.  A launch has at most
// KB_CPB_ARENAS workgroups, each with an arena of its own; they take the learners from a ticket counter, which the last workgroup
// to leave sets back -- so a captured launch replays without a memset node, and the scratch does not grow with the fleet:
//     scratch_bytes = KB_CPB_HEAD + min(n_envs x S, KB_CPB_ARENAS) x 2 x width x max_landmarks x 8
// (KB_CPB_HEAD = 128: work[8] and the two ticket words).  A dictionary the arena cannot hold (m > max_landmarks), and the float32
// regime of fewer than two landmarks, take the parent's statements candidate by candidate.
//
// The pass.  A wave takes one OUTPUT block b of 64 entries and accumulates, for every column of the group, matvec_tri_combine's
// sums in matvec_tri_combine's order with no stored partial sums: first the row of tiles (b, 0) .. (b, b - 1) in increasing b_j
// from zero (matvec_tri_tiles's row-wise partial sum: eight fma chains over the column classes mod 8, the three-step butterfly),
// kept per wave in LDS beside the tile's block of the K_f columns; then the column of tiles (b, b), (b + 1, b), .. in increasing b_i (its column-wise partial sum: eight fma
// chains over the row classes mod 8, ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7))), in registers; then the sum of the two.
// Every output block costs n_b tiles, so the waves are level; an off-diagonal tile is read once per orientation -- twice in all,
// against `width` times by the one-by-one walk -- and each read feeds `width` columns of accumulators (f64 fma is the floor:
// 64 x 64 of them per tile, column and orientation, as in the parent).  The kernel waits on latency more than on anything else,
// so every instance is built for two waves per SIMD (two workgroups per CU); width 8 pays 196 B per lane of scratch for that and
// is still the faster for it (DESIGN.md §8m has the figures of both builds).

namespace kb {

#define KB_CPB_W 8          // the widest group
#define KB_CPB_ARENAS 1024  // workgroups of a launch, each with an arena of its own
#define KB_CPB_HEAD 128     // bytes in front of the arenas: work[8], the ticket (next learner, workgroups that have left)

struct CtlBatchArgs {
    CtlArgs C;
    unsigned long long* work;   // [4] control_plus_kernel's counters
    unsigned long long* bwork;  // [8] kb_control_plus_batch_info
    int32_t* ticket;            // [2]
    double* arena;              // [gridDim.x][2][W][max_m]
    int32_t max_m, T;
};

template <int W>
struct BatchLds {
    double tsum[4][W][64];  // per wave: the row-wise sums of its output block, by column of the group
    double kc[4][W][64];    // per wave: the group's K_f entries of the column block a row-wise tile is multiplied with (in registers
                            // they are 16 W VGPRs, which at W = 8 left the kernel one wave per SIMD)
    double red[W][4];       // block_sum's wave totals, by column
    double f[W];            // the group's scores as step 2 formed them
    int task;
};

// d* = Kinv K_f for the g columns kf[w * ld + j] of a group, into ds[w * ld + j], j < m (2 <= m <= ld, triangle storage).  Whole
// 256-thread block; the caller puts a barrier in front (the columns are in memory) and behind (so is d*).  Per column the sums
// of matvec_tri_tiles + matvec_tri_combine in their order (a change there is made here too).  The body of the loop over b is
// restated as cpw_unit (kb_control_plus_wide.hip), one output block per wave of a chip-wide launch: a change here is made there too.
template <int W>
__device__ __forceinline__ void batch_matvec(const KbState& K, const uint64_t* sh, int m, int g, const double* kf, double* ds, int ld,
                                             BatchLds<W>& bs) {
    const int nb = (m + 63) >> 6, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int cl = lane >> 3, sg = lane & 7;
    double(*ts)[64] = bs.tsum[wv];
    double(*kc)[64] = bs.kc[wv];
    for (int b = wv; b < nb; b += 4) {
        const int rows_b = m - 64 * b < 64 ? m - 64 * b : 64;
        // ---- its row of tiles, increasing b_j, from zero: tpart[r] = sum_c T[r][c] K_f[64 b_j + c]
        for (int bj = 0; bj < b; ++bj) {
            const double* Tp = kinv_tile_lo(K, sh, b, bj);
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < g) kc[w][lane] = kf[(size_t)w * ld + 64 * bj + lane];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int x = 0; x < 8; ++x) {
                if (8 * x >= rows_b) break;  // (wave-uniform; the last row block of the dictionary)
                double tv[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) tv[k] = Tp[(8 * x + cl) * 64 + sg + 8 * k];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w < g) {  // (block-uniform)
                        double ta = 0.0;
#pragma unroll
                        for (int k = 0; k < 8; ++k) ta = __builtin_fma(tv[k], kc[w][sg + 8 * k], ta);
                        ta += __shfl_xor(ta, 1);
                        ta += __shfl_xor(ta, 2);
                        ta += __shfl_xor(ta, 4);
                        if (sg == 0) ts[w][8 * x + cl] = (bj == 0 ? 0.0 : ts[w][8 * x + cl]) + ta;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();  // (read before the next tile's column block overwrites them)
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        // ---- its column of tiles, increasing b_i: dpart[c] = sum_r T[r][c] K_f[64 b_i + r]
        double dsum[W];
#pragma unroll
        for (int w = 0; w < W; ++w) dsum[w] = 0.0;
        for (int br = b; br < nb; ++br) {
            const double* Tp = kinv_tile_lo(K, sh, br, b);
            const int rows = m - 64 * br < 64 ? m - 64 * br : 64;
            double kfr[W];
#pragma unroll
            for (int w = 0; w < W; ++w) kfr[w] = (w < g && 64 * br + lane < m) ? kf[(size_t)w * ld + 64 * br + lane] : 0.0;
            double acc[W][8];
#pragma unroll
            for (int w = 0; w < W; ++w) {
#pragma unroll
                for (int u = 0; u < 8; ++u) acc[w][u] = 0.0;
            }
            for (int x = 0; x < 8; ++x) {
                if (8 * x >= rows) break;  // (wave-uniform)
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = 8 * x + u < rows ? Tp[(8 * x + u) * 64 + lane] : 0.0;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w < g) {
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (8 * x + u < rows) acc[w][u] = __builtin_fma(v[u], readlane_f64(kfr[w], 8 * x + u), acc[w][u]);
                    }
                }
            }
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const double part = ((acc[w][0] + acc[w][1]) + (acc[w][2] + acc[w][3])) + ((acc[w][4] + acc[w][5]) + (acc[w][6] + acc[w][7]));
                dsum[w] = br == b ? part : dsum[w] + part;
            }
        }
        // the wave's own row sums, written by the lanes sg == 0 and read by lane = entry
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (64 * b + lane < m) {
#pragma unroll
            for (int w = 0; w < W; ++w)
                if (w < g) ds[(size_t)w * ld + 64 * b + lane] = dsum[w] + (b == 0 ? 0.0 : ts[w][lane]);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (read before the next output block overwrites them)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

// what a row counted for kb_control_plus_batch_info (block-uniform, in registers)
struct BatchWork {
    unsigned long long w[8];
};

// THE GROUP WALK: the candidates a0 .. a1 of one learner's row, label y, in the reference's order, through the margin rule (step 4
// of DESIGN.md §8l as §8m restates it).  sm.x holds the row's state coordinates, pre its prefixes (thread t: j = t, t + 256, ...);
// kf / ds are the workgroup's arena, W columns of `ld` doubles each.  Whole 256-thread block.  Returns the last candidate's f;
// *m_io, the row's counters and bw are advanced in place.  A device function of its own, so that another row loop
// (fit_steps_learner's) could call it.
//
// A candidate is either ONE BY ONE (fewer than two landmarks: the float32 regime; more than `ld`: the arena cannot hold the
// columns) -- predict_column_steps<true>, fit_decide, and fit_rule<KB_ALG_PROJECTRON_PLUS> RESTATED: its counters and
// apply_update_plus's head (the decision on y f, d* by the float32 product or matvec_tri_colsum; per-replica dictionaries store the
// triangle) -- or a member of a GROUP, whose K_f and d* columns are copied into the page's rows.  Both then run the rule's tail at
// ONE place: finish_update on y f <= 0, margin_update inside the margin (a change to fit_rule or apply_update_plus is made here too;
// behind a call of fit_rule beside the group's own tail finish_update stood twice in the kernel, as two calls with 656 B per lane
// of scratch between them).  cpw_walk_kernel (kb_control_plus_wide.hip) restates the walk cut where a group waits for its pass:
// a change here is made there too.
template <int W>
__device__ __forceinline__ double plus_group_walk(const KbDev& D, const KbState& K, int dt, int task, int env, int s, const uint64_t* sh, int d,
                                                  int y, int a0, int a1, int* m_io, double* pre, Lds& sm, BatchLds<W>& bs, double* kf, double* ds,
                                                  int ld, FitCounts* c, int* row_mist, int* row_grow, int* row_matvec, BatchWork* bw) {
    const int n = D.n_prbs;
    int m = *m_io;
    double f = 0.0;
    int g = 0, gi = 0;  // the group in progress: its size, the next member (gi == g: none)
    bool dirty = false;  // a coefficient has moved since the group's scores were formed
    for (int p = a0; p <= a1; ++p) {
        const bool one = m < 2 || m > ld;  // (block-uniform; m moves only with an insertion, which ends a group)
        if (!one && gi == g) {
            // ---- the group p .. p + g - 1: its K_f columns by predict_column_steps's chain, its scores in predict_column_steps's order
            g = a1 - p + 1 < W ? a1 - p + 1 : W;
            gi = 0;
            dirty = false;
            bw->w[0] += 1;
            __syncthreads();  // (an inserted landmark's prefix is in place; the previous group's readers of the arena are done)
            double ps[W];
#pragma unroll
            for (int w = 0; w < W; ++w) ps[w] = 0.0;
            for (int j = threadIdx.x; j < m; j += 256) {
                const double* P = vec_page(K, sh, j >> 6);
                const int l = j & 63;
                const double base = j < KB_STEPS_PRE ? pre[j] : steps_prefix(K, sh, d, j, sm.x);
                const double lam = P[(d - 1) * KB_CH + l], co = P[KB_ROW_CO * KB_CH + l];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w < g) {  // (block-uniform)
                        const double x_last = (double)(p + w) / (double)n;
                        double dist = base;
                        double t = lam - x_last;
                        dist += t * t;
                        const double k = rs_exp(-D.gamma * dist);
                        kf[(size_t)w * ld + j] = k;
                        ps[w] += k * co;
                    }
                }
            }
            // block_sum, per column: the butterfly per wave, the four wave totals in order
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                double v = ps[w];
                for (int dd = 32; dd >= 1; dd >>= 1) v += __shfl_xor(v, dd);
                if (lane == 0) bs.red[w][wv] = v;
            }
            __syncthreads();  // (behind it the group's columns are in memory for the pass, too)
            if ((int)threadIdx.x < W) {
                double t = 0.0;
                for (int w4 = 0; w4 < 4; ++w4) t += bs.red[threadIdx.x][w4];
                bs.f[threadIdx.x] = t;
            }
            __syncthreads();
            // ---- the skip rule: nobody inside the margin -> the first candidate writes nothing, so the second one's f stands, and so on
            bool any = false;
            for (int w = 0; w < g; ++w) any = any || !((double)y * bs.f[w] >= 1.0);
            if (!any) {
                bw->w[1] += 1;
                for (int w = 0; w < g; ++w) {
                    f = bs.f[w];
                    (void)fit_decide(K, task, env, s, m, &f, sm);  // (y f >= 1: f != 0, no draw)
                    c->evals += (unsigned long long)m;
                }
                p += g - 1;
                gi = g;
                continue;
            }
            // ---- the pass: d* of every column from one read of the stored triangle
            const int nb = (m + 63) >> 6;
            bw->w[2] += 1;
            bw->w[3] += (unsigned long long)(nb * (nb + 1) / 2);
            bw->w[4] += (unsigned long long)g;
            batch_matvec<W>(K, sh, m, g, kf, ds, ld, bs);
            __syncthreads();
        }
        // ---- candidate p: its f
        if (one) {
            __syncthreads();  // (the previous sample's readers of sm.x are done; an inserted landmark's prefix is in place)
            if (threadIdx.x == 0) sm.x[d - 1] = (double)p / (double)n;
            __syncthreads();
            f = predict_column_steps<true>(D, K, sh, d, m, sm.x, pre, sm);
        } else if (dirty) {  // the same products with the coefficients as they are, summed again
            double ps = 0.0;
            for (int j = threadIdx.x; j < m; j += 256) ps += kf[(size_t)gi * ld + j] * *vec_at(K, sh, KB_ROW_CO, j);
            f = block_sum(ps, sm);
        } else {
            f = bs.f[gi];
        }
        (void)fit_decide(K, task, env, s, m, &f, sm);
        c->evals += (unsigned long long)m;
        // ---- the rule (apply_update_plus): y f >= 1 nothing; <= 0 Projectron's update; in between the margin rule
        const double margin = (double)y * f;
        int branch = 0, m_new = m;
        double delta = 0.0;
        if (!(margin >= 1.0)) {
            if (one) {  // d* = Kinv K_f of the K_f row: apply_update_plus's head
                if (m == 1) {
                    __syncthreads();
                    if (threadIdx.x == 0) *vec_at(K, sh, KB_ROW_DS, 0) = (double)(1.0f * (float)*vec_at(K, sh, KB_ROW_KF, 0));
                    __syncthreads();
                } else if (m >= 2) {
                    matvec_tri_colsum(K, sh, m);
                }
            } else {  // the member's two columns into the page's rows
                __syncthreads();  // (the previous candidate's readers of the rows and of sm.x are done)
                for (int j = threadIdx.x; j < m; j += 256) {
                    double* P = vec_page(K, sh, j >> 6);
                    const int l = j & 63;
                    P[KB_ROW_KF * KB_CH + l] = kf[(size_t)gi * ld + j];
                    P[KB_ROW_DS * KB_CH + l] = ds[(size_t)gi * ld + j];
                }
                if (threadIdx.x == 0) sm.x[d - 1] = (double)p / (double)n;
                __syncthreads();
            }
            const double t_last = sm.x[d - 1];
            if (margin <= 0.0)  // (inlined at this one place in every instance: as a call it cost the width-2 instance 640 B per lane of scratch)
                [[clang::always_inline]] m_new = finish_update(D, K, dt, env, m, d, sm.x, t_last, grid_index(t_last, n), y, sm, &branch, &delta, nullptr, false);
            else
                m_new = margin_update(D, K, sh, dt, m, y, margin, sm, &branch, &delta);
            if (branch >= 1 && branch <= 3) *row_mist += 1;  // (fit_rule's counters)
            if (branch == 2 && m_new > m) *row_grow += 1;
            *row_matvec += 1;  // (branches 1-4: the candidate used a d*)
            if (branch == 1 || branch == 3) dirty = true;
        }
        if (one) {
            bw->w[6] += 1;
            bw->w[7] += branch != 0;
        } else {
            ++gi;
        }
        if (m_new > m) {
            // a landmark inserted inside the row: its prefix by the same chain, formed by the thread that reads it
            if (m < KB_STEPS_PRE && (int)threadIdx.x == (m & 255)) pre[m] = steps_prefix(K, sh, d, m, sm.x);
            if (!one) {  // it ends the group behind itself: Kinv and the landmarks have changed, the successors' columns are void
                bw->w[5] += (unsigned long long)(g - gi);
                gi = g = 0;
            }
            m = m_new;
        }
    }
    *m_io = m;
    return f;
}

// control_plus_kernel's row (steps 1-3 and 5 of DESIGN.md §8l; a change there is made here too) around the group walk, once per
// width.  The workgroups are persistent: each takes learners from the ticket until none is left.  cpw_rows_kernel
// (kb_control_plus_wide.hip) is this kernel with the heavy learners' exit behind the head: a change here is made there too.
template <int W>
__global__ __launch_bounds__(256, 2) void control_plus_batch_kernel(CtlBatchArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    __shared__ BatchLds<W> bs;
    const KbDev& D = A.C.D;
    const KbState& K = A.C.K;
    double* kfA = A.arena + (size_t)blockIdx.x * 2 * (size_t)W * (size_t)A.max_m;
    double* dsA = kfA + (size_t)W * (size_t)A.max_m;
    BatchWork bw;
#pragma unroll
    for (int q = 0; q < 8; ++q) bw.w[q] = 0;
    for (;;) {
        __syncthreads();  // (the previous learner's readers of sm, pre and bs are done)
        if (threadIdx.x == 0) bs.task = atomicAdd(&A.ticket[0], 1);
        __syncthreads();
        const int task = bs.task;
        if (task >= A.T) break;
        const int env = task / D.S, s = task - env * D.S;
        const int dt = task;  // (per-replica dictionaries only: the task names the dictionary too)
        const uint64_t* sh = shells_of(D, K, dt);
        const int d = D.dims[s] + 1, n = D.n_prbs;
        int m = K.m[dt];
        const int act = A.C.action[task];
        const int y = A.C.labels[task] == 1 ? 1 : -1;
        stage_state(D, A.C.state, env, s, d, sm);
        if ((int)threadIdx.x == d - 1) sm.x[d - 1] = (double)act / (double)n;
        __syncthreads();
        for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);

        // ---- update_control's first predict, its decision and its bookkeeping: control_plus_kernel's
        double f0 = 0.0;
        if (m > 0) f0 = predict_column_steps<false>(D, K, sh, d, m, sm.x, pre, sm);
        const int y_pred = fit_decide(K, task, env, s, m, &f0, sm);
        if (threadIdx.x < 64) (void)control_bookkeeping(D, K, task, env, s, m, (double)y_pred, y, A.C.hits, sm);

        // ---- sample augmentation, in the reference's order, group by group
        const int a0 = y > 0 ? act : 0, a1 = y > 0 ? n : act;
        FitCounts c = {0, 0, 0, 0};
        int row_mist = 0, row_grow = 0, row_matvec = 0;
        const double f = plus_group_walk<W>(D, K, dt, task, env, s, sh, d, y, a0, a1, &m, pre, sm, bs, kfA, dsA, A.max_m, &c, &row_mist,
                                            &row_grow, &row_matvec, &bw);
        c.samples = (unsigned long long)(a1 - a0 + 1);
        c.mistakes = (unsigned long long)row_mist;
        c.insertions = (unsigned long long)row_grow;
        if (threadIdx.x == 0) {
            K.m[dt] = m;
            fit_epilogue(K, task, f, A.work, &c);
            K.fver[task] = -1;
            if (row_matvec) atomicAdd(&K.hv_work[6], (unsigned long long)row_matvec);
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (bw.w[q]) atomicAdd(&A.bwork[q], bw.w[q]);
        // the last workgroup to leave sets the ticket back for the next launch (every other one has drawn its last ticket)
        __threadfence();
        if (atomicAdd(&A.ticket[1], 1) == (int)gridDim.x - 1) {
            atomicExch(&A.ticket[0], 0);
            atomicExch(&A.ticket[1], 0);
        }
    }
}

}  // namespace kb

static void kb_arena_release(kb_arena_scratch* a) {
    if (a->d) (void)hipFree(a->d);
    a->d = nullptr;
    a->bytes = 0;
}

static uint64_t kb_control_plus_batch_bytes(const kb_handle* k, int32_t width, int32_t max_landmarks) {
    const uint64_t arenas = (uint64_t)(k->T < KB_CPB_ARENAS ? k->T : KB_CPB_ARENAS);
    return KB_CPB_HEAD + arenas * 2 * (uint64_t)width * (uint64_t)max_landmarks * sizeof(double);
}

// ---- what the setters of the grouped walks share (kb_set_control_plus_batch, kb_set_fit_steps_batch, kb_set_control_plus_wide)

// a width: 0, 2, 4 or 8 (`shares`: what the candidates of a group share, in the caller's words)
static int kb_check_width(kb_handle* k, const char* who, int32_t width, const char* shares) {
    if (width != 0 && width != 2 && width != 4 && width != 8) {
        k->err = std::string(who) + ": width = " + std::to_string(width) + " (0: the candidates one by one, the default; 2, 4 or 8: that many " +
                 shares + ")";
        return RS_EINVAL;
    }
    return RS_OK;
}

// the largest dictionary an arena holds: a multiple of 64, at least 64 and at most the handle's capacity
static int kb_check_max_landmarks(kb_handle* k, const char* who, int32_t max_landmarks) {
    if (max_landmarks < 64 || max_landmarks % 64 != 0 || max_landmarks > k->D.cap) {
        k->err = std::string(who) + ": max_landmarks = " + std::to_string(max_landmarks) +
                 " (a multiple of 64, at least 64 and at most the handle's capacity, " + std::to_string(k->D.cap) + ")";
        return RS_EINVAL;
    }
    return RS_OK;
}

// the scratch `s` of the handle at (width, max_landmarks): whatever runs on the stream still uses the arenas, so the stream is
// waited for; the scratch is freed, and allocated again unless the width is 0, when either number changes; the counters and the
// ticket start over.  All device scratch is allocated here -- the first launch may be inside a stream capture.
static int kb_arena_set(kb_handle* k, kb_arena_scratch* s, int32_t width, int32_t max_landmarks) {
    HIPCHK(k, hipStreamSynchronize(k->stream));
    if (s->width != width || s->max != max_landmarks) {
        kb_arena_release(s);
        s->width = 0;
        s->max = 0;
        if (width) {
            const uint64_t bytes = kb_control_plus_batch_bytes(k, width, max_landmarks);
            HIPCHK(k, hipMalloc((void**)&s->d, (size_t)bytes));
            s->bytes = bytes;
        }
    }
    if (s->d) HIPCHK(k, hipMemsetAsync(s->d, 0, KB_CPB_HEAD, k->stream));
    s->width = width;
    s->max = max_landmarks;
    return RS_OK;
}

// the scratch's part of a batch kernel's arguments (CtlBatchArgs, StepsBatchArgs) for a launch over T learners; -> the launch's grid
template <class Args>
static unsigned kb_arena_args(Args* a, const kb_arena_scratch& s, int32_t T) {
    a->bwork = (unsigned long long*)s.d;
    a->ticket = (int32_t*)(s.d + 64);
    a->arena = (double*)(s.d + KB_CPB_HEAD);
    a->max_m = s.max;
    a->T = T;
    return (unsigned)(T < KB_CPB_ARENAS ? T : KB_CPB_ARENAS);
}

// f(std::integral_constant<int, W>) for the instance W = 2, 4 or 8 of a set width
template <class F>
static void kb_by_width(int32_t width, F f) {
    if (width == 2)
        f(std::integral_constant<int, 2>());
    else if (width == 4)
        f(std::integral_constant<int, 4>());
    else
        f(std::integral_constant<int, 8>());
}

// the update phase of a closed-loop step in Projectron++ mode, grouped: one launch (launch_update_control times it as span 0)
static int launch_control_plus_batch(kb_handle* k, const kb::CtlArgs& c) {
    kb::CtlBatchArgs a;
    a.C = c;
    a.work = k->d_ctl_work;
    const unsigned grid = kb_arena_args(&a, k->cpb, k->T);
    kb_by_width(k->cpb.width, [&](auto w) {
        hipLaunchKernelGGL(kb::control_plus_batch_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, k->stream, a);
    });
    return RS_OK;
}

/* How the closed control loop's Projectron++ update phase walks a step's candidates (ranslice.h): host state of
   the handle beside control_plus. */
extern "C" int kb_set_control_plus_batch(kb_handle* k, int32_t width, int32_t max_landmarks) {
    if (!k) return RS_EINVAL;
    int rc = kb_check_width(k, "kb_set_control_plus_batch", width, "candidates share one pass over Kinv");
    if (rc == RS_OK && width != 0) rc = kb_check_max_landmarks(k, "kb_set_control_plus_batch", max_landmarks);
    if (rc == RS_OK) rc = kb_refuse_non_learning(k, "kb_set_control_plus_batch", "kb_update_control");
    if (rc != RS_OK) return rc;
    if (width == 0) max_landmarks = 0;
    HIPCHK(k, hipSetDevice(k->device));
    // (a captured loop carries the update phase and the arenas it was captured with; whatever runs on the stream still uses them)
    if (k->cpb.width != width || k->cpb.max != max_landmarks) {
        rc = kb_retire_graph(k);
        if (rc != RS_OK) return rc;
    }
    return kb_arena_set(k, &k->cpb, width, max_landmarks);
}

extern "C" int kb_get_control_plus_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes) {
    if (!k || !width || !max_landmarks || !scratch_bytes) return RS_EINVAL;
    *width = k->cpb.width;
    *max_landmarks = k->cpb.max;
    *scratch_bytes = k->cpb.bytes;
    return RS_OK;
}

extern "C" int kb_control_plus_batch_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    return kb_read_words(k, k->cpb.d, 8, work);
}
