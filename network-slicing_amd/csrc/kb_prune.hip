// kb_prune.hip -- budgeted dictionaries: kb_prune removes landmarks with an exact downdate of Kinv.
// #included by rs_api.hip after kb_fork.hip: it uses the agent handle and changes none of its kernels.
// The removal rule stands ONCE, here, as device functions over a storage policy (KinvTri: the lower block triangle of a
// per-replica dictionary; KinvFull: both triangles of a shared one).  kb_shared_prune (kb_shared_prune.hip) and the online budget
// (kb_online_prune.hip) instantiate them and share the host sequence below.
//
// The rule.  Write P = Kinv of the live landmarks, c their coefficients.  While a dictionary holds more than `target`
// landmarks, one landmark leaves:
//   1. r = argmin_j (c_j c_j) / P[j][j] over the live landmarks, the lowest j on a tie (P[j][j]: the stored diagonal);
//   2. p = P[:, r], q = P[r][r];
//   3. c_i = c_i + c_r * ((-p_i) / q)            for every survivor i            (the best approximation of c_r k(l_r, .)
//                                                                                  by the survivors; its squared error is c_r^2 / q)
//   4. P[i][j] = P[i][j] - (p_i * p_j) / q       for every survivor pair          (the survivors' inverse Gram matrix: a Schur
//                                                                                  complement, so the downdate is exact)
//   5. landmark m - 1 moves into slot r (unless r = m - 1): its rows of the vector page and row / column m - 1 of Kinv;
//   6. slot m - 1 and row / column m - 1 of Kinv are cleared to zeros;  7. m -= 1.
// Operation order of 3 and 4, as written: one negation, one division, one product, one addition; one product, one division,
// one subtraction (-ffp-contract=off: nothing fuses).  p_i p_j = p_j p_i, so Kinv stays symmetric bit for bit, and no sum is
// formed anywhere: the result does not depend on the launch, on the stretch a wave takes, on which other dictionaries are
// pruned by the same call, or on the storage -- a shared dictionary comes out as its unshared copy does.
//
// A call advances every listed dictionary (m > target) by one removal per round, in three kernels:
//   prune_choose_kernel    a workgroup per listed dictionary: the argmin over a (key bits, index) pair, then column r of Kinv
//                          gathered ONCE into the dictionary's d* row (a scratch row of the vector pages: every Projectron
//                          update writes it before it reads it) and the coefficients of step 3.  The downdate's waves then read
//                          p from coalesced rows, and none of them reads the column while another rewrites it.
//   prune_downdate_kernel  step 4, the hot path: the stored tiles of all listed dictionaries laid end to end by
//                          prune_plan_kernel (block_scan1024), an equal stretch per wave (walk_stretch; units of sixteen rows:
//                          8 KB read, 8 KB written, 16-byte accesses), the shape of heavy_rank1_kernel and its helpers (kb_kbrl.hip).
//   prune_move_kernel      steps 5-7.
// and prune_finish_kernel once per touched dictionary: the chains, the off-grid count, the version, the predict cache.
//
// The chains.  finish_update leaves, per dictionary, head[a] = the LARGEST slot j whose grid index is a (-1: none) and, in
// the link word of every landmark, the next smaller slot with the same grid index (-1: none): links strictly decrease along
// a chain.  Off-grid landmarks (index -1) carry link -1 and are counted in K.offgrid.  Today the chains have writers only
// (finish_update) and travel through kb_fork and the checkpoints; prune_chains rebuilds them from the index row so that the
// invariant holds for whoever reads them next.
//
// What does not travel.  The pruned counters live outside the handle's saved regions (checkpoints keep their size; kb_reset,
// kb_load_state and kb_fork restart them).  Shells are kept: growing back allocates nothing.

#define KB_PRUNE_MIN 64  // the smallest target: one shell, clear of the float32 arithmetic of a single-landmark dictionary
#define KB_FLAG_PRUNE_REFUSED 32  // the online budget's sticky bit of a replica's flag word (kb_online_prune.hip)

namespace kb {

struct PruneArgs {
    KbDev D;
    KbState K;
    int32_t target, n_dict;
    int32_t* list;     // [n_dict] the dictionaries with m > target, in increasing order (prune_list)
    int32_t* vict;     // by list place: the round's victim r
    double* q;         //                P[r][r]
    int32_t* stat;     //                0 active, 1 at the target, 2 refused untouched, 3 stopped after some removals
    int32_t* removed;  //                removals of this call
    long long* base;   // [listed + 1] prefix sums of the downdate's units (prune_plan)
    long long* pruned; // [n_dict] removals since kb_reset
    unsigned long long* info;  // [0] listed, [1] most removals any dictionary needs, [2] refused untouched, [3] removed in all,
                               // [4] stopped after some removals; since kb_reset (kb_prune_restart): [5] the downdate's units
                               // that hold rows, [6] its launches with work
};

// Kinv[i][j] of a dictionary that stores the lower block triangle; diagonal tiles hold both of their halves
__device__ __forceinline__ double* prune_at(const KbState& K, const uint64_t* sh, int i, int j) {  // block of i >= block of j
    return kinv_tile_lo(K, sh, i >> 6, j >> 6) + (i & 63) * 64 + (j & 63);
}
__device__ __forceinline__ double prune_get(const KbState& K, const uint64_t* sh, int i, int j) {
    return (i >> 6) >= (j >> 6) ? *prune_at(K, sh, i, j) : *prune_at(K, sh, j, i);
}
__device__ __forceinline__ void prune_set(const KbState& K, const uint64_t* sh, int i, int j, double v) {
    const int bi = i >> 6, bj = j >> 6;
    if (bi >= bj) *prune_at(K, sh, i, j) = v;
    if (bi <= bj) *prune_at(K, sh, j, i) = v;
}
// Kinv[i][j] of a dictionary that stores both block triangles (KbDev.tri == 0; kinv_tile), each the exact transpose of the other
__device__ __forceinline__ double* sprune_at(const KbState& K, const uint64_t* sh, int i, int j) {
    return kinv_tile(K, sh, i >> 6, j >> 6) + (i & 63) * 64 + (j & 63);
}

// The storage policies: exactly what the rule's functions below do differently on the two storages.
//   diag       P[j][j] (diagonal tiles lie where they do in the triangle)
//   column     entry i of column r, as choose gathers it
//   move_entry P[r][k] = P[k][r] = P[m-1][k] for one k other than r and m - 1;  move_diag: P[r][r] = P[m-1][m-1]
//   clear_last row and column m - 1 to zeros (bl, ll: the block and the row within it of m - 1, the last live landmark: its
//              block is the last one stored), by the whole workgroup
//   tiles, full_row_tiles   the stored tiles of nb blocks, and those of them in full block rows (all but the last)
//   tile_of, tile           the tile (bi, bj) of unit-tile tb of the work line, and its address
struct KinvTri {
    static __device__ __forceinline__ double diag(const KbState& K, const uint64_t* sh, int j) { return *prune_at(K, sh, j, j); }
    static __device__ __forceinline__ double column(const KbState& K, const uint64_t* sh, int i, int r) { return prune_get(K, sh, i, r); }
    static __device__ __forceinline__ void move_entry(const KbState& K, const uint64_t* sh, int r, int last, int k) {
        prune_set(K, sh, r, k, prune_get(K, sh, last, k));
    }
    static __device__ __forceinline__ void move_diag(const KbState& K, const uint64_t* sh, int r, int last) {
        prune_set(K, sh, r, r, prune_get(K, sh, last, last));
    }
    // row m - 1 of every tile of its block row (all 64 columns), column m - 1 of the diagonal tile
    static __device__ __forceinline__ void clear_last(const KbState& K, const uint64_t* sh, int bl, int ll) {
        const int tid = threadIdx.x;
        for (int e = tid; e < (bl + 1) * 64; e += 256) kinv_tile_lo(K, sh, bl, e >> 6)[ll * 64 + (e & 63)] = 0.0;
        if (tid < 64) kinv_tile_lo(K, sh, bl, bl)[tid * 64 + ll] = 0.0;
    }
    static __device__ __forceinline__ long long tiles(long long nb) { return nb * (nb + 1) / 2; }
    static __device__ __forceinline__ long long full_row_tiles(long long nb) { return (nb - 1) * nb / 2; }
    static __device__ __forceinline__ void tile_of(int tb, int nb, int* bi, int* bj) { tri_tile_of(tb, bi, bj); }
    static __device__ __forceinline__ double* tile(const KbState& K, const uint64_t* sh, int bi, int bj) { return kinv_tile_lo(K, sh, bi, bj); }
};
struct KinvFull {
    static __device__ __forceinline__ double diag(const KbState& K, const uint64_t* sh, int j) { return *sprune_at(K, sh, j, j); }
    // column r is read as ROW r: thread i reads entry i of it -- coalesced, and the same bits (the transpose is exact)
    static __device__ __forceinline__ double column(const KbState& K, const uint64_t* sh, int i, int r) { return *sprune_at(K, sh, r, i); }
    // row m - 1 is read (it lies in the lower tiles: coalesced, and the bits KinvTri reads); row r and column r are written,
    // each in the tiles of its own side of the diagonal
    static __device__ __forceinline__ void move_entry(const KbState& K, const uint64_t* sh, int r, int last, int k) {
        const double v = *sprune_at(K, sh, last, k);
        *sprune_at(K, sh, r, k) = v;
        *sprune_at(K, sh, k, r) = v;
    }
    static __device__ __forceinline__ void move_diag(const KbState& K, const uint64_t* sh, int r, int last) {
        *sprune_at(K, sh, r, r) = *sprune_at(K, sh, last, last);
    }
    static __device__ __forceinline__ void clear_last(const KbState& K, const uint64_t* sh, int bl, int ll) {
        for (int e = threadIdx.x; e < (bl + 1) * 64; e += 256) {
            kinv_tile(K, sh, bl, e >> 6)[ll * 64 + (e & 63)] = 0.0;  // row m - 1, all 64 columns of every tile of its block row
            kinv_tile(K, sh, e >> 6, bl)[(e & 63) * 64 + ll] = 0.0;  // column m - 1, all 64 rows of every tile of its block column
        }
    }
    static __device__ __forceinline__ long long tiles(long long nb) { return nb * nb; }
    static __device__ __forceinline__ long long full_row_tiles(long long nb) { return (nb - 1) * nb; }
    static __device__ __forceinline__ void tile_of(int tb, int nb, int* bi, int* bj) {  // row-major (rank1_units with tri == 0)
        *bi = tb / nb;
        *bj = tb - *bi * nb;
    }
    static __device__ __forceinline__ double* tile(const KbState& K, const uint64_t* sh, int bi, int bj) { return kinv_tile(K, sh, bi, bj); }
};

// the dictionaries over the target, in increasing order: one workgroup, a contiguous run per thread (integer sums: the list
// is the same whatever the launch).  info[0] = listed, info[1] = most = the largest excess (thread 0 may read it on return)
__device__ __forceinline__ void prune_list(const PruneArgs& a, int (&part)[1024], int& most) {
    const int t = threadIdx.x, n = a.n_dict, per = (n + 1023) / 1024;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    if (t == 0) most = 0;
    int cnt = 0, mx = 0;
    for (int i = i0; i < i1; ++i) {
        const int over = a.K.m[i] - a.target;
        if (over > 0) {
            ++cnt;
            mx = over > mx ? over : mx;
        }
    }
    part[t] = cnt;
    __syncthreads();
    if (mx > 0) atomicMax(&most, mx);
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int at = t ? part[t - 1] : 0;
    for (int i = i0; i < i1; ++i)
        if (a.K.m[i] > a.target) {
            a.list[at] = i;
            a.stat[at] = 0;
            a.removed[at] = 0;
            ++at;
        }
    if (t == 0) {
        a.info[0] = (unsigned long long)part[1023];
        a.info[1] = (unsigned long long)most;
    }
}

__global__ __launch_bounds__(1024) void prune_list_kernel(PruneArgs a) {
    __shared__ int part[1024];
    __shared__ int most;
    prune_list(a, part, most);
    if (threadIdx.x == 0) a.info[2] = a.info[3] = a.info[4] = 0ull;
}

// Steps 1-3 for list place li, by a workgroup of 256; every branch is uniform over it.  The key (c_j c_j) / P[j][j] is
// non-negative, so its bit pattern orders as the value does: the argmin runs over the pair (key bits, j) in lexicographic
// order and the lowest j wins a tie.  A diagonal entry that is not finite and positive (or a coefficient that is not finite)
// takes the dictionary out of the call: untouched when it is met in the first round -- every live diagonal entry is examined
// there --, left as the completed removals made it otherwise.  FLAG (the online budget, which cannot answer RS_ESTATE from the
// device): the replica's flag word gets KB_FLAG_PRUNE_REFUSED then.
template <class St, bool FLAG>
__device__ __forceinline__ void prune_choose(const PruneArgs& a, int li, unsigned long long (&wkey)[4], int (&widx)[4], int (&wbad)[4]) {
    const KbState& K = a.K;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (a.stat[li] != 0) return;
    const int dict = a.list[li];
    const int m = K.m[dict];
    if (m <= a.target) {
        if (tid == 0) a.stat[li] = 1;
        return;
    }
    const uint64_t* sh = shells_of(a.D, K, dict);
    unsigned long long best = ~0ull;
    int bidx = 0x7fffffff, bad = 0;
    for (int j = tid; j < m; j += 256) {
        const double c = *vec_at(K, sh, KB_ROW_CO, j);
        const double pjj = St::diag(K, sh, j);
        if (!(pjj > 0.0) || !__builtin_isfinite(pjj) || !__builtin_isfinite(c)) {
            bad = 1;
        } else {
            const unsigned long long key = (unsigned long long)__double_as_longlong((c * c) / pjj);
            if (key < best) {  // (j increases: the first of equal keys stays)
                best = key;
                bidx = j;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long ok = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        bad |= __shfl_xor(bad, o);
        if (ok < best || (ok == best && oi < bidx)) {
            best = ok;
            bidx = oi;
        }
    }
    if (lane == 0) {
        wkey[wv] = best;
        widx[wv] = bidx;
        wbad[wv] = bad;
    }
    __syncthreads();
    for (int w = 0; w < 4; ++w) {  // (every thread walks the four waves: the same winner everywhere)
        bad |= wbad[w];
        if (w == 0 || wkey[w] < best || (wkey[w] == best && widx[w] < bidx)) {
            best = wkey[w];
            bidx = widx[w];
        }
    }
    if (bad) {
        if (tid == 0) {
            a.stat[li] = a.removed[li] > 0 ? 3 : 2;
            if (FLAG) atomicOr(&K.err[dict / a.D.S], KB_FLAG_PRUNE_REFUSED);  // (one agent per replica: dictionary = task)
        }
        return;
    }
    const int r = bidx;
    const double q = St::diag(K, sh, r), cr = *vec_at(K, sh, KB_ROW_CO, r);
    if (tid == 0) {
        a.vict[li] = r;
        a.q[li] = q;
    }
    for (int i = tid; i < m; i += 256) {
        const double p = St::column(K, sh, i, r);
        *vec_at(K, sh, KB_ROW_DS, i) = p;
        if (i != r) {
            double* ci = vec_at(K, sh, KB_ROW_CO, i);
            *ci = *ci + cr * ((-p) / q);
        }
    }
}

__global__ __launch_bounds__(256) void prune_choose_kernel(PruneArgs a) {
    __shared__ unsigned long long wkey[4];
    __shared__ int widx[4], wbad[4];
    prune_choose<KinvTri, false>(a, blockIdx.x, wkey, widx, wbad);
}

// the downdate's work line: 4 units of sixteen rows per stored tile of every active dictionary, end to end.  The byte count
// (kb_get_prune_work) takes only the units that hold rows: all four of a full block row's tiles, ceil(rows / 16) of the last one's.
template <class St>
__device__ __forceinline__ void prune_plan(const PruneArgs& a, long long (&sc)[1][1024], unsigned long long& filled) {
    const int count = (int)a.info[0], t = threadIdx.x;
    long long carry = 0;
    if (t == 0) filled = 0ull;
    __syncthreads();
    for (int b0 = 0; b0 < count; b0 += 1024) {
        const int li = b0 + t;
        long long w = 0;
        if (li < count && a.stat[li] == 0) {
            const long long m = a.K.m[a.list[li]], nb = (m + 63) >> 6;
            w = St::tiles(nb) * 4;
            atomicAdd(&filled, (unsigned long long)(St::full_row_tiles(nb) * 4 + nb * ((m - 64 * (nb - 1) + 15) >> 4)));
        }
        long long inc[1] = {w};
        block_scan1024(inc, sc);
        if (li < count) a.base[li] = carry + inc[0] - w;
        carry += sc[0][1023];
    }
    if (t == 0) {
        a.base[count] = carry;
        if (carry > 0) {  // (the roofline's byte count: units of 8 KB read + 8 KB written, launches with work)
            a.info[5] += filled;
            a.info[6] += 1ull;
        }
    }
}

__global__ __launch_bounds__(1024) void prune_plan_kernel(PruneArgs a) {
    __shared__ long long sc[1][1024];
    __shared__ unsigned long long filled;
    prune_plan<KinvTri>(a, sc, filled);
}

// Step 4 on units [u0, u1) of one dictionary of m live landmarks: unit u = rows 16 (u & 3) .. + 15 of stored tile u >> 2
// (St::tile_of).  16-byte accesses as in rank1_units: a lane owns two neighbouring columns of one row, a half-wave a whole
// 512-byte row, one load instruction two rows, eight of them in flight per lane.  p comes from the d* row (prune_choose):
// the 64 row operands as one coalesced load, handed out with v_readlane, the two column operands as one 16-byte load.
// Entries at or beyond m are neither read into the result nor written: vacated rows and columns stay exact zeros.  On full
// storage both triangles are downdated directly and the lower one is not mirrored: p_i p_j = p_j p_i gives the upper entry the
// same bits, no tile is transposed, and the kernel stays bound by the bytes it streams (twice the triangle's).
template <class St>
__device__ __forceinline__ void prune_units(const KbState& K, const uint64_t* sh, int m, double q, int u0, int u1) {
    const int lane = threadIdx.x & 63, nb = (m + 63) >> 6;
    for (int u = u0; u < u1; ++u) {
        const int tb = u >> 2, r0 = (u & 3) * 16;
        int bi, bj;
        St::tile_of(tb, nb, &bi, &bj);
        const int rows = m - 64 * bi < 64 ? m - 64 * bi : 64;
        if (r0 >= rows) continue;  // (wave-uniform)
        const int h = lane >> 5, cp = (lane & 31) * 2;
        const int j0 = 64 * bj + cp;
        kb_f64x2* T = (kb_f64x2*)(St::tile(K, sh, bi, bj) + cp);
        const double pi_v = vec_page(K, sh, bi)[KB_ROW_DS * KB_CH + lane];
        const kb_f64x2 pj = *(const kb_f64x2*)(vec_page(K, sh, bj) + KB_ROW_DS * KB_CH + cp);
        kb_f64x2 old[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = r0 + 2 * k + h;
            kb_f64x2 v = {0.0, 0.0};
            if (r < rows && j0 < m) v = T[r * 32];
            old[k] = v;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int r = r0 + 2 * k + h;
            const double pa = readlane_f64(pi_v, r0 + 2 * k), pb = readlane_f64(pi_v, r0 + 2 * k + 1);
            const double pi = h ? pb : pa;
            kb_f64x2 nv;
            nv[0] = old[k][0] - (pi * pj[0]) / q;
            nv[1] = old[k][1] - (pi * pj[1]) / q;
            if (r < rows) {
                if (j0 + 1 < m)
                    T[r * 32] = nv;
                else if (j0 < m)
                    ((double*)&T[r * 32])[0] = nv[0];
            }
        }
    }
}

template <class St>
__device__ __forceinline__ void prune_downdate(const PruneArgs& a) {
    const int count = (int)a.info[0];
    if (count == 0) return;
    walk_stretch(a.base, count, [&](int slot, long long u0, long long u1) {
        const int dict = a.list[slot];
        prune_units<St>(a.K, shells_of(a.D, a.K, dict), a.K.m[dict], a.q[slot], (int)u0, (int)u1);
    });
}

__global__ __launch_bounds__(256) void prune_downdate_kernel(PruneArgs a) { prune_downdate<KinvTri>(a); }

// Steps 5-7 for list place li, by a workgroup of 256.  Row / column m - 1 of Kinv go to row / column r: for every k other than
// r and m - 1, P[r][k] = P[k][r] = P[m-1][k], and P[r][r] = P[m-1][m-1] -- reads of row m - 1 only, writes to row / column r
// only, so one pass without an order.  The landmark's rows of the vector page follow: the coordinates (all sixteen rows, or,
// for an eMBB dictionary, rows 0..10 and the float32 copy of the ten state coordinates that lives in rows 11..15), the
// coefficient, the grid index (the link is rebuilt by prune_chains).  Then the vacated slot and row / column m - 1 of Kinv are cleared.
template <class St>
__device__ __forceinline__ void prune_move(const PruneArgs& a, int li) {
    const KbState& K = a.K;
    const int tid = threadIdx.x;
    if (a.stat[li] != 0) return;
    const int dict = a.list[li];
    const uint64_t* sh = shells_of(a.D, K, dict);
    const int m = K.m[dict], r = a.vict[li], last = m - 1;
    const bool f32 = a.D.dims[dict % a.D.S] == 10;
    double* Pl = vec_page(K, sh, last >> 6);
    const int ll = last & 63;
    if (r != last) {
        for (int k = tid; k < m; k += 256)
            if (k != r && k != last) St::move_entry(K, sh, r, last, k);
        if (tid == 0) St::move_diag(K, sh, r, last);
        double* Pr = vec_page(K, sh, r >> 6);
        const int lr = r & 63;
        if (tid >= 64 && tid < 64 + (f32 ? KB_ROW_F32 : KB_ROW_CO)) Pr[(tid - 64) * KB_CH + lr] = Pl[(tid - 64) * KB_CH + ll];
        if (f32 && tid >= 128 && tid < 138)
            ((float*)(Pr + KB_ROW_F32 * KB_CH))[(tid - 128) * KB_CH + lr] = ((const float*)(Pl + KB_ROW_F32 * KB_CH))[(tid - 128) * KB_CH + ll];
        if (tid == 192) Pr[KB_ROW_CO * KB_CH + lr] = Pl[KB_ROW_CO * KB_CH + ll];
        if (tid == 193) ((int32_t*)(Pr + KB_ROW_IDX * KB_CH))[lr] = ((const int32_t*)(Pl + KB_ROW_IDX * KB_CH))[ll];
    }
    __syncthreads();  // (row m - 1 and slot m - 1 have been read)
    St::clear_last(K, sh, last >> 6, ll);
    if (tid >= 64 && tid < 64 + (f32 ? KB_ROW_F32 : KB_ROW_CO)) Pl[(tid - 64) * KB_CH + ll] = 0.0;
    if (f32 && tid >= 128 && tid < 138) ((float*)(Pl + KB_ROW_F32 * KB_CH))[(tid - 128) * KB_CH + ll] = 0.0f;
    if (tid >= 192 && tid < 192 + 5) Pl[(KB_ROW_CO + tid - 192) * KB_CH + ll] = 0.0;  // coefficient, D0, E, K_f, d*
    if (tid == 200) {
        int32_t* ix = (int32_t*)(Pl + KB_ROW_IDX * KB_CH);
        ix[ll] = 0;
        ix[64 + ll] = 0;
    }
    if (tid == 0) {
        K.m[dict] = last;
        a.removed[li] += 1;
    }
}

__global__ __launch_bounds__(256) void prune_move_kernel(PruneArgs a) { prune_move<KinvTri>(a, blockIdx.x); }

// What every finishing of a touched dictionary begins with, by a workgroup of 256: the chains from scratch (thread a walks
// the slots upwards and links the landmarks of grid index a: head = the largest slot, links strictly decreasing) and the
// off-grid count, which is complete in `off` behind the caller's next barrier.
__device__ __forceinline__ void prune_chains(const PruneArgs& a, int dict, int& off) {
    const KbState& K = a.K;
    const int tid = threadIdx.x;
    const uint64_t* sh = shells_of(a.D, K, dict);
    const int m = K.m[dict];
    if (tid == 0) off = 0;
    __syncthreads();
    int prev = -1, cnt = 0;
    for (int j = 0; j < m; ++j) {
        int32_t* ix = idx_at(K, sh, j);
        if (ix[0] == tid) {
            ix[64] = prev;
            prev = j;
        }
    }
    K.head[(size_t)dict * KB_HEAD + tid] = prev;
    for (int j = tid; j < m; j += 256) {
        int32_t* ix = idx_at(K, sh, j);
        if (ix[0] < 0) {
            ix[64] = -1;
            ++cnt;
        }
    }
    if (cnt) atomicAdd(&off, cnt);
}

// Once per listed dictionary, after the rounds.  Touched ones: the chains and the off-grid count, the version (stored select
// scores are stale), the predict cache guards (a kb_update without a new kb_predict answers RS_ESTATE), the pruned counter.
// f32bad, the control state, the tie-break stream and the flag word stay.
__global__ __launch_bounds__(256) void prune_finish_kernel(PruneArgs a) {
    __shared__ int off;
    const KbState& K = a.K;
    const int li = blockIdx.x, tid = threadIdx.x;
    const int n = a.removed[li], st = a.stat[li];
    if (tid == 0 && st == 2) atomicAdd(&a.info[2], 1ull);
    if (tid == 0 && st == 3) atomicAdd(&a.info[4], 1ull);
    if (n == 0) return;
    const int dict = a.list[li];
    prune_chains(a, dict, off);
    __syncthreads();
    if (tid == 0) {
        K.offgrid[dict] = off;
        K.ver[dict] += 1;
        K.fver[dict] = -1;   // (one agent per replica: dictionary = task)
        K.f_last[dict] = 0.0;
        K.m_last[dict] = -1;
        K.kf_owner[dict] = -1;
        a.pruned[dict] += (long long)n;
        atomicAdd(&a.info[3], (unsigned long long)n);
    }
}

}  // namespace kb

// what the prune calls and the online budget keep behind a handle, outside its saved regions (created by the first of them)
struct kb_prune_state {
    int32_t *d_list = nullptr, *d_vict = nullptr, *d_stat = nullptr, *d_removed = nullptr;
    double* d_q = nullptr;
    long long *d_base = nullptr, *d_pruned = nullptr;
    unsigned long long* d_info = nullptr;
    unsigned long long* h_info = nullptr;  // pinned
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int grid = 2048, grid_most = 2048;     // the downdate's workgroups: one co-resident round of them, and that round's size
    EventSpans spans;                      // kernel timing: a pair per launch of the three phases, kind 0 choose, 1 downdate, 2 move
};

typedef void (*kb_prune_kernel)(kb::PruneArgs);

static void kb_prune_release(kb_handle* k) {
    kb_prune_state* p = k->prune;
    if (!p) return;
    void* ds[] = {p->d_list, p->d_vict, p->d_stat, p->d_removed, p->d_q, p->d_base, p->d_pruned, p->d_info};
    for (void* d : ds)
        if (d) (void)hipFree(d);
    if (p->h_info) (void)hipHostFree(p->h_info);
    if (p->ev_in) (void)hipEventDestroy(p->ev_in);
    if (p->ev_out) (void)hipEventDestroy(p->ev_out);
    p->spans.release();
    delete p;
    k->prune = nullptr;
}

// kb_reset, kb_load_state, kb_fork (into this handle): the pruned counters start over, on the handle's stream
static void kb_prune_restart(kb_handle* k) {
    if (k->prune && k->prune->d_pruned) (void)hipMemsetAsync(k->prune->d_pruned, 0, sizeof(long long) * (size_t)k->n_dict, k->stream);
    if (k->prune && k->prune->d_info) (void)hipMemsetAsync(k->prune->d_info + 5, 0, sizeof(unsigned long long) * 2, k->stream);
}

// downdate: the handle's downdate kernel (a handle is of one storage for life); its occupancy sizes the grid
static int kb_prune_prepare(kb_handle* k, kb_prune_kernel downdate) {
    if (k->prune) return RS_OK;
    kb_prune_state* p = new kb_prune_state();
    k->prune = p;  // (kb_destroy frees whatever was allocated)
    const size_t nd = (size_t)k->n_dict;
    HIPCHK(k, hipMalloc((void**)&p->d_list, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_vict, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_stat, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_removed, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_q, sizeof(double) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_base, sizeof(long long) * (nd + 1)));
    HIPCHK(k, hipMalloc((void**)&p->d_pruned, sizeof(long long) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_info, sizeof(unsigned long long) * 8));
    HIPCHK(k, hipHostMalloc((void**)&p->h_info, sizeof(unsigned long long) * 8, hipHostMallocDefault));
    HIPCHK(k, hipMemsetAsync(p->d_pruned, 0, sizeof(long long) * nd, k->stream));
    HIPCHK(k, hipMemsetAsync(p->d_info, 0, sizeof(unsigned long long) * 8, k->stream));
    HIPCHK(k, hipEventCreateWithFlags(&p->ev_in, hipEventDisableTiming));
    HIPCHK(k, hipEventCreateWithFlags(&p->ev_out, hipEventDisableTiming));
    int cus = 256, b = 0;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k->device);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, downdate, 256, 0) == hipSuccess && b > 0) p->grid = p->grid_most = b * cus;
    return RS_OK;
}

// the argument block of every prune kernel, from the handle and k->prune; info: the caller's counter words
static kb::PruneArgs kb_prune_args(kb_handle* k, int32_t target, unsigned long long* info) {
    const kb_prune_state* p = k->prune;
    kb::PruneArgs a;
    memset(&a, 0, sizeof a);
    a.D = k->D;
    a.K = k->K;
    a.target = target;
    a.n_dict = k->n_dict;
    a.list = p->d_list;
    a.vict = p->d_vict;
    a.q = p->d_q;
    a.stat = p->d_stat;
    a.removed = p->d_removed;
    a.base = p->d_base;
    a.pruned = p->d_pruned;
    a.info = info;
    return a;
}

// The host sequence of kb_prune and kb_shared_prune, behind their refusals: `who` names the caller in messages, kn = its
// choose, plan, downdate, move and finish kernels, tail (may be null) enqueues what the caller adds behind the finish launch.
static int kb_prune_run(kb_handle* k, const char* who, int32_t target, uint64_t* removed_total, const kb_prune_kernel (&kn)[5],
                        int (*tail)(kb_handle*)) {
    HIPCHK(k, hipSetDevice(k->device));
    int rc = kb_prune_prepare(k, kn[2]);
    if (rc != RS_OK) return rc;
    kb_prune_state* p = k->prune;
    // behind whatever is queued on either of the handle's streams (the resident loop joins the agent's stream itself)
    if (k->side && (rc = stream_after(k, &p->ev_in, k->side, k->stream)) != RS_OK) return rc;
    const kb::PruneArgs a = kb_prune_args(k, target, p->d_info);
    hipLaunchKernelGGL(kb::prune_list_kernel, dim3(1), dim3(1024), 0, k->stream, a);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(p->h_info, p->d_info, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const unsigned listed = (unsigned)p->h_info[0];
    const int rounds = (int)p->h_info[1];
    if (listed == 0) return RS_OK;
    p->spans.on = k->spans.on;  // an event pair around one launch of a phase, when kernel timing is on (kb_set_kernel_timing)
    for (int r = 0; r < rounds; ++r) {
        hipEvent_t e;
        HIPCHK(k, p->spans.begin(k->stream, 0, &e));
        hipLaunchKernelGGL(kn[0], dim3(listed), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        hipLaunchKernelGGL(kn[1], dim3(1), dim3(1024), 0, k->stream, a);
        HIPCHK(k, p->spans.begin(k->stream, 1, &e));
        hipLaunchKernelGGL(kn[2], dim3((unsigned)p->grid), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        HIPCHK(k, p->spans.begin(k->stream, 2, &e));
        hipLaunchKernelGGL(kn[3], dim3(listed), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
    }
    hipLaunchKernelGGL(kn[4], dim3(listed), dim3(256), 0, k->stream, a);
    HIPCHK(k, hipGetLastError());
    if (tail && (rc = tail(k)) != RS_OK) return rc;
    HIPCHK(k, hipMemcpyAsync(p->h_info, p->d_info, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, k->stream));
    if (k->side && (rc = stream_after(k, &p->ev_out, k->stream, k->side)) != RS_OK) return rc;
    HIPCHK(k, hipStreamSynchronize(k->stream));
    k->gemm_fresh = false;
    if (removed_total) *removed_total = (uint64_t)p->h_info[3];
    if (p->h_info[2] || p->h_info[4]) {
        k->err = std::string(who) + ": " + std::to_string(p->h_info[2] + p->h_info[4]) + " dictionaries hold a Kinv diagonal entry that is not finite and positive (" +
                 std::to_string(p->h_info[2]) + " left untouched, " + std::to_string(p->h_info[4]) + " stopped after completed removals); the others were pruned";
        return RS_ESTATE;
    }
    return RS_OK;
}

// the refusals kb_prune and kb_shared_prune share, and come first in both
static int kb_prune_target_ok(kb_handle* k, const char* who, int32_t target) {
    if (target < KB_PRUNE_MIN) {
        k->err = std::string(who) + ": target " + std::to_string(target) + " is below " + std::to_string(KB_PRUNE_MIN) + " landmarks (one shell is the floor)";
        return RS_EINVAL;
    }
    if (target > k->cfg.capacity) {
        k->err = std::string(who) + ": target " + std::to_string(target) + " exceeds the capacity " + std::to_string(k->cfg.capacity);
        return RS_EINVAL;
    }
    return RS_OK;
}

extern "C" int kb_prune(kb_handle* k, int32_t target, uint64_t* removed_total) {
    if (!k) return RS_EINVAL;
    if (removed_total) *removed_total = 0;
    const int rc = kb_prune_target_ok(k, "kb_prune", target);
    if (rc != RS_OK) return rc;
    if (k->D.shared) {
        k->err = "kb_prune: shared-dictionary handles are not supported";
        return RS_ESTATE;
    }
    if (k->ref) {
        k->err = "kb_prune: a by-reference handle (kb_deploy_ref) shares read-only dictionaries: prune the learning handle and deploy again";
        return RS_ESTATE;
    }
    if (k->frozen) {
        k->err = "kb_prune: an inference-only handle (kb_deploy) holds no Kinv: prune the learning handle and deploy again";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_prune: call kb_reset first";
        return RS_ESTATE;
    }
    const kb_prune_kernel kn[5] = {kb::prune_choose_kernel, kb::prune_plan_kernel, kb::prune_downdate_kernel, kb::prune_move_kernel,
                                   kb::prune_finish_kernel};
    return kb_prune_run(k, "kb_prune", target, removed_total, kn, nullptr);
}

extern "C" int kb_get_pruned(kb_handle* k, int64_t* removed) {
    if (!k || !removed) return RS_EINVAL;
    const size_t nd = (size_t)k->n_dict;
    if (!k->prune || !k->prune->d_pruned) {
        for (size_t i = 0; i < nd; ++i) removed[i] = 0;
        return RS_OK;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipMemcpyAsync(removed, k->prune->d_pruned, sizeof(int64_t) * nd, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    return RS_OK;
}

extern "C" int kb_get_prune_work(kb_handle* k, uint64_t work[2]) {
    if (!k || !work) return RS_EINVAL;
    work[0] = work[1] = 0;
    if (!k->prune || !k->prune->d_info) return RS_OK;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipMemcpyAsync(work, k->prune->d_info + 5, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    return RS_OK;
}

extern "C" int kb_prune_time_ms(kb_handle* k, double ms[3], int64_t n[3]) {
    if (!k || !ms || !n) return RS_EINVAL;
    for (int q = 0; q < 3; ++q) {
        ms[q] = 0.0;
        n[q] = 0;
    }
    kb_prune_state* p = k->prune;
    if (!p) return RS_OK;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    HIPCHK(k, p->spans.drain([&](int kind, double t) {
        ms[kind] += t;
        n[kind] += 1;
    }));
    return RS_OK;
}
