// kb_shared_prune.hip -- budgeted shared dictionaries: kb_shared_prune is kb_prune's removal (kb_prune.hip) on
// the storage a shared-dictionary handle has.  #included by rs_api.hip after kb_prune.hip: it uses that file's
// argument block, its list kernel and the state it keeps behind a handle, and changes none of its kernels.
//
// The rule, the operation order and -ffp-contract=off are kb_prune's, to the letter: per coefficient c_i + c_r * ((-p_i) / q),
// per entry P[i][j] - (p_i * p_j) / q, nothing summed.  So one dictionary comes out, bit for bit, as kb_prune leaves its unshared
// copy (kb_unshare): landmarks, slots, coefficients and the lower block triangle.  What differs is the storage.  A shared
// dictionary keeps BOTH block triangles of Kinv (KbDev.tri == 0; kinv_tile), each the exact transpose of the other:
//   prune_shared_choose_kernel    the argmin of prune_choose_kernel; column r is then read as ROW r -- coalesced, and the same bits;
//   prune_shared_plan_kernel      nb * nb * 4 units of sixteen rows per dictionary instead of the triangle's nb (nb + 1) / 2 * 4;
//   prune_shared_downdate_kernel  prune_units with rank1_units' tri == 0 indexing.  Both triangles are downdated directly and the
//                           lower one is not mirrored: p_i p_j = p_j p_i gives the upper entry the same bits, no tile is
//                           transposed, and the kernel stays bound by the bytes it streams (twice the triangle's);
//   prune_shared_move_kernel      row / column m - 1 to r and the clearing, in the tiles of both sides of the diagonal;
//   prune_shared_finish_kernel    one dictionary serves the n_envs tasks of its slice: the cached predict of every one of them is
//                           invalidated, where prune_finish_kernel has dictionary = task.
// Nothing depends on the rank of a handle or on its communicator: ranks that call kb_shared_prune with the same target at the
// same step of a run keep bit-identical dictionaries without a collective.

namespace kb {

// Kinv[i][j] of a dictionary that stores both block triangles
__device__ __forceinline__ double* sprune_at(const KbState& K, const uint64_t* sh, int i, int j) {
    return kinv_tile(K, sh, i >> 6, j >> 6) + (i & 63) * 64 + (j & 63);
}

// Steps 1-3: prune_choose_kernel's argmin over (key bits, slot) and its refusal of a diagonal entry that is not finite and
// positive, unchanged (diagonal tiles lie where they do in the triangle).  p = P[r][:]: thread i reads entry i of row r.
__global__ __launch_bounds__(256) void prune_shared_choose_kernel(PruneArgs a) {
    __shared__ unsigned long long wkey[4];
    __shared__ int widx[4], wbad[4];
    const KbState& K = a.K;
    const int li = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
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
        const double pjj = *sprune_at(K, sh, j, j);
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
        if (tid == 0) a.stat[li] = a.removed[li] > 0 ? 3 : 2;
        return;
    }
    const int r = bidx;
    const double q = *sprune_at(K, sh, r, r), cr = *vec_at(K, sh, KB_ROW_CO, r);
    if (tid == 0) {
        a.vict[li] = r;
        a.q[li] = q;
    }
    for (int i = tid; i < m; i += 256) {
        const double p = *sprune_at(K, sh, r, i);
        *vec_at(K, sh, KB_ROW_DS, i) = p;
        if (i != r) {
            double* ci = vec_at(K, sh, KB_ROW_CO, i);
            *ci = *ci + cr * ((-p) / q);
        }
    }
}

// the downdate's work line: 4 units of sixteen rows per tile of the nb x nb block square of every active dictionary, end to
// end.  The byte count (kb_get_prune_work) takes only the units that hold rows: all four of a full block row's tiles,
// ceil(rows / 16) of the last one's.
__global__ __launch_bounds__(1024) void prune_shared_plan_kernel(PruneArgs a) {
    __shared__ long long sc[1][1024];
    __shared__ unsigned long long filled;
    const int count = (int)a.info[0], t = threadIdx.x;
    long long carry = 0;
    if (t == 0) filled = 0ull;
    __syncthreads();
    for (int b0 = 0; b0 < count; b0 += 1024) {
        const int li = b0 + t;
        long long w = 0;
        if (li < count && a.stat[li] == 0) {
            const long long m = a.K.m[a.list[li]], nb = (m + 63) >> 6;
            w = nb * nb * 4;
            atomicAdd(&filled, (unsigned long long)((nb - 1) * nb * 4 + nb * ((m - 64 * (nb - 1) + 15) >> 4)));
        }
        long long inc[1] = {w};
        block_scan1024(inc, sc);
        if (li < count) a.base[li] = carry + inc[0] - w;
        carry += sc[0][1023];
    }
    if (t == 0) {
        a.base[count] = carry;
        if (carry > 0) {
            a.info[5] += filled;
            a.info[6] += 1ull;
        }
    }
}

// Step 4 on units [u0, u1) of one dictionary of m live landmarks: unit u = rows 16 (u & 3) .. + 15 of tile u >> 2 of the block
// square, row-major (rank1_units with tri == 0).  Accesses, operands and the expression are prune_units': 16-byte loads and
// stores, eight in flight per lane, the 64 row operands from the d* row by v_readlane, the two column operands one 16-byte
// load.  Entries at or beyond m are neither read into the result nor written.
__device__ __forceinline__ void sprune_units(const KbState& K, const uint64_t* sh, int m, double q, int u0, int u1) {
    const int lane = threadIdx.x & 63, nb = (m + 63) >> 6;
    for (int u = u0; u < u1; ++u) {
        const int tb = u >> 2, r0 = (u & 3) * 16;
        const int bi = tb / nb, bj = tb - bi * nb;
        const int rows = m - 64 * bi < 64 ? m - 64 * bi : 64;
        if (r0 >= rows) continue;  // (wave-uniform)
        const int h = lane >> 5, cp = (lane & 31) * 2;
        const int j0 = 64 * bj + cp;
        kb_f64x2* T = (kb_f64x2*)(kinv_tile(K, sh, bi, bj) + cp);
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

__global__ __launch_bounds__(256) void prune_shared_downdate_kernel(PruneArgs a) {
    const int count = (int)a.info[0];
    if (count == 0) return;
    walk_stretch(a.base, count, [&](int slot, long long u0, long long u1) {
        const int dict = a.list[slot];
        sprune_units(a.K, shells_of(a.D, a.K, dict), a.K.m[dict], a.q[slot], (int)u0, (int)u1);
    });
}

// Steps 5-7, a workgroup per active dictionary.  For every k other than r and m - 1, P[r][k] = P[k][r] = P[m-1][k], and
// P[r][r] = P[m-1][m-1]: row m - 1 is read (it lies in the lower tiles: coalesced, and the bits prune_move_kernel reads), row r
// and column r are written, each in the tiles of its own side of the diagonal -- reads of row m - 1 only, writes to row /
// column r only, so one pass without an order.  The landmark's rows of the vector page follow as in prune_move_kernel.  Then
// the vacated slot is cleared, row m - 1 in every tile of its block row and column m - 1 in every tile of its block column
// (m - 1 is the last live landmark: its block is the last one of the block square).
__global__ __launch_bounds__(256) void prune_shared_move_kernel(PruneArgs a) {
    const KbState& K = a.K;
    const int li = blockIdx.x, tid = threadIdx.x;
    if (a.stat[li] != 0) return;
    const int dict = a.list[li];
    const uint64_t* sh = shells_of(a.D, K, dict);
    const int m = K.m[dict], r = a.vict[li], last = m - 1;
    const bool f32 = a.D.dims[dict % a.D.S] == 10;
    double* Pl = vec_page(K, sh, last >> 6);
    const int ll = last & 63;
    if (r != last) {
        for (int k = tid; k < m; k += 256)
            if (k != r && k != last) {
                const double v = *sprune_at(K, sh, last, k);
                *sprune_at(K, sh, r, k) = v;
                *sprune_at(K, sh, k, r) = v;
            }
        if (tid == 0) *sprune_at(K, sh, r, r) = *sprune_at(K, sh, last, last);
        double* Pr = vec_page(K, sh, r >> 6);
        const int lr = r & 63;
        if (tid >= 64 && tid < 64 + (f32 ? KB_ROW_F32 : KB_ROW_CO)) Pr[(tid - 64) * KB_CH + lr] = Pl[(tid - 64) * KB_CH + ll];
        if (f32 && tid >= 128 && tid < 138)
            ((float*)(Pr + KB_ROW_F32 * KB_CH))[(tid - 128) * KB_CH + lr] = ((const float*)(Pl + KB_ROW_F32 * KB_CH))[(tid - 128) * KB_CH + ll];
        if (tid == 192) Pr[KB_ROW_CO * KB_CH + lr] = Pl[KB_ROW_CO * KB_CH + ll];
        if (tid == 193) ((int32_t*)(Pr + KB_ROW_IDX * KB_CH))[lr] = ((const int32_t*)(Pl + KB_ROW_IDX * KB_CH))[ll];
    }
    __syncthreads();  // (row m - 1 and slot m - 1 have been read)
    const int bl = last >> 6;
    for (int e = tid; e < (bl + 1) * 64; e += 256) {
        kinv_tile(K, sh, bl, e >> 6)[ll * 64 + (e & 63)] = 0.0;  // row m - 1, all 64 columns of every tile
        kinv_tile(K, sh, e >> 6, bl)[(e & 63) * 64 + ll] = 0.0;  // column m - 1, all 64 rows of every tile
    }
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

// Once per listed dictionary, after the rounds: prune_finish_kernel's chains, off-grid count (it decides gemm_applies: a
// dictionary whose last off-grid landmark left is scored on the wide path again), version and counters.  A shared dictionary is
// read by the n_envs tasks (replica, slice) of its slice: the cached predict of every one of them goes, and the K_f row
// belongs to nobody.
__global__ __launch_bounds__(256) void prune_shared_finish_kernel(PruneArgs a) {
    __shared__ int off;
    const KbState& K = a.K;
    const int li = blockIdx.x, tid = threadIdx.x;
    const int n = a.removed[li], st = a.stat[li];
    if (tid == 0 && st == 2) atomicAdd(&a.info[2], 1ull);
    if (tid == 0 && st == 3) atomicAdd(&a.info[4], 1ull);
    if (n == 0) return;
    const int dict = a.list[li];
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
    for (int e = tid; e < a.D.n_envs; e += 256) {  // the tasks of the slice
        const size_t task = (size_t)e * a.D.S + dict;
        K.fver[task] = -1;
        K.f_last[task] = 0.0;
        K.m_last[task] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        K.offgrid[dict] = off;
        K.ver[dict] += 1;
        K.kf_owner[dict] = -1;
        a.pruned[dict] += (long long)n;
        atomicAdd(&a.info[3], (unsigned long long)n);
    }
}

}  // namespace kb

extern "C" int kb_shared_prune(kb_handle* k, int32_t target, uint64_t* removed_total) {
    if (!k) return RS_EINVAL;
    if (removed_total) *removed_total = 0;
    if (target < KB_PRUNE_MIN) {
        k->err = "kb_shared_prune: target " + std::to_string(target) + " is below " + std::to_string(KB_PRUNE_MIN) + " landmarks (one shell is the floor)";
        return RS_EINVAL;
    }
    if (target > k->cfg.capacity) {
        k->err = "kb_shared_prune: target " + std::to_string(target) + " exceeds the capacity " + std::to_string(k->cfg.capacity);
        return RS_EINVAL;
    }
    if (!k->D.shared) {
        k->err = "kb_shared_prune: the handle is not a shared-dictionary handle (one agent per replica: kb_prune)";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_shared_prune: call kb_reset first";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_shared_prune: the handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    const bool first = !k->prune;
    int rc = kb_prune_prepare(k);
    if (rc != RS_OK) return rc;
    kb_prune_state* p = k->prune;
    if (first) {  // (kb_prune never runs on this handle: the one co-resident round is this file's downdate kernel's)
        int cus = 256, b = 0;
        p->grid = 2048;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k->device);
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kb::prune_shared_downdate_kernel, 256, 0) == hipSuccess && b > 0) p->grid = b * cus;
    }
    if (k->side && (rc = stream_after(k, &p->ev_in, k->side, k->stream)) != RS_OK) return rc;
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
    a.info = p->d_info;
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
        hipLaunchKernelGGL(kb::prune_shared_choose_kernel, dim3(listed), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        hipLaunchKernelGGL(kb::prune_shared_plan_kernel, dim3(1), dim3(1024), 0, k->stream, a);
        HIPCHK(k, p->spans.begin(k->stream, 1, &e));
        hipLaunchKernelGGL(kb::prune_shared_downdate_kernel, dim3((unsigned)p->grid), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        HIPCHK(k, p->spans.begin(k->stream, 2, &e));
        hipLaunchKernelGGL(kb::prune_shared_move_kernel, dim3(listed), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
    }
    hipLaunchKernelGGL(kb::prune_shared_finish_kernel, dim3(listed), dim3(256), 0, k->stream, a);
    HIPCHK(k, hipGetLastError());
    // What the shared mode derives from a dictionary is rebuilt by the next step, as after kb_share: Q (workq) by every launch of
    // the scoring product, F / E by it once gemm_fresh is off; the proposal cursors of an earlier round name candidates scored
    // against dictionaries that are gone.  Shells, flag words and the communicator stay as they are.
    const size_t T = (size_t)k->T, S = (size_t)k->cfg.n_slices;
    HIPCHK(k, hipMemsetAsync(k->d_cursor, 0xFF, sizeof(int32_t) * T, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_cstar, 0xFF, sizeof(int32_t) * T, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_counts, 0, sizeof(int32_t) * S, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_mcounts, 0, sizeof(int32_t) * S, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_taken, 0, sizeof(int32_t) * S, k->stream));
    HIPCHK(k, hipMemcpyAsync(p->h_info, p->d_info, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost, k->stream));
    if (k->side && (rc = stream_after(k, &p->ev_out, k->stream, k->side)) != RS_OK) return rc;
    HIPCHK(k, hipStreamSynchronize(k->stream));
    k->gemm_fresh = false;
    if (removed_total) *removed_total = (uint64_t)p->h_info[3];
    if (p->h_info[2] || p->h_info[4]) {
        k->err = "kb_shared_prune: " + std::to_string(p->h_info[2] + p->h_info[4]) + " dictionaries hold a Kinv diagonal entry that is not finite and positive (" +
                 std::to_string(p->h_info[2]) + " left untouched, " + std::to_string(p->h_info[4]) + " stopped after completed removals); the others were pruned";
        return RS_ESTATE;
    }
    return RS_OK;
}
