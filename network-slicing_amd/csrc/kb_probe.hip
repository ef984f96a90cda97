// kb_probe.hip -- TEST BUILD ONLY (#included by rs_api.hip inside #ifdef RS_DEV; libranslice.so has none of it).
//
// Read-only accessors for a device test of the scoring chain: what kb_select_action (kb_kbrl.hip: bin_pass /
// select_bin_big_body, select_gemm_kernel, add_direct_terms, score_single) left on the device, stage by stage, so that every
// stage can be held to tests/scoring_mirror.py bit for bit (tests/test_gpu_scoring.py binds them).  Plain copies on
// the agent's stream after it has drained: no kernel is launched, nothing on the device is written.
//
//   kb_dev_get_scores  K.F [T][256], K.Wg [T][256] and K.fdirect [T] as the last kb_select_action left them (rows of learners
//                      with fewer than two landmarks hold no W: select_bin_* leaves them alone)
//   kb_dev_get_rows    the first min(m, max_m) entries of one learner's KB_ROW_D0 / KB_ROW_E / KB_ROW_IDX rows, its
//                      coefficients and last coordinates, and the handle's G table (256 entries)
//   kb_dev_get_chains  the newest-landmark heads (KB_HEAD entries), the first min(m, max_m) chain links of KB_ROW_IDX and the
//                      off-grid count of one learner's dictionary: what agents_finish_kernel (kb_agents.hip) rebuilds
//   kb_dev_get_update_rows  the first min(m, max_m) entries of one learner's KB_ROW_KF / KB_ROW_DS rows as the last
//                      Projectron.update left them (the kernel column and d* = Kinv K_f; after an insertion entry m - 1 of d* is
//                      its -1) and, optionally, the 128 partial sums of every stored tile of the first ceil(min(m, max_m) / 64)
//                      shells, tile (b_i, b_j) at 128 (b_i (b_i + 1) / 2 + b_j): dpart, then tpart (matvec_tri_tiles); a tile the
//                      last mat-vec did not cover holds whatever it held before (tests/test_gpu_update_chain.py)
//   kb_dev_get_shared_scores  shared handles: K.workF [S][KB_GEMM_KS][n_envs][256], the partial scores F = E Q of the eight parts
//                      of the landmarks, and K.workE [S][KB_GEMM_KS][n_envs], the largest E_j every replica met in each part, as
//                      the last kb_shared_scan / kb_select_action left them (shared_fgemm_kernel; a slice it did not score
//                      holds whatever it held before) (tests/test_gpu_shared_chain.py)
//   kb_dev_get_shared_apply  shared handles: the work areas of slice s as the last kb_shared_apply left them, laid out by
//                      the `budget` THAT call was given: KF and DS [budget][capr] (kernel columns and d* = Kinv k_f of the list,
//                      capr = the capacity rounded up to 64), A [budget][budget] the proposals' Gram block stored by column
//                      (A[q * budget + p] = k_p . d*_q, tiles tj <= ti only) and F0 [budget]
//   kb_dev_get_prune_grid  the workgroups (of 256 threads: four waves each) kb_prune / kb_shared_prune launch their downdate
//                      kernel with on this handle: host state of kb_prune_state, chosen by the first prune call the handle
//                      takes (RS_ESTATE before it).  With the plan's prefix sums it gives the stretch of every wave
//                      (tests/test_gpu_prune_chain.py)
//   kb_dev_set_prune_grid  the one entry point that changes host state: the downdate's grid of the handle's later prune calls, from
//                      1 to the grid the handle chose (never more than one co-resident round; RS_EINVAL outside, RS_ESTATE before
//                      the first prune call) -- few waves make stretches of many units on a handle of few dictionaries
// By-reference handles (kb_ref.hip) answer the first two: their scores are per task as everywhere (they keep no W: zeros), their rows are
// those of the store's dictionary the map names for (e, s) -- which no selection may ever have changed.
//
// And ONE entry point that launches a kernel, on buffers of its own (no handle): kb_dev_work_line runs the work-line helpers of
// kb_kbrl.hip on a line the test supplies (tests/test_gpu_work_line.py).
//   op 0, the walker   in = base[0 .. count], grid workgroups of 256 threads call walk_stretch; lane 0 of every wave counts a hit
//                      on, and writes its slot as the owner of, every unit it is handed: out0 = hits [total + 1], out1 = owner
//                      [total + 1] (-1: nobody's), total = base[count]; the last entry lies past the line
//   op 1, the scan     in = values [2][count]; one workgroup runs block_scan1024 in passes of 1,024 with a carry, as the plan
//                      kernels do: out0 = the inclusive sums of row 0 by the one-value scan [count], out1 = those of both rows
//                      by the two-value scan [2][count]

extern "C" int kb_dev_get_scores(kb_handle* k, double* F, double* W, int32_t* fdirect) {
    if (!k) return RS_EINVAL;
    if (k->D.shared) {
        k->err = "kb_dev_get_scores: shared-dictionary handles keep no per-learner scores";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const size_t T = (size_t)k->T;
    if (F) HIPCHK(k, hipMemcpyAsync(F, k->K.F, sizeof(double) * T * 256, hipMemcpyDeviceToHost, k->stream));
    if (W) HIPCHK(k, hipMemcpyAsync(W, k->K.Wg, sizeof(double) * T * 256, hipMemcpyDeviceToHost, k->stream));
    if (fdirect) HIPCHK(k, hipMemcpyAsync(fdirect, k->K.fdirect, sizeof(int32_t) * T, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    return RS_OK;
}

extern "C" int kb_dev_get_rows(kb_handle* k, int e, int s, int32_t max_m, int32_t* m_out, double* D0, double* E, int32_t* idx,
                               double* coeff, double* lam, double* gtab) {
    if (!k || e < 0 || e >= k->cfg.n_envs || s < 0 || s >= k->cfg.n_slices || max_m < 0) return RS_EINVAL;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    size_t dict = k->D.shared ? (size_t)s : (size_t)e * k->cfg.n_slices + s;
    kb_handle* const q = k;
    if (q->ref) {  // (from here on k is the handle whose pool holds the dictionary; errors are reported there and copied back)
        dict = (size_t)kb_ref_dict(q, dict);
        k = kb_ref_store(q);
        HIPCHK(q, hipStreamSynchronize(k->stream));
    }
    const int d = k->cfg.dims[s] + 1;
    int32_t m = 0;
    HIPCHK(q, hipMemcpy(&m, k->K.m + dict, sizeof m, hipMemcpyDeviceToHost));
    if (m_out) *m_out = m;
    if (gtab) HIPCHK(q, hipMemcpy(gtab, k->K.gtab, sizeof(double) * 256, hipMemcpyDeviceToHost));
    const int take = m < max_m ? m : max_m;
    if (take <= 0) return RS_OK;
    const int nch = (take + KB_CH - 1) / KB_CH;
    if (nch > k->D.max_shells) {
        q->err = "kb_dev_get_rows: more landmarks than the shell table holds";
        return RS_ESTATE;
    }
    std::vector<uint64_t> sh((size_t)nch);
    HIPCHK(q, hipMemcpy(sh.data(), k->K.shell + dict * (size_t)k->D.max_shells, sizeof(uint64_t) * (size_t)nch, hipMemcpyDeviceToHost));
    std::vector<double> page(KB_VEC);
    for (int b = 0; b < nch; ++b) {
        if (sh[b] == 0 || sh[b] + KB_VEC > k->D.pool_doubles) {  // (a shell the dictionary's size promises but the table lacks)
            q->err = "kb_dev_get_rows: shell table entry out of the pool";
            return RS_ESTATE;
        }
        HIPCHK(q, hipMemcpy(page.data(), k->K.pool + sh[b], sizeof(double) * KB_VEC, hipMemcpyDeviceToHost));
        const int cnt = take - KB_CH * b < KB_CH ? take - KB_CH * b : KB_CH;
        const int32_t* ix = (const int32_t*)(page.data() + KB_ROW_IDX * KB_CH);
        for (int l = 0; l < cnt; ++l) {
            const int j = KB_CH * b + l;
            if (D0) D0[j] = page[KB_ROW_D0 * KB_CH + l];
            if (E) E[j] = page[KB_ROW_E * KB_CH + l];
            if (idx) idx[j] = ix[l];
            if (coeff) coeff[j] = page[KB_ROW_CO * KB_CH + l];
            if (lam) lam[j] = page[(d - 1) * KB_CH + l];
        }
    }
    return RS_OK;
}

extern "C" int kb_dev_get_chains(kb_handle* k, int e, int s, int32_t max_m, int32_t* m_out, int32_t* head, int32_t* link, int32_t* offgrid) {
    if (!k || e < 0 || e >= k->cfg.n_envs || s < 0 || s >= k->cfg.n_slices || max_m < 0) return RS_EINVAL;
    if (k->ref || k->D.shared) {
        k->err = "kb_dev_get_chains: a handle that owns one dictionary per learner only";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const size_t dict = (size_t)e * k->cfg.n_slices + s;
    int32_t m = 0;
    HIPCHK(k, hipMemcpy(&m, k->K.m + dict, sizeof m, hipMemcpyDeviceToHost));
    if (m_out) *m_out = m;
    if (head) HIPCHK(k, hipMemcpy(head, k->K.head + dict * KB_HEAD, sizeof(int32_t) * KB_HEAD, hipMemcpyDeviceToHost));
    if (offgrid) HIPCHK(k, hipMemcpy(offgrid, k->K.offgrid + dict, sizeof(int32_t), hipMemcpyDeviceToHost));
    const int take = m < max_m ? m : max_m;
    if (take <= 0 || !link) return RS_OK;
    const int nch = (take + KB_CH - 1) / KB_CH;
    if (nch > k->D.max_shells) {
        k->err = "kb_dev_get_chains: more landmarks than the shell table holds";
        return RS_ESTATE;
    }
    std::vector<uint64_t> sh((size_t)nch);
    HIPCHK(k, hipMemcpy(sh.data(), k->K.shell + dict * (size_t)k->D.max_shells, sizeof(uint64_t) * (size_t)nch, hipMemcpyDeviceToHost));
    for (int b = 0; b < nch; ++b) {
        if (sh[b] == 0 || sh[b] + KB_VEC > k->D.pool_doubles) {
            k->err = "kb_dev_get_chains: shell table entry out of the pool";
            return RS_ESTATE;
        }
        const int cnt = take - KB_CH * b < KB_CH ? take - KB_CH * b : KB_CH;
        HIPCHK(k, hipMemcpy(link + KB_CH * b, (const int32_t*)(k->K.pool + sh[b] + KB_ROW_IDX * KB_CH) + 64, sizeof(int32_t) * (size_t)cnt,
                            hipMemcpyDeviceToHost));
    }
    return RS_OK;
}

extern "C" int kb_dev_get_update_rows(kb_handle* k, int e, int s, int32_t max_m, int32_t* m_out, double* kf, double* ds, double* parts) {
    if (!k || e < 0 || e >= k->cfg.n_envs || s < 0 || s >= k->cfg.n_slices || max_m < 0) return RS_EINVAL;
    if (k->ref || k->D.shared || k->D.tri != 1) {
        k->err = "kb_dev_get_update_rows: a handle that owns one dictionary per learner, with its Kinv, only";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const size_t dict = (size_t)e * k->cfg.n_slices + s;
    int32_t m = 0;
    HIPCHK(k, hipMemcpy(&m, k->K.m + dict, sizeof m, hipMemcpyDeviceToHost));
    if (m_out) *m_out = m;
    const int take = m < max_m ? m : max_m;
    if (take <= 0) return RS_OK;
    const int nch = (take + KB_CH - 1) / KB_CH;
    if (nch > k->D.max_shells) {
        k->err = "kb_dev_get_update_rows: more landmarks than the shell table holds";
        return RS_ESTATE;
    }
    std::vector<uint64_t> sh((size_t)nch);
    HIPCHK(k, hipMemcpy(sh.data(), k->K.shell + dict * (size_t)k->D.max_shells, sizeof(uint64_t) * (size_t)nch, hipMemcpyDeviceToHost));
    for (int b = 0; b < nch; ++b) {
        if (sh[b] == 0 || sh[b] + kb::kb_shell_doubles(b, 1) > k->D.pool_doubles) {
            k->err = "kb_dev_get_update_rows: shell table entry out of the pool";
            return RS_ESTATE;
        }
        const int cnt = take - KB_CH * b < KB_CH ? take - KB_CH * b : KB_CH;
        const double* page = k->K.pool + sh[b];
        if (kf) HIPCHK(k, hipMemcpy(kf + KB_CH * b, page + KB_ROW_KF * KB_CH, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost));
        if (ds) HIPCHK(k, hipMemcpy(ds + KB_CH * b, page + KB_ROW_DS * KB_CH, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost));
        if (parts)  // (the partial sums of the shell's b + 1 tiles lie behind them, in the order of the tiles)
            HIPCHK(k, hipMemcpy(parts + (size_t)128 * ((size_t)b * (b + 1) / 2), page + KB_VEC + (size_t)(b + 1) * KB_TILE,
                                sizeof(double) * 128 * (size_t)(b + 1), hipMemcpyDeviceToHost));
    }
    return RS_OK;
}

extern "C" int kb_dev_get_shared_scores(kb_handle* k, double* F_parts, double* E_parts) {
    if (!k) return RS_EINVAL;
    if (!k->D.shared) {
        k->err = "kb_dev_get_shared_scores: shared-dictionary handles only (kb_dev_get_scores answers the others)";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const size_t n = (size_t)k->cfg.n_slices * KB_GEMM_KS * (size_t)k->cfg.n_envs;
    if (F_parts) HIPCHK(k, hipMemcpy(F_parts, k->K.workF, sizeof(double) * n * 256, hipMemcpyDeviceToHost));
    if (E_parts) HIPCHK(k, hipMemcpy(E_parts, k->K.workE, sizeof(double) * n, hipMemcpyDeviceToHost));
    return RS_OK;
}

extern "C" int kb_dev_get_shared_apply(kb_handle* k, int s, int32_t budget, double* KF, double* DS, double* A, double* F0) {
    if (!k || s < 0 || s >= k->cfg.n_slices || budget <= 0 || budget > k->budget_cap) return RS_EINVAL;
    if (!k->D.shared) {
        k->err = "kb_dev_get_shared_apply: shared-dictionary handles only";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    const size_t capr = (size_t)kb::kb_capr(k->cfg.capacity), b = (size_t)budget;
    const double* kf = k->K.workb + (size_t)s * 2 * b * capr;  // (the offsets of shared_cols_kernel / shared_gram_kernel)
    if (KF) HIPCHK(k, hipMemcpy(KF, kf, sizeof(double) * b * capr, hipMemcpyDeviceToHost));
    if (DS) HIPCHK(k, hipMemcpy(DS, kf + b * capr, sizeof(double) * b * capr, hipMemcpyDeviceToHost));
    if (A) HIPCHK(k, hipMemcpy(A, k->K.workg + (size_t)s * b * b, sizeof(double) * b * b, hipMemcpyDeviceToHost));
    if (F0) HIPCHK(k, hipMemcpy(F0, k->K.workf + (size_t)s * b, sizeof(double) * b, hipMemcpyDeviceToHost));
    return RS_OK;
}

extern "C" int kb_dev_get_prune_grid(kb_handle* k, int32_t* grid) {
    if (!k || !grid) return RS_EINVAL;
    if (!k->prune) {
        k->err = "kb_dev_get_prune_grid: the handle has taken no prune call yet (the first one chooses the grid)";
        return RS_ESTATE;
    }
    *grid = (int32_t)k->prune->grid;
    return RS_OK;
}

extern "C" int kb_dev_set_prune_grid(kb_handle* k, int32_t grid) {
    if (!k) return RS_EINVAL;
    if (!k->prune) {
        k->err = "kb_dev_set_prune_grid: the handle has taken no prune call yet (the first one chooses the grid)";
        return RS_ESTATE;
    }
    if (grid < 1 || grid > k->prune->grid_most) {
        k->err = "kb_dev_set_prune_grid: grid " + std::to_string(grid) + " is outside 1 .. " + std::to_string(k->prune->grid_most) + " (one co-resident round)";
        return RS_EINVAL;
    }
    k->prune->grid = grid;
    return RS_OK;
}

namespace kb {

__global__ __launch_bounds__(1024) void work_line_probe_kernel(int op, const long long* in, int count, void* out0, void* out1) {
    if (op == 0) {
        int32_t *hits = (int32_t*)out0, *owner = (int32_t*)out1;
        walk_stretch(in, count, [&](int slot, long long a, long long b) {
            if ((threadIdx.x & 63) == 0)
                for (long long u = a; u < b; ++u) {
                    atomicAdd(&hits[in[slot] + u], 1);
                    owner[in[slot] + u] = slot;
                }
        });
        return;
    }
    __shared__ long long sc1[1][1024], sc2[2][1024];
    long long *one = (long long*)out0, *two = (long long*)out1;
    long long carry1 = 0, carry2[2] = {0, 0};
    for (int b0 = 0; b0 < count; b0 += 1024) {
        const int i = b0 + (int)threadIdx.x;
        long long v1[1] = {i < count ? in[i] : 0};
        long long v2[2] = {v1[0], i < count ? in[count + i] : 0};
        block_scan1024(v1, sc1);
        block_scan1024(v2, sc2);
        if (i < count) {
            one[i] = carry1 + v1[0];
            two[i] = carry2[0] + v2[0];
            two[count + i] = carry2[1] + v2[1];
        }
        carry1 += sc1[0][1023];
        carry2[0] += sc2[0][1023];
        carry2[1] += sc2[1][1023];
    }
}

}  // namespace kb

// the line and the sizes are checked here, the kernel trusts them: base[0] = 0, no step down, at most 2^24 units; out0 / out1 hold
// what the op writes (above).  Values of the scan: any int64 whose sums stay in range.
extern "C" int kb_dev_work_line(int device, int op, const int64_t* in, int32_t count, int32_t grid, void* out0, void* out1) {
    if ((op != 0 && op != 1) || !in || count < 1 || count > (1 << 20) || !out0 || !out1) return RS_EINVAL;
    size_t in_bytes = sizeof(int64_t) * 2 * (size_t)count, out0_bytes = sizeof(int64_t) * (size_t)count, out1_bytes = 2 * out0_bytes;
    if (op == 0) {
        if (grid < 1 || grid > 1024 || in[0] != 0) return RS_EINVAL;
        for (int32_t i = 0; i < count; ++i)
            if (in[i + 1] < in[i]) return RS_EINVAL;
        if (in[count] > ((int64_t)1 << 24)) return RS_EINVAL;
        in_bytes = sizeof(int64_t) * ((size_t)count + 1);
        out0_bytes = out1_bytes = sizeof(int32_t) * ((size_t)in[count] + 1);  // (and one entry past the line, which nobody may touch)
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return RS_EHIP;
    void *d_in = nullptr, *d_0 = nullptr, *d_1 = nullptr;
    int rc = RS_EHIP;
    do {
        if (hipMalloc(&d_in, in_bytes) != hipSuccess || hipMalloc(&d_0, out0_bytes) != hipSuccess || hipMalloc(&d_1, out1_bytes) != hipSuccess) break;
        if (hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemset(d_0, 0, out0_bytes) != hipSuccess || hipMemset(d_1, op == 0 ? 0xff : 0, out1_bytes) != hipSuccess) break;
        hipLaunchKernelGGL(kb::work_line_probe_kernel, dim3(op == 0 ? (unsigned)grid : 1u), dim3(op == 0 ? 256 : 1024), 0, 0, op,
                           (const long long*)d_in, (int)count, d_0, d_1);
        if (hipGetLastError() != hipSuccess) break;
        if (hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out0, d_0, out0_bytes, hipMemcpyDeviceToHost) != hipSuccess) break;
        if (hipMemcpy(out1, d_1, out1_bytes, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = RS_OK;
    } while (0);
    if (d_in) (void)hipFree(d_in);
    if (d_0) (void)hipFree(d_0);
    if (d_1) (void)hipFree(d_1);
    if (hipDeviceSynchronize() != hipSuccess) rc = RS_EHIP;
    return rc;
}
