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
// By-reference handles (kb_ref.hip) answer the first two: their scores are per task as everywhere (they keep no W: zeros), their rows are
// those of the store's dictionary the map names for (e, s) -- which no selection may ever have changed.

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
