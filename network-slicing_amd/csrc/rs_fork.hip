// rs_fork.hip -- device-side replica fork (rs_fork) and the clairvoyant step built on it (rs_step_clairvoyant).
// #included by rs_api.hip after the handle and the step path: it uses both and changes neither.
//
// A replica's whole future is a function of its own slice of the state arrays: every random draw is keyed by the replica's
// seed and by counters held in that state (include/rs_philox.h), never by the replica's index in the batch.  Every per-replica
// array is laid out task-major (rs_device.h), so replica r's slice of it is one contiguous run of bytes_per_replica bytes at
// r * bytes_per_replica, and a fork is a gather of those runs.

#define RS_FORK_MAX 48  // regions a fork table can hold (RsState 21, MtcState 8, step outputs 6)

namespace rs {

struct ForkTable {
    const char* src[RS_FORK_MAX];
    char* dst[RS_FORK_MAX];
    uint32_t bpr[RS_FORK_MAX];  // bytes per replica: a multiple of 4 (16 for the wide path)
    int32_t n;
};

struct ForkArgs {
    ForkTable T;
    const int32_t* index;  // [n_dst] source replica of each destination replica, or null: the search's layout below
    int32_t n_dst;
    const int64_t* run_src;  // slot clock of the source
    int64_t* run_dst;
    // the search (index == null): destination b = i * C + k is candidate k of chunk replica i, a copy of source replica
    // c0 + min(i, cnt - 1); its action row is (a_0 .. a_{s-1}, k, 0 .. 0) from the source's action buffer, with k > R_s and
    // every padding replica (i >= cnt) given k = 0 / all zeros
    int32_t C, c0, cnt, s, n_act, n_prbs;
    const int32_t* acts_src;
    int32_t* acts_dst;
};

// One wave per destination replica, four to a workgroup; the wave walks the region table and copies the replica's run of each
// region with 16-byte vector loads and stores (four-byte ones for the regions of a few words per replica).
__global__ __launch_bounds__(256) void fork_gather_kernel(ForkArgs a) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= a.n_dst) return;
    int i = 0, k = 0, r;
    if (a.index) {
        r = a.index[j];
    } else {
        i = j / a.C;
        k = j - i * a.C;
        r = a.c0 + (i < a.cnt ? i : a.cnt - 1);
    }
    for (int e = 0; e < a.T.n; ++e) {
        const size_t bpr = a.T.bpr[e];
        const char* __restrict__ s = a.T.src[e] + (size_t)r * bpr;
        char* __restrict__ d = a.T.dst[e] + (size_t)j * bpr;
        if ((bpr & 15) == 0) {
            size_t o = (size_t)lane * 16;
            for (; o + 1024 < bpr; o += 2048) {  // two 16-byte loads in flight per lane
                const uint4 v0 = *(const uint4*)(s + o);
                const uint4 v1 = *(const uint4*)(s + o + 1024);
                *(uint4*)(d + o) = v0;
                *(uint4*)(d + o + 1024) = v1;
            }
            if (o < bpr) *(uint4*)(d + o) = *(const uint4*)(s + o);
        } else {
            for (size_t o = (size_t)lane * 4; o < bpr; o += 256) *(uint32_t*)(d + o) = *(const uint32_t*)(s + o);
        }
    }
    if (a.acts_dst && lane < a.n_act) {
        int v = 0;
        if (i < a.cnt) {
            const int32_t* row = a.acts_src + (size_t)r * a.n_act;
            if (lane < a.s) {
                v = row[lane];
            } else if (lane == a.s) {
                int used = 0;
                for (int q = 0; q < a.s; ++q) used += row[q];
                v = k <= a.n_prbs - used ? k : 0;
            }
        }
        a.acts_dst[(size_t)j * a.n_act + lane] = v;
    }
    if (j == 0 && lane == 0) a.run_dst[0] = a.run_src[0];
}

// One wave per chunk replica: candidate k <= R_s with the fewest violations of slice s, the smallest such k (with `widest`, the
// largest when every candidate violates); written into the searched handle's action buffer.  A capacity flag raised in any of the replica's candidates is kept in err_out.
__global__ __launch_bounds__(256) void clairvoyant_select_kernel(const int32_t* __restrict__ bviol, const int32_t* __restrict__ berr,
                                                                 int32_t C, int32_t c0, int32_t cnt, int32_t s, int32_t n_act,
                                                                 int32_t n_prbs, int32_t widest, int32_t* acts, int32_t* err_out) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= cnt) return;
    const int r = c0 + i;
    int used = 0;
    for (int q = 0; q < s; ++q) used += acts[(size_t)r * n_act + q];
    const int R = n_prbs - used;
    unsigned long long best = ~0ull;
    int err = 0;
    for (int k = lane; k <= R; k += 64) {
        const size_t b = (size_t)i * C + k;
        const uint32_t v = (uint32_t)bviol[b * n_act + s];
        // second key k, or (fallback "widest") n_prbs - k among candidates that all violate: one min-reduction either way
        const unsigned long long key = ((unsigned long long)v << 32) | (unsigned)(widest && v != 0u ? 0x10000 + n_prbs - k : k);
        best = key < best ? key : best;
        err |= berr[b];
    }
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(best, m);
        best = o < best ? o : best;
        err |= __shfl_xor(err, m);
    }
    if (lane == 0) {
        const unsigned lo = (unsigned)(best & 0xffffffffull);
        acts[(size_t)r * n_act + s] = (int32_t)(lo >= 0x10000u ? 0x10000 + n_prbs - (int)lo : (int)lo);
        if (err) err_out[r] |= err;
    }
}

}  // namespace rs

// Every device array behind a handle is a region of its saved state (h->regions, filled by dalloc).  The fork names each one:
// copied per replica, per replica but not copied, or handle-wide.  A region it does not know is a refusal, so that an array
// added to the state later cannot be left out of forks unnoticed.
static int fork_table(rs_handle* dst, rs_handle* src, bool with_actions, rs::ForkTable* T) {
    const RsState &a = src->st, &b = dst->st;
    const rs::MtcState &ma = src->mst, &mb = dst->mst;
    const size_t E = (size_t)src->cfg.n_embb, M = (size_t)src->cfg.n_mmtc, U = E * RS_GROUP;
    const size_t MD = M * MTC_DEV_MAX, MQ = M * (size_t)src->mst.cap;
    struct Ent {
        const void* s;
        void* d;
        size_t bpr;
    };
    const Ent copied[] = {
        {a.t_n_ue, b.t_n_ue, 4 * E}, {a.t_cbr_at, b.t_cbr_at, 4 * E}, {a.t_vbr_at, b.t_vbr_at, 4 * E},
        {a.t_ctr, b.t_ctr, 4 * E}, {a.t_serial, b.t_serial, 4 * E},
        {a.u_queue, b.u_queue, 8 * U}, {a.u_th, b.u_th, 8 * U}, {a.u_nominal, b.u_nominal, 8 * U},
        {a.u_hold_at, b.u_hold_at, 4 * U}, {a.u_e_snr, b.u_e_snr, 4 * U}, {a.u_findex, b.u_findex, 4 * U},
        {a.u_bits, b.u_bits, 4 * U}, {a.u_prbs, b.u_prbs, 4 * U}, {a.u_vbr_at, b.u_vbr_at, 4 * U},
        {a.u_ctr, b.u_ctr, 4 * U}, {a.u_serial, b.u_serial, 4 * U}, {a.u_flags, b.u_flags, 4 * U},
        {a.u_burst, b.u_burst, 2 * U * RS_BURSTS},
        {a.seeds, b.seeds, 8}, {a.err, b.err, 4},
        {ma.n_users, mb.n_users, 4 * M}, {ma.s_start, mb.s_start, 8 * M}, {ma.s_rep, mb.s_rep, 8 * M},
        {ma.dev_next, mb.dev_next, 4 * MD}, {ma.dev_period, mb.dev_period, 4 * MD}, {ma.dev_rep, mb.dev_rep, 4 * MD},
        {ma.q_rep, mb.q_rep, 4 * MQ}, {ma.q_start, mb.q_start, 4 * MQ},
        // the outputs of the last step (no step reads them; copied so that rs_fetch / rs_get_info show the source's)
        {src->d_obs, dst->d_obs, 4 * (size_t)src->n_vars}, {src->d_reward, dst->d_reward, 8},
        {src->d_labels, dst->d_labels, 4 * (size_t)src->n_slices}, {src->d_viol, dst->d_viol, 4 * (size_t)src->n_slices},
        {src->d_info, dst->d_info, 80 * (size_t)src->n_ran},
        {src->d_actions, dst->d_actions, with_actions ? 4 * (size_t)src->n_slices : 0},
    };
    // per replica, not copied: the scheduling key (t_cost) and the diagnostic counters, which no result depends on; handle-wide:
    // the constants, the pointer table, the slot clock (written by the gather), order / replay scratch, profiles
    const void* skipped[] = {a.t_cost, src->d_counters, src->ddev, src->d_st, src->d_run, src->d_counter_sum, src->d_sections,
                             src->d_redo, src->d_order, src->d_oslot, src->d_ohist, src->d_pace};
    const size_t n_src = (size_t)src->cfg.n_envs, n_dst = (size_t)dst->cfg.n_envs;
    auto region_bytes = [](const rs_handle* h, const void* p) -> size_t {
        for (auto& r : h->regions)
            if (r.first == p) return r.second;
        return 0;
    };
    for (auto& r : src->regions) {
        bool known = false;
        for (const Ent& e : copied) known = known || e.s == r.first;
        for (const void* p : skipped) known = known || p == r.first;
        if (!known) {
            src->err = "rs_fork: a state region of the handle is not classified for forking";
            return RS_ESTATE;
        }
    }
    T->n = 0;
    for (const Ent& e : copied) {
        if (e.bpr == 0 || !e.s) continue;
        if (T->n == RS_FORK_MAX || (e.bpr & 3) != 0 || e.bpr > 0xffffffffull || region_bytes(src, e.s) < e.bpr * n_src ||
            region_bytes(dst, e.d) < e.bpr * n_dst) {
            src->err = "rs_fork: internal region layout mismatch";
            return RS_ESTATE;
        }
        T->src[T->n] = (const char*)e.s;
        T->dst[T->n] = (char*)e.d;
        T->bpr[T->n] = (uint32_t)e.bpr;
        T->n++;
    }
    return RS_OK;
}

// rs_cfg_hash with n_envs masked: the configuration two handles must share to fork between them
static uint64_t fork_cfg_hash(const rs_handle* h) {
    rs_config c = h->cfg;
    c.n_envs = 0;
    return fnv1a(&c, sizeof c);
}

static int fork_check(rs_handle* dst, rs_handle* src, const char* who) {
    if (fork_cfg_hash(dst) != fork_cfg_hash(src)) {
        dst->err = std::string(who) + ": the handles' configurations differ (beyond n_envs)";
        return RS_EINVAL;
    }
    if (!src->is_reset) {
        dst->err = std::string(who) + ": the source was never reset";
        return RS_ESTATE;
    }
    if (dst->device != src->device) {
        dst->err = std::string(who) + ": the handles live on different devices";
        return RS_ESTATE;
    }
    if (!fading_ready(src) || !fading_ready(dst) || dst->fad_hash != src->fad_hash) {
        dst->err = std::string(who) + ": the handles' fading tables are not identical";
        return RS_ESTATE;
    }
    return RS_OK;
}

// dst takes src's host-side clock and becomes reset; its counters restart
static int fork_adopt(rs_handle* dst, const rs_handle* src) {
    if (dst->cfg.n_embb == 0)  // (rs_reset uploads the constants of a handle without fading tables)
        HIPCHK(dst, hipMemcpyAsync(dst->ddev, &dst->hdev, sizeof(RsDev), hipMemcpyHostToDevice, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_counters, 0, sizeof(uint64_t) * 4 * (dst->n_tasks ? dst->n_tasks : 1), dst->stream));
    dst->clock = src->clock;
    dst->steps = src->steps;
    dst->is_reset = true;
    return RS_OK;
}

extern "C" int rs_fork(rs_handle* dst, rs_handle* src, const int32_t* src_index) {
    if (!dst || !src || !src_index) return RS_EINVAL;
    if (lanes_close(dst) != RS_OK) return RS_EHIP;
    if (lanes_close(src) != RS_OK) return RS_EHIP;
    if (dst == src) {
        dst->err = "rs_fork: source and destination must be different handles";
        return RS_EINVAL;
    }
    int rc = fork_check(dst, src, "rs_fork");
    if (rc != RS_OK) return rc;
    const int n_dst = dst->cfg.n_envs;
    for (int j = 0; j < n_dst; ++j)
        if (src_index[j] < 0 || src_index[j] >= src->cfg.n_envs) {
            dst->err = "rs_fork: source index " + std::to_string(src_index[j]) + " of destination replica " + std::to_string(j) +
                       " out of range";
            return RS_EINVAL;
        }
    rs::ForkArgs a;
    memset(&a, 0, sizeof a);
    if ((rc = fork_table(dst, src, true, &a.T)) != RS_OK) {
        dst->err = src->err;
        return rc;
    }
    HIPCHK(dst, hipSetDevice(dst->device));
    drop_graph(dst);
    if ((rc = ensure_event(dst, &dst->ev_fork_in)) != RS_OK || (rc = ensure_event(dst, &dst->ev_fork_out)) != RS_OK) return rc;
    if (!dst->d_fork_idx) HIPCHK(dst, hipMalloc((void**)&dst->d_fork_idx, sizeof(int32_t) * n_dst));
    // the index goes up from a pinned buffer of dst's, so that the copy waits for nothing on the host; a previous fork's copy
    // out of it must have finished first
    if (!dst->h_fork_idx) HIPCHK(dst, hipHostMalloc((void**)&dst->h_fork_idx, sizeof(int32_t) * n_dst, hipHostMallocDefault));
    else HIPCHK(dst, hipEventSynchronize(dst->ev_fork_out));
    memcpy(dst->h_fork_idx, src_index, sizeof(int32_t) * n_dst);
    // after src's queued work (its finalize_kernel has joined its side streams); src's next step waits for the gather
    if ((rc = stream_after(dst, &dst->ev_fork_in, src->stream, dst->stream)) != RS_OK) return rc;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, sizeof(int32_t) * n_dst, hipMemcpyHostToDevice,
                               dst->stream));
    a.index = dst->d_fork_idx;
    a.n_dst = n_dst;
    a.run_src = src->d_run;
    a.run_dst = dst->d_run;
    hipLaunchKernelGGL(rs::fork_gather_kernel, dim3((unsigned)((n_dst + 3) / 4)), dim3(256), 0, dst->stream, a);
    HIPCHK(dst, hipGetLastError());
    if ((rc = fork_adopt(dst, src)) != RS_OK) return rc;
    return stream_after(dst, &dst->ev_fork_out, dst->stream, src->stream);
}

static void fork_release(rs_handle* h) {
    if (h->la) {
        rs_destroy(h->la);
        h->la = nullptr;
    }
    if (h->d_la_err) (void)hipFree(h->d_la_err);
    if (h->d_fork_idx) (void)hipFree(h->d_fork_idx);
    if (h->h_fork_idx) (void)hipHostFree(h->h_fork_idx);
    h->h_fork_idx = nullptr;
    h->d_la_err = nullptr;
    h->d_fork_idx = nullptr;
    if (h->ev_fork_in) (void)hipEventDestroy(h->ev_fork_in);
    if (h->ev_fork_out) (void)hipEventDestroy(h->ev_fork_out);
    h->ev_fork_in = h->ev_fork_out = nullptr;
}

// ------------------------------------------------------------------ clairvoyant step

extern "C" int rs_set_lookahead(rs_handle* h, int max_branches) {
    if (!h) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    if (max_branches < 0 || (max_branches > 0 && max_branches < h->cfg.n_prbs + 1)) {
        h->err = "rs_set_lookahead: max_branches must be 0 or at least n_prbs + 1";
        return RS_EINVAL;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->la) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        rs_destroy(h->la);
        h->la = nullptr;
    }
    h->la_max = max_branches;
    return RS_OK;
}

extern "C" int rs_set_clairvoyant_fallback(rs_handle* h, int mode) {
    if (!h || mode < 0 || mode > 1) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    h->la_widest = mode;
    return RS_OK;
}

// The branch handle: h's configuration with chunk * (n_prbs + 1) replicas, reading h's fading tables (not copying them)
static int ensure_branches(rs_handle* h) {
    if (h->la) return RS_OK;
    const long long C = h->cfg.n_prbs + 1;
    // the step kernels index the per-UE burst table of a task, and the mMTC tables, with 32-bit offsets: the branch handle stays
    // below 2^31 entries in both (4,194,303 eMBB tasks), whatever max_branches allows
    long long reps = 0x7fffffffll;
    if (h->cfg.n_embb > 0) reps = std::min(reps, 0x7fffffffll / ((long long)RS_BURSTS * RS_GROUP * h->cfg.n_embb) - 1);
    if (h->cfg.n_mmtc > 0)
        reps = std::min(reps, 0x7fffffffll / ((long long)h->cfg.n_mmtc * std::max<long long>(MTC_DEV_MAX, h->mst.cap)) - 1);
    const long long chunk = std::min<long long>(std::min<long long>(h->la_max, reps) / C, h->cfg.n_envs);
    if (chunk < 1) {
        h->err = "rs_step_clairvoyant: one replica's candidates exceed the largest branch handle";
        return RS_EINVAL;
    }
    rs_config c = h->cfg;
    c.n_envs = (int32_t)(chunk * C);
    rs_handle* b = nullptr;
    int rc = rs_create(&c, h->device, &b);
    if (rc != RS_OK) {
        h->err = std::string("rs_step_clairvoyant: creating the branch handle: ") + (b ? b->err : "");
        rs_destroy(b);
        return rc;
    }
    b->fad = h->fad;
    b->fad_valid = h->fad_valid;
    b->fad32 = h->fad32;
    b->fps = h->fps;
    b->tables_borrowed = true;
    for (int f = 0; f < RS_N_TRACES; ++f) b->fad_loaded[f] = h->fad_loaded[f];
    b->fad_hash = h->fad_hash;
    b->hdev = h->hdev;  // (everything in it but n_envs follows from the configuration and the tables)
    b->hdev.n_envs = c.n_envs;
    b->hint_auto = false;  // BLOCK instance: the branches are agent-like allocations (a hint only)
    b->block_hint = 1;
    if (hipMemcpyAsync(b->ddev, &b->hdev, sizeof(RsDev), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
        hipStreamSynchronize(b->stream) != hipSuccess || ensure_event(b, &b->ev_fork_in) != RS_OK ||
        ensure_event(b, &b->ev_fork_out) != RS_OK) {
        h->err = "rs_step_clairvoyant: setting up the branch handle failed";
        rs_destroy(b);
        return RS_EHIP;
    }
    if (!h->d_la_err) HIPCHK(h, hipMalloc((void**)&h->d_la_err, sizeof(int32_t) * h->cfg.n_envs));
    h->la = b;
    return RS_OK;
}

extern "C" int rs_step_clairvoyant(rs_handle* h, int32_t* actions_out, float* obs, double* reward, int32_t* labels,
                                   int32_t* violations) {
    if (!h) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->is_reset) {
        h->err = "rs_step_clairvoyant: call rs_reset first";
        return RS_ESTATE;
    }
    if (h->la_max <= 0) {
        h->err = "rs_step_clairvoyant: no lookahead capacity (rs_set_lookahead)";
        return RS_ESTATE;
    }
    if (h->clock > 2000000000 - h->cfg.slots_per_step) {
        h->err = "rs_step_clairvoyant: slot clock would overflow; reset the environment";
        return RS_ESTATE;
    }
    int rc = ensure_branches(h);
    if (rc != RS_OK) return rc;
    rs_handle* B = h->la;
    rs::ForkArgs a;
    memset(&a, 0, sizeof a);
    if ((rc = fork_table(B, h, false, &a.T)) != RS_OK) return rc;
    const int N = h->cfg.n_envs, S = h->n_slices, C = h->cfg.n_prbs + 1;
    const int chunk = B->cfg.n_envs / C;
    a.index = nullptr;
    a.n_dst = B->cfg.n_envs;
    a.run_src = h->d_run;
    a.run_dst = B->d_run;
    a.C = C;
    a.n_act = S;
    a.n_prbs = h->cfg.n_prbs;
    a.acts_src = h->d_actions;
    a.acts_dst = B->d_actions;
    // every round of every chunk on the branch handle's stream, behind h's queued work; h's real step behind the last select
    if ((rc = stream_after(h, &B->ev_fork_in, h->stream, B->stream)) != RS_OK) return rc;
    HIPCHK(h, hipMemsetAsync(h->d_la_err, 0, sizeof(int32_t) * N, B->stream));
    for (int s = 0; s < S; ++s)
        for (int c0 = 0; c0 < N; c0 += chunk) {
            a.c0 = c0;
            a.cnt = std::min(chunk, N - c0);
            a.s = s;
            hipLaunchKernelGGL(rs::fork_gather_kernel, dim3((unsigned)((a.n_dst + 3) / 4)), dim3(256), 0, B->stream, a);
            HIPCHK(h, hipGetLastError());
            B->clock = h->clock;
            B->steps = h->steps;
            B->is_reset = true;
            if ((rc = launch_step(B)) != RS_OK) {
                h->err = "rs_step_clairvoyant: branch step: " + B->err;
                return rc;
            }
            hipLaunchKernelGGL(rs::clairvoyant_select_kernel, dim3((unsigned)((a.cnt + 3) / 4)), dim3(256), 0, B->stream,
                               (const int32_t*)B->d_viol, (const int32_t*)B->st.err, C, c0, a.cnt, s, S, h->cfg.n_prbs,
                               h->la_widest, h->d_actions, h->d_la_err);
            HIPCHK(h, hipGetLastError());
        }
    if ((rc = stream_after(h, &B->ev_fork_out, B->stream, h->stream)) != RS_OK) return rc;
    if ((rc = launch_step(h)) != RS_OK) return rc;
    if ((rc = rs_fetch(h, actions_out, obs, reward, labels, violations)) != RS_OK) return rc;
    std::vector<int32_t> e((size_t)N);
    HIPCHK(h, hipMemcpyAsync(e.data(), h->d_la_err, sizeof(int32_t) * N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < N; ++i)
        if (e[i]) {
            h->err = "capacity exceeded in a lookahead branch of replica " + std::to_string(i) + ":" +
                     ((e[i] & 1) ? " UEs per slice" : "") + ((e[i] & 2) ? " active VBR bursts per UE" : "") +
                     ((e[i] & 4) ? " backlogged mMTC devices" : "");
            return RS_EOVERFLOW;
        }
    return RS_OK;
}
