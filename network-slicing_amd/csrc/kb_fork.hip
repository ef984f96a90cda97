// kb_fork.hip -- device-side agent fork (kb_fork) and deployment into inference-only handles (kb_deploy).
// #included by rs_api.hip after kb_api.hip: it uses the agent handle and changes none of its kernels.
//
// An agent is its slice of the per-learner tables, the control state, its tie-break stream, its flag word and its
// dictionaries.  Nothing in them names the agent's place in the batch but kf_owner (a task id, remapped) and the shell
// table (pool offsets, rebuilt): every draw is keyed by the agent's seed and counters.  A dictionary is scattered over the
// source's pool shell by shell, in the order its learner happened to win the allocator; the destination lays every
// dictionary out whole, in (dictionary, shell) order, from an exclusive scan of the shells' sizes -- so the layout depends
// on the arguments alone.  An inference-only destination (KbDev.tri == KB_TRI_NONE) takes the vector page of every shell and
// nothing else: select_action reads coordinates, coefficients and the grid-index row, never Kinv.

#define KB_FORK_BLK 2048  // doubles (16 KB) of the destination pool one wave copies per turn

namespace kb {

struct ForkArgs {
    KbDev Dd;              // destination
    KbState Kd, Ks;
    uint64_t src_pool_doubles;
    int32_t src_tri;
    int32_t n_dict;        // destination dictionaries (= learners: one agent per replica)
    int32_t empty;         // 1: the dictionaries did not fit -- the destination gets the control state and empty dictionaries
    const int32_t* index;  // [Dd.n_envs] source agent of every destination agent
    uint64_t* base;        // [n_dict + 1] sizes, then (fork_scan_kernel) first pool double of every dictionary; [n_dict] = the top
    uint64_t* total;       // [1] the top again, for the host
    const float* prev_s;   // [n_envs][nv] the observation the executed action was chosen in (resident loop)
    float* prev_d;
    int32_t* hits_d;       // [T] the hits an inference-mode history column repeats: none yet
};

// source dictionary of destination dictionary jd
__device__ __forceinline__ int fork_src_dict(const ForkArgs& a, int jd) {
    const int j = jd / a.Dd.S;
    return a.index[j] * a.Dd.S + (jd - j * a.Dd.S);
}

// doubles every destination dictionary needs: its source's shells (64 landmarks each) at the destination's shell sizes
__global__ __launch_bounds__(256) void fork_count_kernel(ForkArgs a) {
    const int jd = blockIdx.x * blockDim.x + threadIdx.x;
    if (jd >= a.n_dict) return;
    const int m = a.Ks.m[fork_src_dict(a, jd)];
    a.base[jd] = kb_shells_before((m + KB_CH - 1) / KB_CH, a.Dd.tri);
}

// exclusive scan of the sizes, in place, starting at 64 (offset 0 means "no shell"): one workgroup, a contiguous run per
// thread -- integer sums, so the layout is the same whatever the launch
__global__ __launch_bounds__(1024) void fork_scan_kernel(uint64_t* base, int n, uint64_t* total) {
    __shared__ unsigned long long part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
    unsigned long long sum = 0;
    for (int i = i0; i < i1; ++i) sum += base[i];
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = 64 + (t ? part[t - 1] : 0ull);
    for (int i = i0; i < i1; ++i) {
        const unsigned long long c = base[i];
        base[i] = run;
        run += c;
    }
    if (t == 1023) {
        base[n] = 64 + part[1023];
        total[0] = 64 + part[1023];
    }
}

// Table gather: a wave per destination dictionary (= learner) copies its rows of the per-dictionary and per-learner tables,
// writes its shell table from the scan, and -- the wave of learner 0 of an agent -- the agent's own words.
__global__ __launch_bounds__(256) void fork_tables_kernel(ForkArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= a.n_dict) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int r = a.index[j], sd = r * D.S + s;
    const int m = a.empty ? 0 : a.Ks.m[sd];
    const int nsh = (m + KB_CH - 1) / KB_CH;
    const uint64_t at = a.base[jd];
    for (int b = lane; b < D.max_shells; b += 64)
        a.Kd.shell[(size_t)jd * D.max_shells + b] = b < nsh ? at + kb_shells_before(b, D.tri) : 0ull;
    {   // newest landmark per grid index: KB_HEAD int32 = 64 x 16 bytes
        const int4 none = {-1, -1, -1, -1};
        int4* hd = (int4*)(a.Kd.head + (size_t)jd * KB_HEAD);
        const int4* hs = (const int4*)(a.Ks.head + (size_t)sd * KB_HEAD);
        hd[lane] = a.empty ? none : hs[lane];
    }
    for (int c = lane; c < D.n_prbs; c += 64) a.Kd.acc[(size_t)jd * D.n_prbs + c] = a.Ks.acc[(size_t)sd * D.n_prbs + c];
    if (lane == 0) {
        a.Kd.m[jd] = m;
        a.Kd.offgrid[jd] = a.empty ? 0 : a.Ks.offgrid[sd];
        a.Kd.f32bad[jd] = a.empty ? 0 : a.Ks.f32bad[sd];
        a.Kd.ver[jd] = a.empty ? 0 : a.Ks.ver[sd];
        // (one agent per replica: dictionary = task; the K_f row belongs to this learner's last predict, or to nobody)
        a.Kd.kf_owner[jd] = (!a.empty && a.Ks.kf_owner[sd] == sd) ? jd : -1;
        a.Kd.f_last[jd] = a.empty ? 0.0 : a.Ks.f_last[sd];
        a.Kd.m_last[jd] = a.empty ? 0 : a.Ks.m_last[sd];
        a.Kd.tie_ctr[jd] = a.Ks.tie_ctr[sd];
        a.Kd.action[jd] = a.Ks.action[sd];
        a.Kd.security[jd] = a.Ks.security[sd];
        a.Kd.margins[jd] = a.Ks.margins[sd];
        a.Kd.fver[jd] = -1;  // no stored scores: an optimisation no result depends on
        for (int q = 0; q < 4; ++q) a.Kd.stats[(size_t)jd * 4 + q] = 0;
        a.hits_d[jd] = 0;
    }
    if (s == 0) {
        if (lane == 0) {
            a.Kd.seeds[j] = a.Ks.seeds[r];
            a.Kd.adjusted[j] = a.Ks.adjusted[r];
            a.Kd.err[j] = a.Ks.err[r];  // verbatim: "a dictionary is at its capacity" / "the pool was exhausted" travel with the agent
        }
        for (int q = lane; q < D.nv; q += 64) a.prev_d[(size_t)j * D.nv + q] = a.prev_s[(size_t)r * D.nv + q];
    }
    if (jd == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[a.n_dict];
}

// Shell gather.  The destination's dictionaries fill [64, top) of its pool without a gap, so the work line is that range cut
// into pieces of KB_FORK_BLK doubles, a wave each: balanced by bytes whatever the dictionaries' sizes (one dictionary of 3,000
// landmarks among hundred-landmark ones is ~700 pieces spread over the launch, not one long tail).  A piece finds its
// dictionary by bisection of the scan, its shell by walking the sizes, and copies run after run with 16-byte loads and stores,
// two in flight per lane.  Every size is a multiple of 64 doubles, so every run is 16-byte aligned on both sides.  Sources that
// repeat in the index are read again through the cache.
// (The bisection and the walk are a few dozen dependent loads of the scan and of the size formula per piece -- twice per piece for
// an inference-only destination, whose 1,920-double shells are shorter than a piece.  That is latency beside a 16 KB copy, not
// bandwidth: 4096 agents' 7.8 GB are written in 2.1 ms, 3.7 TB/s, profiles/deploy_fanout_kernel_trace_stats.txt.)
__global__ __launch_bounds__(256) void fork_shells_kernel(ForkArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t top = a.base[a.n_dict];
    const uint64_t n_blk = (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK;
    for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < n_blk; blk += (uint64_t)gridDim.x * 4) {
        uint64_t p = 64 + blk * KB_FORK_BLK;
        const uint64_t pe = p + KB_FORK_BLK < top ? p + KB_FORK_BLK : top;
        int lo = 0, hi = a.n_dict - 1;  // the last dictionary that starts at or before p (empty ones share their start with the next)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.base[mid] <= p) lo = mid;
            else hi = mid - 1;
        }
        int jd = lo;
        while (p < pe) {
            while (a.base[jd + 1] <= p) ++jd;  // (p < top = base[n_dict]: ends)
            const uint64_t q = p - a.base[jd];
            int b = 0;
            uint64_t c = 0, sz = kb_shell_doubles(0, D.tri);
            while (q >= c + sz) {
                c += sz;
                ++b;
                sz = kb_shell_doubles(b, D.tri);
            }
            const uint64_t in = q - c;
            const uint64_t seg = sz - in < pe - p ? sz - in : pe - p;
            const uint64_t so = b < D.max_shells ? a.Ks.shell[(size_t)fork_src_dict(a, jd) * D.max_shells + b] : 0ull;
            double* __restrict__ d = a.Kd.pool + p;
            // a source shell that is missing or does not lie inside the source's pool is never read (zeros instead)
            const bool ok = so >= 64 && so + kb_shell_doubles(b, a.src_tri) <= a.src_pool_doubles;
            if (ok) {
                const double* __restrict__ sp = a.Ks.pool + so + in;
                uint64_t o = (uint64_t)lane * 2;
                for (; o + 128 < seg; o += 256) {
                    const kb_f64x2 v0 = *(const kb_f64x2*)(sp + o);
                    const kb_f64x2 v1 = *(const kb_f64x2*)(sp + o + 128);
                    *(kb_f64x2*)(d + o) = v0;
                    *(kb_f64x2*)(d + o + 128) = v1;
                }
                if (o < seg) *(kb_f64x2*)(d + o) = *(const kb_f64x2*)(sp + o);
            } else {
                const kb_f64x2 z = {0.0, 0.0};
                for (uint64_t o = (uint64_t)lane * 2; o < seg; o += 128) *(kb_f64x2*)(d + o) = z;
            }
            p += seg;
        }
    }
}

}  // namespace kb

// kb_config with the batch size and the pool's size masked: what two handles must share to move agents between them
static uint64_t kb_fork_cfg_hash(const kb_handle* k) {
    kb_config c = k->cfg;
    c.n_envs = 0;
    c.pool_bytes = 0;
    return fnv1a(&c, sizeof c);
}

// Every device array behind a handle is a region of its saved state (k->regions, filled by kalloc).  The fork names each one:
// copied per agent, copied per dictionary, restarted, or handle-wide.  A region it does not know is a refusal, so that an
// array added to the state later cannot be left out of forks unnoticed.
static int kb_fork_classify(kb_handle* k, std::string* err) {
    const kb::KbState& K = k->K;
    // per agent / per learner, gathered by fork_tables_kernel
    const void* per_agent[] = {K.f_last, K.m_last, K.tie_ctr, K.seeds, K.action, K.security, K.margins, K.adjusted, K.acc, K.err,
                               k->d_prev_state};
    // per dictionary: the tables (kf_owner remapped to the new task id, the shell table rebuilt from the scan) and, shell by
    // shell, the pool (fork_shells_kernel); pool_top is the scan's total
    const void* per_dict[] = {K.m, K.shell, K.head, K.kf_owner, K.offgrid, K.f32bad, K.ver, K.pool, K.pool_top};
    // restarted as after kb_reset: the counters, the repair queues (empty between steps), the launch-order lists, the stored
    // select scores (fver = -1) and their operands, the retained hits; staging and scratch that every call writes before it reads
    const void* restarted[] = {K.stats, K.hv_work, K.heavy, K.hv_cfrom, K.hv_cstar, K.hv_state, K.hv_grew, K.hv_m, K.hv_pend,
                               K.hv_delta, K.hv_f, K.hv_mvbase, K.hv_r1base, K.big, K.isbig, K.F, K.fstate, K.fver, K.Wg, K.fdirect,
                               K.dlist, k->d_hits, k->d_state, k->d_action, k->d_labels, k->d_out, k->d_gstats};
    // handle-wide: the G table (a function of the configuration); the buffers of the shared-dictionary mode (unused here)
    const void* handle_wide[] = {K.gtab, K.workb, K.workq, K.workF, K.workE, K.workg, K.workf, k->d_cursor, k->d_cstar, k->d_props,
                                 k->d_counts, k->d_block, k->d_mprops, k->d_mcounts, k->d_taken, k->d_total};
    for (auto& r : k->regions) {
        bool known = false;
        for (const void* p : per_agent) known = known || p == r.first;
        for (const void* p : per_dict) known = known || p == r.first;
        for (const void* p : restarted) known = known || p == r.first;
        for (const void* p : handle_wide) known = known || p == r.first;
        if (!known) {
            *err = "a state region of the handle is not classified for forking";
            return RS_ESTATE;
        }
    }
    return RS_OK;
}

// dst agent j := src agent src_index[j], on dst's stream behind src's queued work; src's later work behind the gather.  One
// host wait: the scan's total, for the overflow check.
static int kb_fork_core(kb_handle* dst, kb_handle* src, const int32_t* src_index, const char* who) {
    int rc;
    std::string why;
    if ((rc = kb_fork_classify(src, &why)) != RS_OK || (rc = kb_fork_classify(dst, &why)) != RS_OK) {
        dst->err = std::string(who) + ": " + why;
        return rc;
    }
    const int n_dst = dst->cfg.n_envs, ND = dst->n_dict;
    const size_t T = (size_t)dst->T;
    HIPCHK(dst, hipSetDevice(dst->device));
    kb_drop_graph(dst);
    if (!dst->d_fork_idx) HIPCHK(dst, hipMalloc((void**)&dst->d_fork_idx, sizeof(int32_t) * n_dst));
    if (!dst->d_fork_base) HIPCHK(dst, hipMalloc((void**)&dst->d_fork_base, sizeof(uint64_t) * ((size_t)ND + 2)));
    if (!dst->h_fork_idx) HIPCHK(dst, hipHostMalloc((void**)&dst->h_fork_idx, sizeof(int32_t) * n_dst, hipHostMallocDefault));
    if (!dst->h_fork_total) HIPCHK(dst, hipHostMalloc((void**)&dst->h_fork_total, sizeof(uint64_t), hipHostMallocDefault));
    memcpy(dst->h_fork_idx, src_index, sizeof(int32_t) * n_dst);  // (a previous fork ended with its host wait: the buffer is free)
    if ((rc = stream_after(dst, &dst->ev_fork_in, src->stream, dst->stream)) != RS_OK) return rc;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, sizeof(int32_t) * n_dst, hipMemcpyHostToDevice, dst->stream));
    // what kb_reset restarts (the tables kernel writes stats, fver and the retained hits)
    HIPCHK(dst, hipMemsetAsync(dst->d_gstats, 0, sizeof(uint64_t) * 32, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.hv_work, 0, sizeof(unsigned long long) * 8, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.heavy, 0, sizeof(int32_t) * 4, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.big, 0, sizeof(int32_t) * 2 * (1 + KB_BIG_MAX), dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.isbig, 0, sizeof(int32_t) * 2 * T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.pool, 0, sizeof(double) * 64, dst->stream));  // (below every shell; never read)
    kb_prune_restart(dst);
    kb::ForkArgs a;
    memset(&a, 0, sizeof a);
    a.Dd = dst->D;
    a.Kd = dst->K;
    a.Ks = src->K;
    a.src_pool_doubles = src->D.pool_doubles;
    a.src_tri = src->D.tri;
    a.n_dict = ND;
    a.index = dst->d_fork_idx;
    a.base = dst->d_fork_base;
    a.total = dst->d_fork_base + ND + 1;
    a.prev_s = src->d_prev_state;
    a.prev_d = dst->d_prev_state;
    a.hits_d = dst->d_hits;
    hipLaunchKernelGGL(kb::fork_count_kernel, dim3((unsigned)((ND + 255) / 256)), dim3(256), 0, dst->stream, a);
    hipLaunchKernelGGL(kb::fork_scan_kernel, dim3(1), dim3(1024), 0, dst->stream, a.base, ND, a.total);
    HIPCHK(dst, hipGetLastError());
    dst->h_fork_total[0] = 0;
    HIPCHK(dst, hipMemcpyAsync(dst->h_fork_total, a.total, sizeof(uint64_t), hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    const uint64_t top = dst->h_fork_total[0];
    a.empty = top > dst->D.pool_doubles ? 1 : 0;
    hipLaunchKernelGGL(kb::fork_tables_kernel, dim3((unsigned)((ND + 3) / 4)), dim3(256), 0, dst->stream, a);
    if (!a.empty && top > 64) {
        const uint64_t n_blk = (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK;
        const uint64_t grid = (n_blk + 3) / 4;
        hipLaunchKernelGGL(kb::fork_shells_kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, dst->stream, a);
    }
    HIPCHK(dst, hipGetLastError());
    if ((rc = stream_after(dst, &dst->ev_fork_out, dst->stream, src->stream)) != RS_OK) return rc;
    if (dst->h_seen) dst->h_seen[0] = dst->h_seen[1] = 0;
    dst->gemm_fresh = false;
    dst->big_par = 0;
    dst->is_reset = true;
    if (a.empty) {
        dst->err = std::string(who) + ": the source dictionaries need " + std::to_string(top * 8) + " bytes of pool, the destination's pool has " +
                   std::to_string((uint64_t)dst->D.pool_doubles * 8) + "; the destination was left reset with empty dictionaries";
        return RS_EOVERFLOW;
    }
    return RS_OK;
}

static int kb_fork_check(kb_handle* dst_or_null, kb_handle* src, const int32_t* src_index, int n, std::string* err, const char* who) {
    if (src->D.shared || (dst_or_null && dst_or_null->D.shared)) {
        *err = std::string(who) + ": shared-dictionary handles are not supported";
        return RS_EINVAL;
    }
    if (src->ref || (dst_or_null && dst_or_null->ref)) {
        *err = std::string(who) + ": a by-reference handle (kb_deploy_ref) holds its dictionaries in a shared read-only store: deploy from its source";
        return RS_ESTATE;
    }
    if (dst_or_null && kb_fork_cfg_hash(dst_or_null) != kb_fork_cfg_hash(src)) {
        *err = std::string(who) + ": the handles' configurations differ (beyond n_envs and pool_bytes)";
        return RS_EINVAL;
    }
    for (int j = 0; j < n; ++j)
        if (src_index[j] < 0 || src_index[j] >= src->cfg.n_envs) {
            *err = std::string(who) + ": source index " + std::to_string(src_index[j]) + " of destination agent " + std::to_string(j) +
                   " out of range";
            return RS_EINVAL;
        }
    if (!src->is_reset) {
        *err = std::string(who) + ": the source was never reset";
        return RS_ESTATE;
    }
    if (dst_or_null && dst_or_null->device != src->device) {
        *err = std::string(who) + ": the handles live on different devices";
        return RS_ESTATE;
    }
    return RS_OK;
}

extern "C" int kb_fork(kb_handle* dst, kb_handle* src, const int32_t* src_index) {
    if (!dst || !src || !src_index) return RS_EINVAL;
    if (dst == src) {
        dst->err = "kb_fork: source and destination must be different handles";
        return RS_EINVAL;
    }
    int rc = kb_fork_check(dst, src, src_index, dst->cfg.n_envs, &dst->err, "kb_fork");
    if (rc != RS_OK) return rc;
    if (dst->frozen || src->frozen) {
        dst->err = "kb_fork: an inference-only handle (kb_deploy) holds no Kinv: it can be deployed again (kb_deploy), not forked";
        return RS_ESTATE;
    }
    return kb_fork_core(dst, src, src_index, "kb_fork");
}

extern "C" int kb_deploy(kb_handle* src, const int32_t* src_index, int32_t n, kb_handle** out) {
    if (!src || !src_index || !out || n <= 0) return RS_EINVAL;
    *out = nullptr;
    int rc = kb_fork_check(nullptr, src, src_index, n, &src->err, "kb_deploy");
    if (rc != RS_OK) return rc;
    HIPCHK(src, hipSetDevice(src->device));
    // the one host read: the source's dictionary sizes, to size the compact pool exactly
    std::vector<int32_t> m((size_t)src->n_dict);
    HIPCHK(src, hipMemcpyAsync(m.data(), src->K.m, sizeof(int32_t) * m.size(), hipMemcpyDeviceToHost, src->stream));
    HIPCHK(src, hipStreamSynchronize(src->stream));
    const int S = src->cfg.n_slices;
    unsigned long long doubles = 64;  // offset 0 means "no shell": the pool starts with 64 unused doubles
    for (int j = 0; j < n; ++j)
        for (int s = 0; s < S; ++s)
            doubles += kb::kb_shells_before((m[(size_t)src_index[j] * S + s] + KB_CH - 1) / KB_CH, KB_TRI_NONE);
    kb_config c = src->cfg;
    c.n_envs = n;
    c.pool_bytes = (int64_t)(doubles * 8);
    kb_handle* d = nullptr;
    rc = kb_create_impl(&c, src->device, &d, doubles);
    if (rc != RS_OK) {
        src->err = std::string("kb_deploy: creating the inference-only handle: ") + (d ? d->err : "");
        kb_destroy(d);
        return rc;
    }
    rc = kb_fork_core(d, src, src_index, "kb_deploy");
    if (rc != RS_OK) {
        src->err = d->err;
        kb_destroy(d);
        return rc;
    }
    *out = d;
    return RS_OK;
}
