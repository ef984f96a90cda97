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

namespace kb {

// what a transfer kernel is given: kb_fork / kb_deploy / kb_fork_rebuild, and kb_unshare / kb_share (kb_bridge.hip)
struct XferArgs {
    KbDev Dd;              // destination
    KbState Kd, Ks;
    uint64_t src_pool_doubles;
    int32_t src_tri;
    int32_t src_max_shells;  // (capacities may differ towards the triangle: the source's shell table has its own width)
    int32_t n_dict;        // destination dictionaries
    int32_t empty;         // 1: the dictionaries did not fit -- the destination gets the control state and empty dictionaries
    int32_t dict_agent;    // kb_share: the source agent whose dictionaries become the shared ones
    const int32_t* index;  // [Dd.n_envs] source agent (replica, of a shared source) of every destination agent's control state
    uint64_t* base;        // [n_dict + 1] sizes, then (fork_scan_kernel) first pool double of every dictionary; [n_dict] = the top
                           // (kb_share: the host's own sums); the scan leaves the top in [n_dict + 1] as well, for the host
    uint64_t* words;       // kb_unshare: [0] the largest source dictionary (the capacity check), [1] the Kinv tiles of the S sources
    const float* prev_s;   // [n_envs][nv] the observation the executed action was chosen in (resident loop)
    float* prev_d;
    int32_t* hits_d;       // [T] the hits an inference-mode history column repeats: none yet
};

// source dictionary of destination dictionary jd, one agent per replica on both sides
__device__ __forceinline__ int fork_src_dict(const XferArgs& a, int jd) {
    const int j = jd / a.Dd.S;
    return a.index[j] * a.Dd.S + (jd - j * a.Dd.S);
}

// doubles every destination dictionary needs: its source's shells (64 landmarks each) at the destination's shell sizes
__global__ __launch_bounds__(256) void fork_count_kernel(XferArgs a) {
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

// ---- the control state, gathered.  What crosses is written once here; the cache of the last kb_predict (f_last, m_last,
// kf_owner) is each caller's own three words.

// destination task td := source task ts, by one lane: the control words; what kb_reset restarts, restarted
__device__ __forceinline__ void gather_task_words(const KbState& Kd, const KbState& Ks, int32_t* hits_d, int td, int ts) {
    Kd.tie_ctr[td] = Ks.tie_ctr[ts];
    Kd.action[td] = Ks.action[ts];
    Kd.security[td] = Ks.security[ts];
    Kd.margins[td] = Ks.margins[ts];
    Kd.fver[td] = -1;  // no stored scores: an optimisation no result depends on
    for (int q = 0; q < 4; ++q) Kd.stats[(size_t)td * 4 + q] = 0;
    hits_d[td] = 0;
}
// destination agent j := source agent r, by the wave of its learner 0: its own words and its previous observation
__device__ __forceinline__ void gather_agent_words(const KbDev& D, const KbState& Kd, const KbState& Ks, float* prev_d, const float* prev_s,
                                                   int j, int r, int lane) {
    if (lane == 0) {
        Kd.seeds[j] = Ks.seeds[r];
        Kd.adjusted[j] = Ks.adjusted[r];
        Kd.err[j] = Ks.err[r];  // verbatim: "a dictionary is at its capacity" / "the pool was exhausted" travel with the agent
    }
    for (int q = lane; q < D.nv; q += 64) prev_d[(size_t)j * D.nv + q] = prev_s[(size_t)r * D.nv + q];
}
// destination dictionary jd := source dictionary sd of m landmarks (empty: none crosses, m = 0).  By one wave its shell table,
// the shells laid out whole from `at`, and its heads; by one lane its words
__device__ __forceinline__ void gather_dict_tables(const KbDev& D, const KbState& Kd, const KbState& Ks, int jd, int sd, int m, int empty,
                                                   uint64_t at, int lane) {
    const int nsh = (m + KB_CH - 1) / KB_CH;
    for (int b = lane; b < D.max_shells; b += 64) Kd.shell[(size_t)jd * D.max_shells + b] = b < nsh ? at + kb_shells_before(b, D.tri) : 0ull;
    {   // newest landmark per grid index: KB_HEAD int32 = 64 x 16 bytes
        const int4 none = {-1, -1, -1, -1};
        int4* hd = (int4*)(Kd.head + (size_t)jd * KB_HEAD);
        const int4* hs = (const int4*)(Ks.head + (size_t)sd * KB_HEAD);
        hd[lane] = empty ? none : hs[lane];
    }
}
__device__ __forceinline__ void gather_dict_words(const KbState& Kd, const KbState& Ks, int jd, int sd, int m, int empty) {
    Kd.m[jd] = m;
    Kd.offgrid[jd] = empty ? 0 : Ks.offgrid[sd];
    Kd.f32bad[jd] = empty ? 0 : Ks.f32bad[sd];
    Kd.ver[jd] = empty ? 0 : Ks.ver[sd];
}

// Table gather: a wave per destination dictionary (= learner) copies its rows of the per-dictionary and per-learner tables,
// writes its shell table from the scan, and -- the wave of learner 0 of an agent -- the agent's own words.
__global__ __launch_bounds__(256) void fork_tables_kernel(XferArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= a.n_dict) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int r = a.index[j], sd = r * D.S + s;
    const int m = a.empty ? 0 : a.Ks.m[sd];
    gather_dict_tables(D, a.Kd, a.Ks, jd, sd, m, a.empty, a.base[jd], lane);
    for (int c = lane; c < D.n_prbs; c += 64) a.Kd.acc[(size_t)jd * D.n_prbs + c] = a.Ks.acc[(size_t)sd * D.n_prbs + c];
    if (lane == 0) {
        gather_dict_words(a.Kd, a.Ks, jd, sd, m, a.empty);
        // (one agent per replica: dictionary = task; the K_f row belongs to this learner's last predict, or to nobody)
        a.Kd.kf_owner[jd] = (!a.empty && a.Ks.kf_owner[sd] == sd) ? jd : -1;
        a.Kd.f_last[jd] = a.empty ? 0.0 : a.Ks.f_last[sd];
        a.Kd.m_last[jd] = a.empty ? 0 : a.Ks.m_last[sd];
        gather_task_words(a.Kd, a.Ks, a.hits_d, jd, sd);
    }
    if (s == 0) gather_agent_words(D, a.Kd, a.Ks, a.prev_d, a.prev_s, j, r, lane);
    if (jd == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[a.n_dict];
}

// ---- the shell gathers.  Every one walks the work line of its destination (kb_layout.h): a wave takes piece after piece and,
// for each run, copies from its source or writes zeros.
// (The bisection and the walk are a few dozen dependent loads of the scan and of the size formula per piece -- twice per piece for
// an inference-only destination, whose 1,920-double shells are shorter than a piece.  That is latency beside a 16 KB copy, not
// bandwidth: 4096 agents' 7.8 GB are written in 2.1 ms, 3.7 TB/s, profiles/deploy_fanout_kernel_trace_stats.txt.)
template <class Cut, class Body>
__device__ __forceinline__ void line_walk(const uint64_t* base, int n, int tri, Cut cut, Body body) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t n_blk = kb_line_pieces(base[n]);
    for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < n_blk; blk += (uint64_t)gridDim.x * 4) kb_line_walk(base, n, tri, blk, cut, body);
}
// 16-byte copies of `n` doubles (a multiple of 64, 16-byte aligned on both sides) by one wave, two in flight per lane
__device__ __forceinline__ void wave_copy(double* __restrict__ d, const double* __restrict__ sp, uint64_t n, int lane) {
    uint64_t o = (uint64_t)lane * 2;
    for (; o + 128 < n; o += 256) {
        const kb_f64x2 v0 = *(const kb_f64x2*)(sp + o);
        const kb_f64x2 v1 = *(const kb_f64x2*)(sp + o + 128);
        *(kb_f64x2*)(d + o) = v0;
        *(kb_f64x2*)(d + o + 128) = v1;
    }
    if (o < n) *(kb_f64x2*)(d + o) = *(const kb_f64x2*)(sp + o);
}
__device__ __forceinline__ void wave_zero(double* __restrict__ d, uint64_t n, int lane) {
    const kb_f64x2 z = {0.0, 0.0};
    for (uint64_t o = (uint64_t)lane * 2; o < n; o += 128) *(kb_f64x2*)(d + o) = z;
}
// pool offset of shell b of source dictionary sd if its first `need` doubles lie inside the source's pool, else 0: a source
// shell that is missing or does not lie there is never read (zeros instead)
__device__ __forceinline__ uint64_t src_shell(const XferArgs& a, int sd, int b, uint64_t need) {
    const uint64_t so = b < a.src_max_shells ? a.Ks.shell[(size_t)sd * a.src_max_shells + b] : 0ull;
    return so >= 64 && so + need <= a.src_pool_doubles ? so : 0ull;
}

// kb_fork, kb_deploy: whole shells, at the destination's sizes.  Sources that repeat in the index are read again through the cache.
__global__ __launch_bounds__(256) void fork_shells_kernel(XferArgs a) {
    const int lane = threadIdx.x & 63;
    line_walk(a.base, a.n_dict, a.Dd.tri, KbCutShell(), [&](int jd, int b, uint64_t in, uint64_t p, uint64_t seg) {
        const uint64_t so = src_shell(a, fork_src_dict(a, jd), b, kb_shell_doubles(b, a.src_tri));
        if (so) wave_copy(a.Kd.pool + p, a.Ks.pool + so + in, seg, lane);
        else wave_zero(a.Kd.pool + p, seg, lane);
    });
}

}  // namespace kb

// kb_config with what two handles may differ in masked: what they must share to move agents between them.  A fork masks the
// batch size and the pool's size; the bridge (kb_bridge.hip) also the storage, and towards the triangle the capacity
static uint64_t kb_xfer_cfg_hash(const kb_handle* k, bool mask_storage, bool mask_capacity) {
    kb_config c = k->cfg;
    c.n_envs = 0;
    c.pool_bytes = 0;
    if (mask_storage) c.shared_dictionary = c.first_env = 0;
    if (mask_capacity) c.capacity = 0;
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

// ---- the host sequence of a transfer into dst: enter, the caller's count, scan and wait, tables and line kernels, leave.

// Both handles classified, dst's graph dropped, the index pinned and uploaded, dst's stream behind src's queued work, and what
// kb_reset restarts restarted (the tables kernels write stats, fver and the retained hits).
static int kb_xfer_enter(kb_handle* dst, kb_handle* src, const int32_t* index, const char* who) {
    int rc;
    std::string why;
    if ((rc = kb_fork_classify(src, &why)) != RS_OK || (rc = kb_fork_classify(dst, &why)) != RS_OK) {
        dst->err = std::string(who) + ": " + why;
        return rc;
    }
    const size_t n_dst = (size_t)dst->cfg.n_envs;
    HIPCHK(dst, hipSetDevice(dst->device));
    kb_drop_graph(dst);
    if (!dst->d_fork_idx) HIPCHK(dst, hipMalloc((void**)&dst->d_fork_idx, sizeof(int32_t) * n_dst));
    if (!dst->d_fork_base) HIPCHK(dst, hipMalloc((void**)&dst->d_fork_base, sizeof(uint64_t) * ((size_t)dst->n_dict + 2)));
    if (!dst->h_fork_idx) HIPCHK(dst, hipHostMalloc((void**)&dst->h_fork_idx, sizeof(int32_t) * n_dst, hipHostMallocDefault));
    if (!dst->h_fork_total) HIPCHK(dst, hipHostMalloc((void**)&dst->h_fork_total, sizeof(uint64_t), hipHostMallocDefault));
    memcpy(dst->h_fork_idx, index, sizeof(int32_t) * n_dst);  // (a previous transfer ended with its host wait: the buffer is free)
    if ((rc = stream_after(dst, &dst->ev_fork_in, src->stream, dst->stream)) != RS_OK) return rc;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, sizeof(int32_t) * n_dst, hipMemcpyHostToDevice, dst->stream));
    return kb_restart(dst);
}

// the kernels' arguments, but `empty` (known after the wait) and what is one call's own
static kb::XferArgs kb_xfer_args(kb_handle* dst, kb_handle* src, int n_dict) {
    kb::XferArgs a;
    memset(&a, 0, sizeof a);
    a.Dd = dst->D;
    a.Kd = dst->K;
    a.Ks = src->K;
    a.src_pool_doubles = src->D.pool_doubles;
    a.src_tri = src->D.tri;
    a.src_max_shells = src->D.max_shells;
    a.n_dict = n_dict;
    a.index = dst->d_fork_idx;
    a.base = dst->d_fork_base;
    a.prev_s = src->d_prev_state;
    a.prev_d = dst->d_prev_state;
    a.hits_d = dst->d_hits;
    return a;
}

// the sizes a count kernel left in a.base scanned, and the call's one host wait: for the scan's total -- the overflow check --
// and for whatever the caller queued for the host before
static int kb_xfer_scan_wait(kb_handle* dst, const kb::XferArgs& a, uint64_t* top) {
    uint64_t* d_total = a.base + a.n_dict + 1;
    hipLaunchKernelGGL(kb::fork_scan_kernel, dim3(1), dim3(1024), 0, dst->stream, a.base, a.n_dict, d_total);
    HIPCHK(dst, hipGetLastError());
    dst->h_fork_total[0] = 0;
    HIPCHK(dst, hipMemcpyAsync(dst->h_fork_total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    *top = dst->h_fork_total[0];
    return RS_OK;
}

// a wave per destination dictionary (count kernels: a thread), and a shell gather over the work line [64, top)
static void kb_xfer_launch(kb_handle* dst, void (*kernel)(kb::XferArgs), const kb::XferArgs& a, size_t n, int per_block) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + per_block - 1) / per_block)), dim3(256), 0, dst->stream, a);
}
static void kb_xfer_launch_line(kb_handle* dst, void (*kernel)(kb::XferArgs), const kb::XferArgs& a, uint64_t top) {
    if (a.empty || top <= 64) return;
    const uint64_t grid = (kb::kb_line_pieces(top) + 3) / 4;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, dst->stream, a);
}

// src's later work behind the gather; the destination is reset whatever the outcome
static int kb_xfer_leave(kb_handle* dst, kb_handle* src) {
    const int rc = stream_after(dst, &dst->ev_fork_out, dst->stream, src->stream);
    if (dst->h_seen) dst->h_seen[0] = dst->h_seen[1] = 0;
    dst->gemm_fresh = false;
    dst->big_par = 0;
    dst->round_open = false;
    dst->is_reset = true;
    return rc;
}

static int kb_xfer_overflow(kb_handle* dst, const char* who, uint64_t top) {
    dst->err = std::string(who) + ": the source dictionaries need " + std::to_string(top * 8) + " bytes of pool, the destination's pool has " +
               std::to_string((uint64_t)dst->D.pool_doubles * 8) + "; the destination was left reset with empty dictionaries";
    return RS_EOVERFLOW;
}

// dst agent j := src agent src_index[j], on dst's stream behind src's queued work; src's later work behind the gather.  One
// host wait: the scan's total, for the overflow check.
static int kb_fork_core(kb_handle* dst, kb_handle* src, const int32_t* src_index, const char* who) {
    int rc;
    if ((rc = kb_xfer_enter(dst, src, src_index, who)) != RS_OK) return rc;
    kb::XferArgs a = kb_xfer_args(dst, src, dst->n_dict);
    uint64_t top;
    kb_xfer_launch(dst, kb::fork_count_kernel, a, (size_t)a.n_dict, 256);
    if ((rc = kb_xfer_scan_wait(dst, a, &top)) != RS_OK) return rc;
    a.empty = top > dst->D.pool_doubles ? 1 : 0;
    kb_xfer_launch(dst, kb::fork_tables_kernel, a, (size_t)a.n_dict, 4);
    kb_xfer_launch_line(dst, kb::fork_shells_kernel, a, top);
    HIPCHK(dst, hipGetLastError());
    if ((rc = kb_xfer_leave(dst, src)) != RS_OK) return rc;
    return a.empty ? kb_xfer_overflow(dst, who, top) : RS_OK;
}

// the refusals every transfer shares, in the order they are made: a by-reference handle (`ref_why`: what the caller says about
// it), configurations that differ beyond what kb_xfer_cfg_hash masks, an index out of range, a source never reset, two devices
static int kb_xfer_check(kb_handle* dst_or_null, kb_handle* src, const int32_t* index, int n, bool mask_storage, bool mask_capacity,
                         const char* what_dst, const char* ref_why, std::string* err, const char* who) {
    if (src->ref || (dst_or_null && dst_or_null->ref)) {
        *err = std::string(who) + ": a by-reference handle (kb_deploy_ref) holds its dictionaries in a shared read-only store" + ref_why;
        return RS_ESTATE;
    }
    if (dst_or_null && kb_xfer_cfg_hash(dst_or_null, mask_storage, mask_capacity) != kb_xfer_cfg_hash(src, mask_storage, mask_capacity)) {
        *err = std::string(who) + ": the handles' configurations differ (beyond " +
               (mask_storage ? "n_envs, pool_bytes, shared_dictionary and first_env" : "n_envs and pool_bytes") +
               (mask_capacity ? ", and the capacity)" : ")");
        return RS_EINVAL;
    }
    for (int j = 0; j < n; ++j)
        if (index[j] < 0 || index[j] >= src->cfg.n_envs) {
            *err = std::string(who) + ": source index " + std::to_string(index[j]) + " of destination " + what_dst + " " + std::to_string(j) +
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

static int kb_fork_check(kb_handle* dst_or_null, kb_handle* src, const int32_t* src_index, int n, std::string* err, const char* who) {
    if (src->D.shared || (dst_or_null && dst_or_null->D.shared)) {
        *err = std::string(who) + ": shared-dictionary handles are not supported";
        return RS_EINVAL;
    }
    return kb_xfer_check(dst_or_null, src, src_index, n, false, false, "agent", ": deploy from its source", err, who);
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
