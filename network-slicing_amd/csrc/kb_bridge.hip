// kb_bridge.hip -- dictionaries cross between a shared-dictionary handle and a per-replica one: kb_unshare (shared -> one private
// copy per agent) and kb_share (one agent's dictionaries -> the shared ones of a fleet).  #included by rs_api.hip after
// kb_rebuild.hip: it uses the agent handle and kb_fork's count / scan machinery, and changes none of their kernels.
//
// The two storages (kb_kbrl.hip, "Storage") differ in Kinv alone.  Shell b of a per-replica dictionary (KbDev.tri == 1) is
//     [ vector page ][ tiles (b,0) .. (b,b) ][ (b + 1) x 128 partial sums ]
// and shell b of a shared one (KbDev.tri == 0) is
//     [ vector page ][ tiles (b,0) .. (b,b) ][ tiles (0,b) .. (b-1,b) ]          (upper tile (bi,b) at index b + 1 + bi)
// so the first KB_VEC + (b + 1) KB_TILE doubles of a shell -- the page and the lower tiles -- are the same bytes at the same
// offsets in both, and only the tail differs.  Towards the triangle the tail is the partial-sum area, which is scratch:
// matvec_tri_tiles writes every partial sum that matvec_tri_combine then reads (all 64 column sums of every tile, and the row
// sums of every row below the dictionary's end of every off-diagonal tile) before the combine of the SAME mat-vec reads it, so
// nothing read ever predates the call -- the area is zeroed here, which makes the destination a function of the arguments
// alone.  Towards the square the tail is the upper tiles: (bi,b) is the transpose of the lower tile (b,bi) of the same shell,
// and since Kinv only ever receives (d_i d_j) / delta it is bit for bit what the shared mode's own rank-1 update would have put
// there.  Vector pages, heads, chain links and the marks are written by the same finish_update in both modes and cross whole.

namespace kb {

struct BridgeArgs {
    KbDev Dd;              // destination
    KbState Kd, Ks;
    uint64_t src_pool_doubles;
    int32_t src_max_shells;  // (capacities may differ towards the triangle: the source's shell table has its own width)
    int32_t n_dict;        // destination dictionaries
    int32_t empty;         // 1: the dictionaries did not fit -- the destination gets the control state and empty dictionaries
    int32_t dict_agent;    // kb_share: the source agent whose dictionaries become the shared ones
    const int32_t* index;  // [Dd.n_envs] source replica (kb_unshare) / source agent (kb_share) of every destination replica's control state
    uint64_t* base;        // [n_dict + 1] first pool double of every destination dictionary, [n_dict] = the top: kb_unshare's sizes
                           // scanned in place (fork_scan_kernel); kb_share's sums, from the host
    uint64_t* words;       // kb_unshare: [0] the largest source dictionary (the capacity check), [1] the Kinv tiles of the S sources
    const float* prev_s;   // [n_envs][nv] the observation the executed action was chosen in (resident loop)
    float* prev_d;
    int32_t* hits_d;       // [T] the hits an inference-mode history column repeats: none yet
};

// doubles of the shells 0 .. b - 1 of a dictionary that stores both triangles: b pages and 1 + 3 + .. + (2 b - 1) = b^2 tiles
__host__ __device__ inline uint64_t kb_shells_before_full(int b) {
    return (uint64_t)b * KB_VEC + (uint64_t)KB_TILE * ((uint64_t)b * (uint64_t)b);
}
// the part of shell b that is the same bytes in both storages: the vector page and the lower tiles
__host__ __device__ inline uint64_t kb_shell_common(int b) { return (uint64_t)KB_VEC + (uint64_t)(b + 1) * KB_TILE; }

// the control state of destination task (j, s) := that of source task (r, s); what kb_fork restarts, restarted; and -- the
// cache of the last kb_predict does not cross storages -- f_last / m_last cleared.  One lane.
__device__ __forceinline__ void bridge_task_words(const BridgeArgs& a, int td, int ts) {
    a.Kd.f_last[td] = 0.0;
    a.Kd.m_last[td] = 0;
    a.Kd.tie_ctr[td] = a.Ks.tie_ctr[ts];
    a.Kd.action[td] = a.Ks.action[ts];
    a.Kd.security[td] = a.Ks.security[ts];
    a.Kd.margins[td] = a.Ks.margins[ts];
    a.Kd.fver[td] = -1;  // no stored scores: an optimisation no result depends on
    for (int q = 0; q < 4; ++q) a.Kd.stats[(size_t)td * 4 + q] = 0;
    a.hits_d[td] = 0;
}
// the agent's own words, by the wave of its learner 0
__device__ __forceinline__ void bridge_agent_words(const BridgeArgs& a, int j, int r, int lane) {
    if (lane == 0) {
        a.Kd.seeds[j] = a.Ks.seeds[r];
        a.Kd.adjusted[j] = a.Ks.adjusted[r];
        a.Kd.err[j] = a.Ks.err[r];  // verbatim, as kb_fork
    }
    for (int q = lane; q < a.Dd.nv; q += 64) a.prev_d[(size_t)j * a.Dd.nv + q] = a.prev_s[(size_t)r * a.Dd.nv + q];
}
// the per-dictionary tables of destination dictionary jd := those of source dictionary sd, its `nsh` shells laid out whole from `at`
__device__ __forceinline__ void bridge_dict_words(const BridgeArgs& a, int jd, int sd, int m, uint64_t at, int lane) {
    const KbDev& D = a.Dd;
    const int nsh = (m + KB_CH - 1) / KB_CH;
    for (int b = lane; b < D.max_shells; b += 64)
        a.Kd.shell[(size_t)jd * D.max_shells + b] =
            b < nsh ? at + (D.tri ? kb_shells_before(b, 1) : kb_shells_before_full(b)) : 0ull;
    {   // newest landmark per grid index: KB_HEAD int32 = 64 x 16 bytes
        const int4 none = {-1, -1, -1, -1};
        int4* hd = (int4*)(a.Kd.head + (size_t)jd * KB_HEAD);
        const int4* hs = (const int4*)(a.Ks.head + (size_t)sd * KB_HEAD);
        hd[lane] = a.empty ? none : hs[lane];
    }
    if (lane == 0) {
        a.Kd.m[jd] = m;
        a.Kd.offgrid[jd] = a.empty ? 0 : a.Ks.offgrid[sd];
        a.Kd.f32bad[jd] = a.empty ? 0 : a.Ks.f32bad[sd];
        a.Kd.ver[jd] = a.empty ? 0 : a.Ks.ver[sd];
        a.Kd.kf_owner[jd] = -1;  // the K_f row belongs to nobody: kb_update answers RS_ESTATE until a new kb_predict
    }
}

// ------------------------------------------------------------------ kb_unshare: shared -> per replica

// doubles every destination dictionary needs (its shared source's shells at the triangle's sizes), and the largest source
__global__ __launch_bounds__(256) void unshare_count_kernel(BridgeArgs a) {
    const int jd = blockIdx.x * blockDim.x + threadIdx.x;
    if (jd >= a.n_dict) return;
    const int m = a.Ks.m[jd % a.Dd.S];
    a.base[jd] = kb_shells_before((m + KB_CH - 1) / KB_CH, 1);
    if (jd < a.Dd.S) {
        const unsigned long long nsh = (unsigned long long)((m + KB_CH - 1) / KB_CH);
        atomicMax((unsigned long long*)a.words, (unsigned long long)m);
        atomicAdd((unsigned long long*)a.words + 1, nsh * (nsh + 1) / 2);
    }
}

// a wave per destination dictionary (= learner): its tables from shared dictionary s, its control state from replica index[j]
__global__ __launch_bounds__(256) void unshare_tables_kernel(BridgeArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= a.n_dict) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int r = a.index[j], ts = r * D.S + s;
    bridge_dict_words(a, jd, s, a.empty ? 0 : a.Ks.m[s], a.base[jd], lane);
    for (int c = lane; c < D.n_prbs; c += 64) a.Kd.acc[(size_t)jd * D.n_prbs + c] = a.Ks.acc[(size_t)ts * D.n_prbs + c];
    if (lane == 0) bridge_task_words(a, jd, ts);
    if (s == 0) bridge_agent_words(a, j, r, lane);
    if (jd == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[a.n_dict];
}

// 16-byte copies of `n` doubles (a multiple of 64, 16-byte aligned on both sides) by one wave, two in flight per lane
__device__ __forceinline__ void bridge_copy(double* __restrict__ d, const double* __restrict__ sp, uint64_t n, int lane) {
    uint64_t o = (uint64_t)lane * 2;
    for (; o + 128 < n; o += 256) {
        const kb_f64x2 v0 = *(const kb_f64x2*)(sp + o);
        const kb_f64x2 v1 = *(const kb_f64x2*)(sp + o + 128);
        *(kb_f64x2*)(d + o) = v0;
        *(kb_f64x2*)(d + o + 128) = v1;
    }
    if (o < n) *(kb_f64x2*)(d + o) = *(const kb_f64x2*)(sp + o);
}
__device__ __forceinline__ void bridge_zero(double* __restrict__ d, uint64_t n, int lane) {
    const kb_f64x2 z = {0.0, 0.0};
    for (uint64_t o = (uint64_t)lane * 2; o < n; o += 128) *(kb_f64x2*)(d + o) = z;
}

// Shell gather, on kb_fork's work line: the destination's dictionaries fill [64, top) of its pool without a gap; a wave takes
// a piece of KB_FORK_BLK doubles, finds its dictionary by bisection of the scan and its shell by walking the sizes.  Inside a
// shell the page and the lower tiles are copied from the same offsets of the shared source's shell; the partial-sum area behind
// them is zeroed.  Every boundary is a multiple of 64 doubles.  The S sources are read by every agent: through the cache.
__global__ __launch_bounds__(256) void unshare_shells_kernel(BridgeArgs a) {
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
            uint64_t c = 0, sz = kb_shell_doubles(0, 1);
            while (q >= c + sz) {
                c += sz;
                ++b;
                sz = kb_shell_doubles(b, 1);
            }
            const uint64_t in = q - c, common = kb_shell_common(b);
            // the run inside the shell: up to the end of the common part, or of the partial-sum area
            const uint64_t run_end = in < common ? common : sz;
            const uint64_t seg = run_end - in < pe - p ? run_end - in : pe - p;
            const uint64_t so = b < a.src_max_shells ? a.Ks.shell[(size_t)(jd % D.S) * a.src_max_shells + b] : 0ull;
            // a source shell that is missing or does not lie inside the source's pool is never read (zeros instead)
            const bool ok = in < common && so >= 64 && so + kb_shell_doubles(b, 0) <= a.src_pool_doubles;
            if (ok) bridge_copy(a.Kd.pool + p, a.Ks.pool + so + in, seg, lane);
            else bridge_zero(a.Kd.pool + p, seg, lane);
            p += seg;
        }
    }
}

// ------------------------------------------------------------------ kb_share: one agent's dictionaries -> the shared ones

// a wave per destination task (j, s): its control state from source agent index[j]; the waves of replica 0 also write the
// tables of shared dictionary s from dictionary (dict_agent, s)
__global__ __launch_bounds__(256) void share_tables_kernel(BridgeArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int td = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (td >= D.n_envs * D.S) return;
    const int j = td / D.S, s = td - j * D.S;
    const int r = a.index[j], ts = r * D.S + s;
    if (j == 0) bridge_dict_words(a, s, a.dict_agent * D.S + s, a.empty ? 0 : a.Ks.m[a.dict_agent * D.S + s], a.base[s], lane);
    for (int c = lane; c < D.n_prbs; c += 64) a.Kd.acc[(size_t)td * D.n_prbs + c] = a.Ks.acc[(size_t)ts * D.n_prbs + c];
    if (lane == 0) bridge_task_words(a, td, ts);
    if (s == 0) bridge_agent_words(a, j, r, lane);
    if (td == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[D.S];
}

// The same work line over the shared destination's [64, top).  A piece finds its dictionary among the (at most eight) bases and
// its shell by walking the sizes; the page and the lower tiles are copied from the same offsets of the source's shell, and the
// rows of an upper tile (bi,b) behind them are the columns of the lower tile (b,bi) of that same source shell: lane c reads
// element (c, r) and the wave writes row r coalesced.  (The strided reads meet the same 128-byte lines for sixteen rows running,
// and at most eight dictionaries are ever written: the tile stays in the cache, and the call is no hot path.)
__global__ __launch_bounds__(256) void share_shells_kernel(BridgeArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t top = a.base[D.S];
    const uint64_t n_blk = (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK;
    for (uint64_t blk = (uint64_t)blockIdx.x * 4 + wave; blk < n_blk; blk += (uint64_t)gridDim.x * 4) {
        uint64_t p = 64 + blk * KB_FORK_BLK;
        const uint64_t pe = p + KB_FORK_BLK < top ? p + KB_FORK_BLK : top;
        int s = 0;
        while (p < pe) {
            while (a.base[s + 1] <= p) ++s;  // (p < top = base[S]: ends)
            const uint64_t q = p - a.base[s];
            int b = 0;
            uint64_t c = 0, sz = kb_shell_doubles(0, 0);
            while (q >= c + sz) {
                c += sz;
                ++b;
                sz = kb_shell_doubles(b, 0);
            }
            const uint64_t in = q - c, common = kb_shell_common(b);
            // the run inside the shell: up to the end of the common part, or of the upper tile the piece stands in
            const uint64_t run_end = in < common ? common : common + ((in - common) / KB_TILE + 1) * KB_TILE;
            const uint64_t seg = run_end - in < pe - p ? run_end - in : pe - p;
            const uint64_t so = b < a.src_max_shells ? a.Ks.shell[(size_t)(a.dict_agent * D.S + s) * a.src_max_shells + b] : 0ull;
            // a source shell that is missing or does not lie inside the source's pool is never read (zeros instead)
            const bool ok = so >= 64 && so + kb_shell_doubles(b, 1) <= a.src_pool_doubles;
            double* __restrict__ d = a.Kd.pool + p;
            if (!ok) {
                bridge_zero(d, seg, lane);
            } else if (in < common) {
                bridge_copy(d, a.Ks.pool + so + in, seg, lane);
            } else {
                const uint64_t u = in - common;
                const int bi = (int)(u / KB_TILE);                      // upper tile (bi, b), bi < b
                const int r0 = (int)((u - (uint64_t)bi * KB_TILE) >> 6);  // first row of the run; seg is whole rows
                const int nr = (int)(seg >> 6);
                const double* __restrict__ T = a.Ks.pool + so + KB_VEC + (uint64_t)bi * KB_TILE;  // lower tile (b, bi)
                int r = 0;
                for (; r + 1 < nr; r += 2) {
                    const double v0 = T[lane * 64 + r0 + r], v1 = T[lane * 64 + r0 + r + 1];
                    d[r * 64 + lane] = v0;
                    d[(r + 1) * 64 + lane] = v1;
                }
                if (r < nr) d[r * 64 + lane] = T[lane * 64 + r0 + r];
            }
            p += seg;
        }
    }
}

}  // namespace kb

// what a bridge call keeps behind its destination, outside the saved regions (created by the first call)
struct kb_bridge_state {
    uint64_t* d_words = nullptr;  // [4] device result words of kb_unshare's count
    uint64_t* h_words = nullptr;  // pinned [16]: those words (kb_unshare); the bases [S + 1] and, from [12], the source sizes as int32 (kb_share)
    EventSpans spans;             // kernel timing: one pair around the gather
    double last_ms = 0.0;
    uint64_t bytes[2] = {0, 0};   // of the last call's plan: read, written
};

static void kb_bridge_release(kb_handle* k) {
    kb_bridge_state* r = k->bridge;
    if (!r) return;
    if (r->d_words) (void)hipFree(r->d_words);
    if (r->h_words) (void)hipHostFree(r->h_words);
    r->spans.release();
    delete r;
    k->bridge = nullptr;
}

static int kb_bridge_prepare(kb_handle* k) {
    if (!k->bridge) {
        kb_bridge_state* r = new kb_bridge_state();
        k->bridge = r;  // (kb_destroy frees whatever was allocated)
        HIPCHK(k, hipMalloc((void**)&r->d_words, sizeof(uint64_t) * 4));
        HIPCHK(k, hipHostMalloc((void**)&r->h_words, sizeof(uint64_t) * 16, hipHostMallocDefault));
    }
    const int n_dst = k->cfg.n_envs;
    if (!k->d_fork_idx) HIPCHK(k, hipMalloc((void**)&k->d_fork_idx, sizeof(int32_t) * n_dst));
    if (!k->d_fork_base) HIPCHK(k, hipMalloc((void**)&k->d_fork_base, sizeof(uint64_t) * ((size_t)k->n_dict + 2)));
    if (!k->h_fork_idx) HIPCHK(k, hipHostMalloc((void**)&k->h_fork_idx, sizeof(int32_t) * n_dst, hipHostMallocDefault));
    if (!k->h_fork_total) HIPCHK(k, hipHostMalloc((void**)&k->h_fork_total, sizeof(uint64_t), hipHostMallocDefault));
    k->bridge->last_ms = 0.0;
    k->bridge->bytes[0] = k->bridge->bytes[1] = 0;
    k->bridge->spans.on = k->spans.on;
    k->bridge->spans.reset();
    return RS_OK;
}

// kb_config with what the two kinds of handle may differ in masked; towards the triangle the capacity as well (every
// dictionary is then checked against the destination's)
static uint64_t kb_bridge_cfg_hash(const kb_handle* k, bool mask_capacity) {
    kb_config c = k->cfg;
    c.n_envs = 0;
    c.pool_bytes = 0;
    c.shared_dictionary = 0;
    c.first_env = 0;
    if (mask_capacity) c.capacity = 0;
    return fnv1a(&c, sizeof c);
}

// the checks both directions share; `shared` / `priv` are the two handles by kind
static int kb_bridge_check(kb_handle* dst, kb_handle* src, kb_handle* shared, kb_handle* priv, const int32_t* index, int n, int n_src,
                           bool mask_capacity, const char* who) {
    std::string& err = dst->err;
    if (!shared->D.shared) {
        err = std::string(who) + (shared == src ? ": the source is not a shared-dictionary handle (between per-replica handles: kb_fork)"
                                                : ": the destination is not a shared-dictionary handle (between per-replica handles: kb_fork)");
        return RS_EINVAL;
    }
    if (priv->D.shared) {
        err = std::string(who) + (priv == dst ? ": the destination is a shared-dictionary handle: it must hold one agent per replica"
                                              : ": the source is a shared-dictionary handle: it must hold one agent per replica");
        return RS_EINVAL;
    }
    if (src->ref || dst->ref) {
        err = std::string(who) + ": a by-reference handle (kb_deploy_ref) holds its dictionaries in a shared read-only store and no Kinv";
        return RS_ESTATE;
    }
    if (kb_bridge_cfg_hash(dst, mask_capacity) != kb_bridge_cfg_hash(src, mask_capacity)) {
        err = std::string(who) + ": the handles' configurations differ (beyond n_envs, pool_bytes, shared_dictionary and first_env" +
              (mask_capacity ? ", and the capacity)" : ")");
        return RS_EINVAL;
    }
    for (int j = 0; j < n; ++j)
        if (index[j] < 0 || index[j] >= n_src) {
            err = std::string(who) + ": source index " + std::to_string(index[j]) + " of destination replica " + std::to_string(j) + " out of range";
            return RS_EINVAL;
        }
    if (!src->is_reset) {
        err = std::string(who) + ": the source was never reset";
        return RS_ESTATE;
    }
    if (dst->frozen || src->frozen) {
        err = std::string(who) + ": an inference-only handle (kb_deploy) holds no Kinv" +
              (src->frozen ? ": rebuild it first (kb_fork_rebuild)" : ": the destination must be a learning handle (kb_create)");
        return RS_ESTATE;
    }
    if (dst->device != src->device) {
        err = std::string(who) + ": the handles live on different devices";
        return RS_ESTATE;
    }
    if (shared->round_open) {
        err = std::string(who) + ": the shared-dictionary handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    return RS_OK;
}

// what kb_reset restarts in the destination, on its stream (the tables kernels write stats, fver and the retained hits)
static int kb_bridge_restart(kb_handle* dst) {
    const size_t T = (size_t)dst->T;
    HIPCHK(dst, hipMemsetAsync(dst->d_gstats, 0, sizeof(uint64_t) * 32, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.hv_work, 0, sizeof(unsigned long long) * 8, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.heavy, 0, sizeof(int32_t) * 4, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.big, 0, sizeof(int32_t) * 2 * (1 + KB_BIG_MAX), dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.isbig, 0, sizeof(int32_t) * 2 * T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->K.pool, 0, sizeof(double) * 64, dst->stream));  // (below every shell; never read)
    kb_prune_restart(dst);
    return RS_OK;
}

static int kb_bridge_leave(kb_handle* dst, kb_handle* src) {
    const int rc = stream_after(dst, &dst->ev_fork_out, dst->stream, src->stream);
    if (dst->h_seen) dst->h_seen[0] = dst->h_seen[1] = 0;
    dst->gemm_fresh = false;
    dst->big_par = 0;
    dst->round_open = false;
    dst->is_reset = true;
    return rc;
}

extern "C" int kb_unshare(kb_handle* dst, kb_handle* src, const int32_t* src_index) {
    const char* who = "kb_unshare";
    if (!dst || !src || !src_index) return RS_EINVAL;
    if (dst == src) {
        dst->err = "kb_unshare: source and destination must be different handles";
        return RS_EINVAL;
    }
    int rc = kb_bridge_check(dst, src, src, dst, src_index, dst->cfg.n_envs, src->cfg.n_envs, true, who);
    if (rc != RS_OK) return rc;
    std::string why;
    if ((rc = kb_fork_classify(src, &why)) != RS_OK || (rc = kb_fork_classify(dst, &why)) != RS_OK) {
        dst->err = std::string(who) + ": " + why;
        return rc;
    }
    const int n_dst = dst->cfg.n_envs, ND = dst->n_dict;
    HIPCHK(dst, hipSetDevice(dst->device));
    kb_drop_graph(dst);
    if ((rc = kb_bridge_prepare(dst)) != RS_OK) return rc;
    kb_bridge_state* r = dst->bridge;
    memcpy(dst->h_fork_idx, src_index, sizeof(int32_t) * n_dst);  // (a previous call ended with its host wait: the buffer is free)
    if ((rc = stream_after(dst, &dst->ev_fork_in, src->stream, dst->stream)) != RS_OK) return rc;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, sizeof(int32_t) * n_dst, hipMemcpyHostToDevice, dst->stream));
    HIPCHK(dst, hipMemsetAsync(r->d_words, 0, sizeof(uint64_t) * 4, dst->stream));
    if ((rc = kb_bridge_restart(dst)) != RS_OK) return rc;
    kb::BridgeArgs a;
    memset(&a, 0, sizeof a);
    a.Dd = dst->D;
    a.Kd = dst->K;
    a.Ks = src->K;
    a.src_pool_doubles = src->D.pool_doubles;
    a.src_max_shells = src->D.max_shells;
    a.n_dict = ND;
    a.index = dst->d_fork_idx;
    a.base = dst->d_fork_base;
    a.words = r->d_words;
    a.prev_s = src->d_prev_state;
    a.prev_d = dst->d_prev_state;
    a.hits_d = dst->d_hits;
    uint64_t* d_total = dst->d_fork_base + ND + 1;
    hipLaunchKernelGGL(kb::unshare_count_kernel, dim3((unsigned)((ND + 255) / 256)), dim3(256), 0, dst->stream, a);
    hipLaunchKernelGGL(kb::fork_scan_kernel, dim3(1), dim3(1024), 0, dst->stream, a.base, ND, d_total);
    HIPCHK(dst, hipGetLastError());
    dst->h_fork_total[0] = 0;
    r->h_words[0] = r->h_words[1] = 0;
    HIPCHK(dst, hipMemcpyAsync(dst->h_fork_total, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipMemcpyAsync(r->h_words, r->d_words, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));  // the one host wait
    const uint64_t top = dst->h_fork_total[0], m_max = r->h_words[0];
    const bool too_large = m_max > (uint64_t)dst->cfg.capacity;
    a.empty = (too_large || top > dst->D.pool_doubles) ? 1 : 0;
    hipEvent_t e_end;
    HIPCHK(dst, r->spans.begin(dst->stream, 0, &e_end));
    hipLaunchKernelGGL(kb::unshare_tables_kernel, dim3((unsigned)((ND + 3) / 4)), dim3(256), 0, dst->stream, a);
    if (!a.empty && top > 64) {
        const uint64_t n_blk = (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK;
        const uint64_t grid = (n_blk + 3) / 4;
        hipLaunchKernelGGL(kb::unshare_shells_kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, dst->stream, a);
        // the plan: everything in [64, top) is written; read is all of it but the partial-sum areas, 128 doubles per stored
        // tile of every agent's copy
        r->bytes[1] = (top - 64) * 8;
        r->bytes[0] = r->bytes[1] - (uint64_t)n_dst * r->h_words[1] * 128 * 8;
    }
    if (e_end) HIPCHK(dst, hipEventRecord(e_end, dst->stream));
    HIPCHK(dst, hipGetLastError());
    if ((rc = kb_bridge_leave(dst, src)) != RS_OK) return rc;
    if (too_large) {
        dst->err = std::string(who) + ": a source dictionary holds " + std::to_string(m_max) + " landmarks, the destination's capacity is " +
                   std::to_string(dst->cfg.capacity) + "; the destination was left reset with empty dictionaries";
        return RS_EOVERFLOW;
    }
    if (a.empty) {
        dst->err = std::string(who) + ": the source dictionaries need " + std::to_string(top * 8) + " bytes of pool, the destination's pool has " +
                   std::to_string((uint64_t)dst->D.pool_doubles * 8) + "; the destination was left reset with empty dictionaries";
        return RS_EOVERFLOW;
    }
    return RS_OK;
}

extern "C" int kb_share(kb_handle* dst, kb_handle* src, int32_t dict_agent, const int32_t* ctl_index) {
    const char* who = "kb_share";
    if (!dst || !src) return RS_EINVAL;
    if (dst == src) {
        dst->err = "kb_share: source and destination must be different handles";
        return RS_EINVAL;
    }
    const int n_dst = dst->cfg.n_envs, S = dst->cfg.n_slices;
    // NULL: every replica takes the control state of dict_agent (whose own range is checked below, behind the handles' kinds)
    std::vector<int32_t> idx((size_t)n_dst, dict_agent >= 0 && dict_agent < src->cfg.n_envs ? dict_agent : 0);
    if (ctl_index) memcpy(idx.data(), ctl_index, sizeof(int32_t) * (size_t)n_dst);
    int rc = kb_bridge_check(dst, src, dst, src, idx.data(), n_dst, src->cfg.n_envs, false, who);
    if (rc != RS_OK) return rc;
    if (dict_agent < 0 || dict_agent >= src->cfg.n_envs) {
        dst->err = std::string(who) + ": dict_agent " + std::to_string(dict_agent) + " out of range";
        return RS_EINVAL;
    }
    std::string why;
    if ((rc = kb_fork_classify(src, &why)) != RS_OK || (rc = kb_fork_classify(dst, &why)) != RS_OK) {
        dst->err = std::string(who) + ": " + why;
        return rc;
    }
    HIPCHK(dst, hipSetDevice(dst->device));
    kb_drop_graph(dst);
    if ((rc = kb_bridge_prepare(dst)) != RS_OK) return rc;
    kb_bridge_state* r = dst->bridge;
    memcpy(dst->h_fork_idx, idx.data(), sizeof(int32_t) * (size_t)n_dst);
    if ((rc = stream_after(dst, &dst->ev_fork_in, src->stream, dst->stream)) != RS_OK) return rc;
    // (before the wait, so that the pinned index is free again when the call returns)
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_idx, dst->h_fork_idx, sizeof(int32_t) * (size_t)n_dst, hipMemcpyHostToDevice, dst->stream));
    // the one host wait: the S sizes of the chosen agent -- the layout of at most eight dictionaries is then the host's own sum
    int32_t* h_m = (int32_t*)(r->h_words + 12);
    for (int s = 0; s < S; ++s) h_m[s] = 0;
    HIPCHK(dst, hipMemcpyAsync(h_m, src->K.m + (size_t)dict_agent * S, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    kb::BridgeArgs a;
    memset(&a, 0, sizeof a);
    uint64_t top = 64;
    for (int s = 0; s < S; ++s) {
        const int m = h_m[s] < 0 ? 0 : h_m[s] > src->cfg.capacity ? src->cfg.capacity : h_m[s];  // (capacities are equal: it fits dst's)
        r->h_words[s] = top;
        top += kb::kb_shells_before_full((m + KB_CH - 1) / KB_CH);
    }
    r->h_words[S] = top;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_base, r->h_words, sizeof(uint64_t) * (size_t)(S + 1), hipMemcpyHostToDevice, dst->stream));
    if ((rc = kb_bridge_restart(dst)) != RS_OK) return rc;
    // what the shared mode derives from a dictionary is rebuilt by the next step: Q (workq) by every launch of the scoring
    // product, F / E by it unless gemm_fresh says they are current (cleared by kb_bridge_leave); the proposal cursors of an
    // earlier round name candidates of dictionaries that are gone
    HIPCHK(dst, hipMemsetAsync(dst->d_cursor, 0xFF, sizeof(int32_t) * (size_t)dst->T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_cstar, 0xFF, sizeof(int32_t) * (size_t)dst->T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_counts, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_mcounts, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_taken, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    a.Dd = dst->D;
    a.Kd = dst->K;
    a.Ks = src->K;
    a.src_pool_doubles = src->D.pool_doubles;
    a.src_max_shells = src->D.max_shells;
    a.n_dict = S;
    a.dict_agent = dict_agent;
    a.index = dst->d_fork_idx;
    a.base = dst->d_fork_base;
    a.prev_s = src->d_prev_state;
    a.prev_d = dst->d_prev_state;
    a.hits_d = dst->d_hits;
    a.empty = top > dst->D.pool_doubles ? 1 : 0;
    hipEvent_t e_end;
    HIPCHK(dst, r->spans.begin(dst->stream, 0, &e_end));
    hipLaunchKernelGGL(kb::share_tables_kernel, dim3((unsigned)((dst->T + 3) / 4)), dim3(256), 0, dst->stream, a);
    if (!a.empty && top > 64) {
        const uint64_t n_blk = (top - 64 + KB_FORK_BLK - 1) / KB_FORK_BLK;
        const uint64_t grid = (n_blk + 3) / 4;
        hipLaunchKernelGGL(kb::share_shells_kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, dst->stream, a);
        // the plan: everything in [64, top) is written, and as much is read -- every off-diagonal lower tile once per orientation
        r->bytes[0] = r->bytes[1] = (top - 64) * 8;
    }
    if (e_end) HIPCHK(dst, hipEventRecord(e_end, dst->stream));
    HIPCHK(dst, hipGetLastError());
    if ((rc = kb_bridge_leave(dst, src)) != RS_OK) return rc;
    if (a.empty) {
        dst->err = std::string(who) + ": the source dictionaries need " + std::to_string(top * 8) + " bytes of pool, the destination's pool has " +
                   std::to_string((uint64_t)dst->D.pool_doubles * 8) + "; the destination was left reset with empty dictionaries";
        return RS_EOVERFLOW;
    }
    return RS_OK;
}

extern "C" int kb_bridge_time_ms(kb_handle* k, double* ms, uint64_t bytes[2]) {
    if (!k || !ms || !bytes) return RS_EINVAL;
    *ms = 0.0;
    bytes[0] = bytes[1] = 0;
    kb_bridge_state* r = k->bridge;
    if (!r) return RS_OK;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    HIPCHK(k, r->spans.drain([&](int, double t) { r->last_ms = t; }));
    *ms = r->last_ms;
    bytes[0] = r->bytes[0];
    bytes[1] = r->bytes[1];
    return RS_OK;
}
