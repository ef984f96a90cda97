// kb_bridge.hip -- dictionaries cross between a shared-dictionary handle and a per-replica one: kb_unshare (shared -> one private
// copy per agent) and kb_share (one agent's dictionaries -> the shared ones of a fleet).  #included by rs_api.hip after
// kb_rebuild.hip: it uses the agent handle and kb_fork.hip's transfer sequence -- the work line, the gather helpers, the host
// steps -- with its own cuts and bodies.
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

// destination task td := source task ts, by one wave: the accuracy row and the control state, and -- the cache of the last
// kb_predict does not cross storages -- f_last / m_last cleared
__device__ __forceinline__ void bridge_task_words(const XferArgs& a, int td, int ts, int lane) {
    for (int c = lane; c < a.Dd.n_prbs; c += 64) a.Kd.acc[(size_t)td * a.Dd.n_prbs + c] = a.Ks.acc[(size_t)ts * a.Dd.n_prbs + c];
    if (lane == 0) {
        a.Kd.f_last[td] = 0.0;
        a.Kd.m_last[td] = 0;
        gather_task_words(a.Kd, a.Ks, a.hits_d, td, ts);
    }
}
// the per-dictionary tables of destination dictionary jd := those of source dictionary sd, laid out whole from a.base[jd]
__device__ __forceinline__ void bridge_dict_words(const XferArgs& a, int jd, int sd, int lane) {
    const int m = a.empty ? 0 : a.Ks.m[sd];
    gather_dict_tables(a.Dd, a.Kd, a.Ks, jd, sd, m, a.empty, a.base[jd], lane);
    if (lane == 0) {
        gather_dict_words(a.Kd, a.Ks, jd, sd, m, a.empty);
        a.Kd.kf_owner[jd] = -1;  // the K_f row belongs to nobody: kb_update answers RS_ESTATE until a new kb_predict
    }
}

// ------------------------------------------------------------------ kb_unshare: shared -> per replica

// doubles every destination dictionary needs (its shared source's shells at the triangle's sizes), and the largest source
__global__ __launch_bounds__(256) void unshare_count_kernel(XferArgs a) {
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
__global__ __launch_bounds__(256) void unshare_tables_kernel(XferArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= a.n_dict) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int r = a.index[j];
    bridge_dict_words(a, jd, s, lane);
    bridge_task_words(a, jd, r * D.S + s, lane);
    if (s == 0) gather_agent_words(D, a.Kd, a.Ks, a.prev_d, a.prev_s, j, r, lane);
    if (jd == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[a.n_dict];
}

// Shell gather: inside a shell the page and the lower tiles are copied from the same offsets of the shared source's shell; the
// partial-sum area behind them is zeroed.  The S sources are read by every agent: through the cache.
__global__ __launch_bounds__(256) void unshare_shells_kernel(XferArgs a) {
    const int lane = threadIdx.x & 63;
    line_walk(a.base, a.n_dict, 1, KbCutCommon(), [&](int jd, int b, uint64_t in, uint64_t p, uint64_t seg) {
        const uint64_t so = in < kb_shell_common(b) ? src_shell(a, jd % a.Dd.S, b, kb_shell_doubles(b, 0)) : 0ull;
        if (so) wave_copy(a.Kd.pool + p, a.Ks.pool + so + in, seg, lane);
        else wave_zero(a.Kd.pool + p, seg, lane);
    });
}

// ------------------------------------------------------------------ kb_share: one agent's dictionaries -> the shared ones

// a wave per destination task (j, s): its control state from source agent index[j]; the waves of replica 0 also write the
// tables of shared dictionary s from dictionary (dict_agent, s)
__global__ __launch_bounds__(256) void share_tables_kernel(XferArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int td = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (td >= D.n_envs * D.S) return;
    const int j = td / D.S, s = td - j * D.S;
    const int r = a.index[j];
    if (j == 0) bridge_dict_words(a, s, a.dict_agent * D.S + s, lane);
    bridge_task_words(a, td, r * D.S + s, lane);
    if (s == 0) gather_agent_words(D, a.Kd, a.Ks, a.prev_d, a.prev_s, j, r, lane);
    if (td == 0 && lane == 0) a.Kd.pool_top[0] = a.empty ? 64ull : a.base[D.S];
}

// Shell gather over the shared destination's (at most eight) dictionaries: the page and the lower tiles are copied from the same
// offsets of the source's shell, and the rows of an upper tile (bi,b) behind them are the columns of the lower tile (b,bi) of
// that same source shell: lane c reads element (c, r) and the wave writes row r coalesced.  (The strided reads meet the same
// 128-byte lines for sixteen rows running, and at most eight dictionaries are ever written: the tile stays in the cache, and the
// call is no hot path.)
__global__ __launch_bounds__(256) void share_shells_kernel(XferArgs a) {
    const int lane = threadIdx.x & 63;
    line_walk(a.base, a.n_dict, 0, KbCutTiles(), [&](int s, int b, uint64_t in, uint64_t p, uint64_t seg) {
        const uint64_t so = src_shell(a, a.dict_agent * a.Dd.S + s, b, kb_shell_doubles(b, 1)), common = kb_shell_common(b);
        double* __restrict__ d = a.Kd.pool + p;
        if (!so) {
            wave_zero(d, seg, lane);
        } else if (in < common) {
            wave_copy(d, a.Ks.pool + so + in, seg, lane);
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
    });
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
    k->bridge->last_ms = 0.0;
    k->bridge->bytes[0] = k->bridge->bytes[1] = 0;
    k->bridge->spans.on = k->spans.on;
    k->bridge->spans.reset();
    return RS_OK;
}

// the checks both directions share; `shared` / `priv` are the two handles by kind
static int kb_bridge_check(kb_handle* dst, kb_handle* src, kb_handle* shared, kb_handle* priv, const int32_t* index, int n,
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
    // (towards the triangle the capacity may differ: every dictionary is then checked against the destination's)
    const int rc = kb_xfer_check(dst, src, index, n, true, mask_capacity, "replica", " and no Kinv", &err, who);
    if (rc != RS_OK) return rc;
    if (dst->frozen || src->frozen) {
        err = std::string(who) + ": an inference-only handle (kb_deploy) holds no Kinv" +
              (src->frozen ? ": rebuild it first (kb_fork_rebuild)" : ": the destination must be a learning handle (kb_create)");
        return RS_ESTATE;
    }
    if (shared->round_open) {
        err = std::string(who) + ": the shared-dictionary handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    return RS_OK;
}

extern "C" int kb_unshare(kb_handle* dst, kb_handle* src, const int32_t* src_index) {
    const char* who = "kb_unshare";
    if (!dst || !src || !src_index) return RS_EINVAL;
    if (dst == src) {
        dst->err = "kb_unshare: source and destination must be different handles";
        return RS_EINVAL;
    }
    int rc = kb_bridge_check(dst, src, src, dst, src_index, dst->cfg.n_envs, true, who);
    if (rc != RS_OK) return rc;
    if ((rc = kb_xfer_enter(dst, src, src_index, who)) != RS_OK) return rc;
    if ((rc = kb_bridge_prepare(dst)) != RS_OK) return rc;
    kb_bridge_state* r = dst->bridge;
    kb::XferArgs a = kb_xfer_args(dst, src, dst->n_dict);
    a.words = r->d_words;
    uint64_t top;
    HIPCHK(dst, hipMemsetAsync(r->d_words, 0, sizeof(uint64_t) * 4, dst->stream));
    kb_xfer_launch(dst, kb::unshare_count_kernel, a, (size_t)a.n_dict, 256);
    r->h_words[0] = r->h_words[1] = 0;
    HIPCHK(dst, hipMemcpyAsync(r->h_words, r->d_words, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, dst->stream));
    if ((rc = kb_xfer_scan_wait(dst, a, &top)) != RS_OK) return rc;  // the one host wait
    const uint64_t m_max = r->h_words[0];
    const bool too_large = m_max > (uint64_t)dst->cfg.capacity;
    a.empty = (too_large || top > dst->D.pool_doubles) ? 1 : 0;
    hipEvent_t e_end;
    HIPCHK(dst, r->spans.begin(dst->stream, 0, &e_end));
    kb_xfer_launch(dst, kb::unshare_tables_kernel, a, (size_t)a.n_dict, 4);
    kb_xfer_launch_line(dst, kb::unshare_shells_kernel, a, top);
    if (!a.empty && top > 64) {
        // the plan: everything in [64, top) is written; read is all of it but the partial-sum areas, 128 doubles per stored
        // tile of every agent's copy
        r->bytes[1] = (top - 64) * 8;
        r->bytes[0] = r->bytes[1] - (uint64_t)dst->cfg.n_envs * r->h_words[1] * 128 * 8;
    }
    if (e_end) HIPCHK(dst, hipEventRecord(e_end, dst->stream));
    HIPCHK(dst, hipGetLastError());
    if ((rc = kb_xfer_leave(dst, src)) != RS_OK) return rc;
    if (too_large) {
        dst->err = std::string(who) + ": a source dictionary holds " + std::to_string(m_max) + " landmarks, the destination's capacity is " +
                   std::to_string(dst->cfg.capacity) + "; the destination was left reset with empty dictionaries";
        return RS_EOVERFLOW;
    }
    return a.empty ? kb_xfer_overflow(dst, who, top) : RS_OK;
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
    int rc = kb_bridge_check(dst, src, dst, src, idx.data(), n_dst, false, who);
    if (rc != RS_OK) return rc;
    if (dict_agent < 0 || dict_agent >= src->cfg.n_envs) {
        dst->err = std::string(who) + ": dict_agent " + std::to_string(dict_agent) + " out of range";
        return RS_EINVAL;
    }
    if ((rc = kb_xfer_enter(dst, src, idx.data(), who)) != RS_OK) return rc;
    if ((rc = kb_bridge_prepare(dst)) != RS_OK) return rc;
    kb_bridge_state* r = dst->bridge;
    // the one host wait: the S sizes of the chosen agent -- the layout of at most eight dictionaries is then the host's own sum
    int32_t* h_m = (int32_t*)(r->h_words + 12);
    for (int s = 0; s < S; ++s) h_m[s] = 0;
    HIPCHK(dst, hipMemcpyAsync(h_m, src->K.m + (size_t)dict_agent * S, sizeof(int32_t) * (size_t)S, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    uint64_t top = 64;
    for (int s = 0; s < S; ++s) {
        const int m = h_m[s] < 0 ? 0 : h_m[s] > src->cfg.capacity ? src->cfg.capacity : h_m[s];  // (capacities are equal: it fits dst's)
        r->h_words[s] = top;
        top += kb::kb_shells_before((m + KB_CH - 1) / KB_CH, 0);
    }
    r->h_words[S] = top;
    HIPCHK(dst, hipMemcpyAsync(dst->d_fork_base, r->h_words, sizeof(uint64_t) * (size_t)(S + 1), hipMemcpyHostToDevice, dst->stream));
    // what the shared mode derives from a dictionary is rebuilt by the next step: Q (workq) by every launch of the scoring
    // product, F / E by it unless gemm_fresh says they are current (cleared by kb_xfer_leave); the proposal cursors of an
    // earlier round name candidates of dictionaries that are gone
    HIPCHK(dst, hipMemsetAsync(dst->d_cursor, 0xFF, sizeof(int32_t) * (size_t)dst->T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_cstar, 0xFF, sizeof(int32_t) * (size_t)dst->T, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_counts, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_mcounts, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    HIPCHK(dst, hipMemsetAsync(dst->d_taken, 0, sizeof(int32_t) * (size_t)S, dst->stream));
    kb::XferArgs a = kb_xfer_args(dst, src, S);
    a.dict_agent = dict_agent;
    a.empty = top > dst->D.pool_doubles ? 1 : 0;
    hipEvent_t e_end;
    HIPCHK(dst, r->spans.begin(dst->stream, 0, &e_end));
    kb_xfer_launch(dst, kb::share_tables_kernel, a, (size_t)dst->T, 4);
    kb_xfer_launch_line(dst, kb::share_shells_kernel, a, top);
    // the plan: everything in [64, top) is written, and as much is read -- every off-diagonal lower tile once per orientation
    if (!a.empty && top > 64) r->bytes[0] = r->bytes[1] = (top - 64) * 8;
    if (e_end) HIPCHK(dst, hipEventRecord(e_end, dst->stream));
    HIPCHK(dst, hipGetLastError());
    if ((rc = kb_xfer_leave(dst, src)) != RS_OK) return rc;
    return a.empty ? kb_xfer_overflow(dst, who, top) : RS_OK;
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
