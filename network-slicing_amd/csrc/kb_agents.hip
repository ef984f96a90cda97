// kb_agents.hip -- agent files: kb_export_bytes / kb_export_agents pack trained agents into a compact, layout-independent blob,
// kb_agents_info validates one on the host, kb_import_agents builds an inference-only handle (kb_deploy's) from it.
// #included by rs_api.hip after kb_ref.hip: it uses the agent handle and the fork's scan and checks, and changes none of their
// kernels.
//
// THE FILE ("KBAGENT1", little-endian, every array 8-byte aligned; ranslice/agent_file.py writes and reads the same bytes):
//   header (kb_agents_header, 120 bytes): magic, total bytes, FNV-1a of everything behind the hash field, agents n, and what of
//     kb_config defines an agent (n_slices S, n_prbs, capacity, dims[8], alfa, acc_lo, acc_hi, gamma, eta), then the doubles of
//     all dictionaries together -- so that the header alone implies the file's size
//   dense agent-major tables of what kb_fork copies per agent: m[n][S], f32bad[n][S] (int32); action, security, margins
//     [n][S], adjusted[n] (int32); acc[n][S][n_prbs] (f64); seeds[n] (uint64); tie_ctr[n][S] (uint32); the observation the
//     resident loop chose its last action in [n][nv] (float32); the flag word [n] (int32), verbatim
//   the dictionaries (16-byte aligned), in (agent, slice) order at an exclusive scan of m (d + 1), d = dims[s] + 1:
//     landmarks[m][d] f64 LANDMARK-MAJOR (the shape kb_get_learner returns and the reference holds), then coeff[m]
// Slot j of the file is slot j of the dictionary: the order of every sum of the scoring kernels depends on it.  No shell
// offsets, no padding lanes, no scratch rows, no Kinv: the file is a function of the arguments and the agents' state alone.
//
// Pages are coordinate-major (64 landmarks per row, kb_kbrl.hip "Storage"), the file landmark-major: both directions transpose
// a 64 x d tile through the wave's own LDS.  Rows of the tile are KB_AGENT_LD(d) = d | 1 doubles apart: odd, so that the
// strided side (ds_write_b64 in groups of 16 lanes over 32 banks when packing, ds_read_b64 in groups of 32 lanes over 64 banks
// when building) meets every bank once; 64 x 17 doubles = 8,704 bytes per wave at d = 16.

#include <cmath>

namespace kb {

#define KB_AGENT_LD_MAX 17

struct AgentTables {  // the file's tables and dictionaries, in a device copy of the blob
    int32_t *m, *f32bad, *action, *security, *margins, *adjusted;
    double* acc;
    uint64_t* seeds;
    uint32_t* tie_ctr;
    float* prev;
    int32_t* flags;
    double* dict;
};

struct AgentArgs {
    KbDev D;               // the handle: the source of an export, the new handle of an import
    KbState K;
    AgentTables F;
    const int32_t* index;  // export: [n_agents] agent of the handle behind agent j of the file; import: nullptr (the same agent)
    int32_t n_dict;        // dictionaries of the file = agents x S
    int32_t pack;          // 1: handle -> file, 0: file -> handle
    uint64_t* pbase;       // [n_dict + 1] 64 + the doubles of the vector pages (KB_VEC per started 64 landmarks) of the dictionaries
                           //   before: the chunks' work line, and the pool of an imported handle (kb_deploy's layout)
    uint64_t* fbase;       // [n_dict + 1] 64 + the doubles m (d + 1) of the file's dictionaries before
    uint64_t* total;       // [3] the two tops, and the doubles the pack kernel's plan reads (whole rows of the pages), for the host
    float* prev;           // the handle's d_prev_state
    int32_t* hits;
    int32_t* bad;          // import: raised by a coordinate or coefficient that is not finite
};

__device__ __forceinline__ int agents_dict(const AgentArgs& a, int jd) {  // dictionary of the handle behind dictionary jd of the file
    if (!a.index) return jd;
    const int j = jd / a.D.S;
    return a.index[j] * a.D.S + (jd - j * a.D.S);
}

// sizes of every dictionary of the file on both lines (fork_scan_kernel then scans each in place)
__global__ __launch_bounds__(256) void agents_count_kernel(AgentArgs a) {
    const int jd = blockIdx.x * blockDim.x + threadIdx.x;
    if (jd >= a.n_dict) return;
    const int s = jd % a.D.S;
    const int m = a.pack ? a.K.m[agents_dict(a, jd)] : a.F.m[jd];
    const unsigned long long chunks = (unsigned long long)((m + KB_CH - 1) / KB_CH);
    a.pbase[jd] = chunks * KB_VEC;
    a.fbase[jd] = (uint64_t)m * (uint64_t)(a.D.dims[s] + 2);
    if (chunks) atomicAdd((unsigned long long*)&a.total[2], chunks * (unsigned long long)(a.D.dims[s] + 2) * KB_CH);  // (integer sum)
}

// The per-agent tables, a wave per dictionary as fork_tables_kernel gathers them.  Packing copies what travels; building also
// writes the shell table from the scan and restarts what kb_reset / kb_fork restart (the heads, links and the off-grid count
// are agents_finish_kernel's).
__global__ __launch_bounds__(256) void agents_tables_kernel(AgentArgs a) {
    const KbDev& D = a.D;
    const KbState& K = a.K;
    const AgentTables& F = a.F;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= a.n_dict) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int sd = agents_dict(a, jd), r = sd / D.S;
    if (a.pack) {
        for (int c = lane; c < D.n_prbs; c += 64) F.acc[(size_t)jd * D.n_prbs + c] = K.acc[(size_t)sd * D.n_prbs + c];
        if (lane == 0) {
            F.m[jd] = K.m[sd];
            F.f32bad[jd] = K.f32bad[sd] != 0;
            F.action[jd] = K.action[sd];
            F.security[jd] = K.security[sd];
            F.margins[jd] = K.margins[sd];
            F.tie_ctr[jd] = K.tie_ctr[sd];
        }
        if (s == 0) {
            if (lane == 0) {
                F.adjusted[j] = K.adjusted[r];
                F.seeds[j] = K.seeds[r];
                F.flags[j] = K.err[r];
            }
            for (int q = lane; q < D.nv; q += 64) F.prev[(size_t)j * D.nv + q] = a.prev[(size_t)r * D.nv + q];
        }
        return;
    }
    const int m = F.m[jd];
    const int nsh = (m + KB_CH - 1) / KB_CH;
    const uint64_t at = a.pbase[jd];
    for (int b = lane; b < D.max_shells; b += 64) K.shell[(size_t)jd * D.max_shells + b] = b < nsh ? at + (uint64_t)b * KB_VEC : 0ull;
    for (int c = lane; c < D.n_prbs; c += 64) K.acc[(size_t)jd * D.n_prbs + c] = F.acc[(size_t)jd * D.n_prbs + c];
    if (lane == 0) {
        K.m[jd] = m;
        K.f32bad[jd] = F.f32bad[jd] != 0;  // (agents_build_kernel ORs in what it finds itself)
        K.ver[jd] = 0;
        K.kf_owner[jd] = -1;  // the kb_predict cache: nobody's
        K.f_last[jd] = 0.0;
        K.m_last[jd] = -1;
        K.tie_ctr[jd] = F.tie_ctr[jd];
        K.action[jd] = F.action[jd];
        K.security[jd] = F.security[jd];
        K.margins[jd] = F.margins[jd];
        K.fver[jd] = -1;  // no stored scores: an optimisation no result depends on
        for (int q = 0; q < 4; ++q) K.stats[(size_t)jd * 4 + q] = 0;
        a.hits[jd] = 0;
    }
    if (s == 0) {
        if (lane == 0) {
            K.seeds[j] = F.seeds[j];
            K.adjusted[j] = F.adjusted[j];
            K.err[j] = F.flags[j];
        }
        for (int q = lane; q < D.nv; q += 64) a.prev[(size_t)j * D.nv + q] = F.prev[(size_t)j * D.nv + q];
    }
    if (jd == 0 && lane == 0) K.pool_top[0] = a.pbase[a.n_dict];
}

// position in the LDS tile of element i of a run of landmark-major rows of d doubles
__device__ __forceinline__ int agents_tile_at(int i, int d, int ld) {
    const int r = i / d;
    return r * ld + (i - r * d);
}

// Pack.  The work line is the chosen dictionaries' chunks laid end to end; a wave takes one chunk of 64 landmarks: the d
// coordinate rows of its vector page (64 lanes x 8 bytes, coalesced) into the tile, then the chunk's min(64, m - 64 b)
// landmark-major rows -- ONE contiguous run of the file -- out with 16-byte stores (the run starts 8-byte aligned: an odd
// first double and an odd last one go alone), and the coefficient row.  A ragged last chunk writes its live rows only.
__global__ __launch_bounds__(256) void agents_pack_kernel(AgentArgs a) {
    __shared__ double tiles[4][64 * KB_AGENT_LD_MAX];
    const KbDev& D = a.D;
    const KbState& K = a.K;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double* T = tiles[wave];
    const uint64_t n_chunks = (a.pbase[a.n_dict] - 64) / KB_VEC;
    for (uint64_t c = (uint64_t)blockIdx.x * 4 + wave; c < n_chunks; c += (uint64_t)gridDim.x * 4) {
        const uint64_t p = 64 + c * KB_VEC;
        const int jd = kb_line_find(a.pbase, a.n_dict, p);  // (empty dictionaries share their start with the next)
        const int b = (int)((p - a.pbase[jd]) / KB_VEC);
        const int s = jd % D.S, d = D.dims[s] + 1, ld = d | 1;
        const int sd = agents_dict(a, jd);
        const int m = K.m[sd];
        int cnt = m - KB_CH * b;
        cnt = cnt < 0 ? 0 : cnt > KB_CH ? KB_CH : cnt;
        const uint64_t so = b < D.max_shells ? K.shell[(size_t)sd * D.max_shells + b] : 0ull;
        // a shell that is missing or does not lie inside the pool is never read (zeros instead), as in fork_shells_kernel
        const bool ok = so >= 64 && so + kb_shell_doubles(b, D.tri) <= D.pool_doubles;
        const double* __restrict__ P = K.pool + so;
        for (int q = 0; q < d; ++q) T[lane * ld + q] = ok ? P[q * KB_CH + lane] : 0.0;
        const double co = ok ? P[KB_ROW_CO * KB_CH + lane] : 0.0;
        bin_wave_sync<false>();
        double* __restrict__ out = a.F.dict + (a.fbase[jd] - 64);
        double* __restrict__ o = out + (size_t)KB_CH * b * d;
        const int total = cnt * d;
        const int head = (int)(((uintptr_t)o >> 3) & 1);
        if (head && lane == 0 && total > 0) o[0] = T[0];
        for (int i = head + 2 * lane; i < total; i += 128) {
            if (i + 1 < total) {
                const kb_f64x2 v = {T[agents_tile_at(i, d, ld)], T[agents_tile_at(i + 1, d, ld)]};
                *(kb_f64x2*)(o + i) = v;
            } else {
                o[i] = T[agents_tile_at(i, d, ld)];
            }
        }
        if (lane < cnt) out[(size_t)m * d + KB_CH * b + lane] = co;
        bin_wave_sync<false>();  // (the tile is free for the wave's next chunk)
    }
}

// Build, the reverse: a wave per chunk of the destination's pages writes the WHOLE page -- the coordinate rows, the float32
// copy of the ten state coordinates of an eMBB dictionary (KB_ROW_F32), the coefficient row, the grid index of the last
// coordinate by grid_index() itself (what apply_update stores on insertion), and zeros in every other row and in every lane
// from m on.  The chain links are agents_finish_kernel's.  f32bad is found again from the values (the file's flag is ORed in by
// agents_tables_kernel: the source's is sticky across kb_prune, a host-packed file's need not be true).
__global__ __launch_bounds__(256) void agents_build_kernel(AgentArgs a) {
    __shared__ double tiles[4][64 * KB_AGENT_LD_MAX];
    const KbDev& D = a.D;
    const KbState& K = a.K;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double* T = tiles[wave];
    const uint64_t n_chunks = (a.pbase[a.n_dict] - 64) / KB_VEC;
    for (uint64_t c = (uint64_t)blockIdx.x * 4 + wave; c < n_chunks; c += (uint64_t)gridDim.x * 4) {
        const uint64_t p = 64 + c * KB_VEC;
        const int jd = kb_line_find(a.pbase, a.n_dict, p);  // (empty dictionaries share their start with the next)
        const int b = (int)((p - a.pbase[jd]) / KB_VEC);
        const int s = jd % D.S, d = D.dims[s] + 1, ld = d | 1;
        const int m = a.F.m[jd];
        int cnt = m - KB_CH * b;
        cnt = cnt < 0 ? 0 : cnt > KB_CH ? KB_CH : cnt;
        const double* __restrict__ in = a.F.dict + (a.fbase[jd] - 64);
        const double* __restrict__ o = in + (size_t)KB_CH * b * d;
        const int total = cnt * d;
        const int head = (int)(((uintptr_t)o >> 3) & 1);
        if (head && lane == 0 && total > 0) T[0] = o[0];
        for (int i = head + 2 * lane; i < total; i += 128) {
            if (i + 1 < total) {
                const kb_f64x2 v = *(const kb_f64x2*)(o + i);
                T[agents_tile_at(i, d, ld)] = v[0];
                T[agents_tile_at(i + 1, d, ld)] = v[1];
            } else {
                T[agents_tile_at(i, d, ld)] = o[i];
            }
        }
        const bool live = lane < cnt;
        const double co = live ? in[(size_t)m * d + KB_CH * b + lane] : 0.0;
        bin_wave_sync<false>();
        double* __restrict__ P = K.pool + p;  // (the pool's layout IS the work line)
        const bool embb = d - 1 == 10;
        bool bad = !(__builtin_fabs(co) < __builtin_inf()), nf32 = false;
        double last = 0.0;
        for (int q = 0; q < d; ++q) {
            const double v = live ? T[lane * ld + q] : 0.0;
            bad = bad || !(__builtin_fabs(v) < __builtin_inf());
            P[q * KB_CH + lane] = v;
            if (embb && q < 10) {
                const float vf = (float)v;
                ((float*)(P + KB_ROW_F32 * KB_CH))[q * KB_CH + lane] = vf;
                nf32 = nf32 || (double)vf != v;
            }
            last = v;
        }
        for (int q = embb ? KB_ROW_CO : d; q < KB_ROW_CO; ++q) P[q * KB_CH + lane] = 0.0;
        P[KB_ROW_CO * KB_CH + lane] = co;
        for (int q = KB_ROW_CO + 1; q < KB_VEC_ROWS; ++q)
            if (q != KB_ROW_IDX) P[q * KB_CH + lane] = 0.0;
        int32_t* ix = (int32_t*)(P + KB_ROW_IDX * KB_CH);
        ix[lane] = live ? grid_index(last, D.n_prbs) : 0;
        ix[64 + lane] = 0;
        if (nf32) K.f32bad[jd] = 1;
        if (bad) a.bad[0] = 1;
        bin_wave_sync<false>();  // (the tile is free for the wave's next chunk)
    }
}

// Per dictionary: head and the chain links under the invariant prune_finish_kernel states -- head[a] the largest slot with grid
// index a, links strictly decreasing, -1 for a landmark off the grid -- and the off-grid count.  prune_finish_kernel's walk,
// restated (its code object stays what it was) with the index row staged in LDS 1024 slots at a time: thread a walks the slots
// upwards and links the landmarks of grid index a.
__global__ __launch_bounds__(256) void agents_finish_kernel(AgentArgs a) {
    __shared__ int32_t tile[1024];
    __shared__ int off;
    const KbState& K = a.K;
    const int dict = blockIdx.x, tid = threadIdx.x;
    const uint64_t* sh = shells_of(a.D, K, dict);
    const int m = K.m[dict];
    if (tid == 0) off = 0;
    int prev = -1, cnt = 0;
    for (int j0 = 0; j0 < m; j0 += 1024) {
        __syncthreads();
        const int nt = m - j0 < 1024 ? m - j0 : 1024;
        for (int k = tid; k < nt; k += 256) {
            int32_t* ix = idx_at(K, sh, j0 + k);
            const int v = ix[0];
            tile[k] = v;
            if (v < 0) {
                ix[64] = -1;
                ++cnt;
            }
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k)
            if (tile[k] == tid) {
                idx_at(K, sh, j0 + k)[64] = prev;
                prev = j0 + k;
            }
    }
    K.head[(size_t)dict * KB_HEAD + tid] = prev;
    __syncthreads();
    if (cnt) atomicAdd(&off, cnt);
    __syncthreads();
    if (tid == 0) K.offgrid[dict] = off;
}

}  // namespace kb

// ------------------------------------------------------------------ the file, on the host
struct kb_agents_header {
    char magic[8];  // "KBAGENT1"
    uint64_t bytes;
    uint64_t hash;  // fnv1a of [24, bytes)
    int32_t n_agents, n_slices, n_prbs, capacity;
    int32_t dims[KB_MAX_SLICES];
    double alfa, acc_lo, acc_hi, gamma, eta;
    uint64_t dict_doubles;  // sum of m (d + 1) over all dictionaries
};
static_assert(sizeof(kb_agents_header) == 120, "KBAGENT1 header");
static const char kKbAgentsMagic[8] = {'K', 'B', 'A', 'G', 'E', 'N', 'T', '1'};
#define KB_AGENTS_HASH_FROM 24
#define KB_AGENTS_MAX 16777216  // agents in one file

struct kb_agents_layout {  // byte offsets of the tables, of the dictionaries, and the total
    uint64_t m, f32bad, action, security, margins, adjusted, acc, seeds, tie_ctr, prev, flags, dict, bytes;
};
static kb_agents_layout kb_agents_layout_of(uint64_t n, uint64_t S, uint64_t n_prbs, uint64_t nv, uint64_t dict_doubles) {
    kb_agents_layout L;
    uint64_t at = sizeof(kb_agents_header);
    auto take = [&](uint64_t bytes) {
        const uint64_t here = at;
        at = (at + bytes + 7) & ~7ull;
        return here;
    };
    L.m = take(4 * n * S);
    L.f32bad = take(4 * n * S);
    L.action = take(4 * n * S);
    L.security = take(4 * n * S);
    L.margins = take(4 * n * S);
    L.adjusted = take(4 * n);
    L.acc = take(8 * n * S * n_prbs);
    L.seeds = take(8 * n);
    L.tie_ctr = take(4 * n * S);
    L.prev = take(4 * n * nv);
    L.flags = take(4 * n);
    at = (at + 15) & ~15ull;
    L.dict = at;
    L.bytes = at + 8 * dict_doubles;
    return L;
}
static kb::AgentTables kb_agents_tables(void* blob, const kb_agents_layout& L) {
    char* p = (char*)blob;
    kb::AgentTables F;
    F.m = (int32_t*)(p + L.m);
    F.f32bad = (int32_t*)(p + L.f32bad);
    F.action = (int32_t*)(p + L.action);
    F.security = (int32_t*)(p + L.security);
    F.margins = (int32_t*)(p + L.margins);
    F.adjusted = (int32_t*)(p + L.adjusted);
    F.acc = (double*)(p + L.acc);
    F.seeds = (uint64_t*)(p + L.seeds);
    F.tie_ctr = (uint32_t*)(p + L.tie_ctr);
    F.prev = (float*)(p + L.prev);
    F.flags = (int32_t*)(p + L.flags);
    F.dict = (double*)(p + L.dict);
    return F;
}

static int kb_agents_refuse(const std::string& why) {
    kb_nohandle_err = "kb_agents_info: " + why;
    return RS_EINVAL;
}

// Host only; the one function that parses untrusted bytes.  Everything is checked against `bytes` before it is read: first the
// header alone (magic, its own size field, kb_create's limits, finite parameters, the size its fields imply), then the hash of
// everything behind the hash field, then the sizes (0 <= m <= capacity, their doubles the header's) and the actions.
extern "C" int kb_agents_info(const void* blob, uint64_t bytes, kb_config* cfg, int32_t* m_out) {
    if (!blob) return kb_agents_refuse("no blob");
    if (bytes < sizeof(kb_agents_header)) return kb_agents_refuse("shorter than the header");
    kb_agents_header h;
    memcpy(&h, blob, sizeof h);
    if (memcmp(h.magic, kKbAgentsMagic, 8) != 0) return kb_agents_refuse("not an agent file (magic KBAGENT1)");
    if (h.bytes != bytes) return kb_agents_refuse("the header names " + std::to_string(h.bytes) + " bytes, the blob has " + std::to_string(bytes));
    if (h.n_agents <= 0 || h.n_agents > KB_AGENTS_MAX) return kb_agents_refuse("number of agents out of range");
    if (h.n_slices <= 0 || h.n_slices > KB_MAX_SLICES || h.n_prbs <= 0 || h.n_prbs > KB_NPRB_MAX || h.capacity < 2 ||
        h.capacity > KB_CAPACITY_MAX)
        return kb_agents_refuse("unsupported configuration (<= 8 learners, n_prbs <= 255, 2 <= capacity <= 65536)");
    uint64_t nv = 0;
    for (int s = 0; s < KB_MAX_SLICES; ++s) {
        if (s < h.n_slices ? (h.dims[s] <= 0 || h.dims[s] + 1 > KB_DMAX) : h.dims[s] != 0) return kb_agents_refuse("learner dimension out of range");
        nv += (uint64_t)h.dims[s];
    }
    if (!std::isfinite(h.alfa) || !std::isfinite(h.acc_lo) || !std::isfinite(h.acc_hi) || !std::isfinite(h.gamma) || !std::isfinite(h.eta))
        return kb_agents_refuse("alfa, the accuracy range, gamma or eta is not finite");
    if (h.dict_doubles > bytes / 8) return kb_agents_refuse("the header's fields imply more bytes than the blob has");
    const uint64_t n = (uint64_t)h.n_agents, S = (uint64_t)h.n_slices;
    const kb_agents_layout L = kb_agents_layout_of(n, S, (uint64_t)h.n_prbs, nv, h.dict_doubles);
    if (L.bytes != bytes) return kb_agents_refuse("the header's fields imply " + std::to_string(L.bytes) + " bytes, the blob has " + std::to_string(bytes));
    if (fnv1a((const char*)blob + KB_AGENTS_HASH_FROM, (size_t)(bytes - KB_AGENTS_HASH_FROM)) != h.hash)
        return kb_agents_refuse("the hash does not match the contents");
    const char* p = (const char*)blob;
    uint64_t doubles = 0, pages = 0;
    for (uint64_t i = 0; i < n * S; ++i) {
        int32_t m, act;
        memcpy(&m, p + L.m + 4 * i, 4);
        memcpy(&act, p + L.action + 4 * i, 4);
        if (m < 0 || m > h.capacity) return kb_agents_refuse("a dictionary's size is negative or beyond the capacity");
        if (act < 0 || act > h.n_prbs) return kb_agents_refuse("an action is not one of the candidates 0 .. n_prbs");
        doubles += (uint64_t)m * (uint64_t)(h.dims[i % S] + 2);
        pages += (uint64_t)(m + KB_CH - 1) / KB_CH;
        if (m_out) m_out[i] = m;
    }
    if (doubles != h.dict_doubles) return kb_agents_refuse("the sizes do not add up to the dictionaries' doubles in the header");
    if (cfg) {
        memset(cfg, 0, sizeof *cfg);
        cfg->n_envs = h.n_agents;
        cfg->n_slices = h.n_slices;
        cfg->n_prbs = h.n_prbs;
        cfg->capacity = h.capacity;
        for (int s = 0; s < KB_MAX_SLICES; ++s) cfg->dims[s] = h.dims[s];
        cfg->alfa = h.alfa;
        cfg->acc_lo = h.acc_lo;
        cfg->acc_hi = h.acc_hi;
        cfg->gamma = h.gamma;
        cfg->eta = h.eta;
        cfg->pool_bytes = (int64_t)(8 * (64 + pages * KB_VEC));
    }
    return RS_OK;
}

// ------------------------------------------------------------------ export
// the index on the device, sizes and the two scans on src's own stream (behind everything queued there), the totals on the host
struct kb_agents_plan {
    int32_t* d_index = nullptr;
    uint64_t* d_base = nullptr;  // pbase [ND + 1], fbase [ND + 1], total [2]
    int32_t* d_bad = nullptr;
    void* d_blob = nullptr;
    uint64_t tops[3] = {0, 0, 0};
    hipEvent_t e0 = nullptr, e1 = nullptr;  // around the transposing kernel
    ~kb_agents_plan() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (d_index) (void)hipFree(d_index);
        if (d_base) (void)hipFree(d_base);
        if (d_bad) (void)hipFree(d_bad);
        if (d_blob) (void)hipFree(d_blob);
    }
};

// device time of the transposing kernel of this thread's last kb_export_agents ([0], agents_pack_kernel) and kb_import_agents
// ([1], agents_build_kernel), from a pair of HIP events around the one launch, and the bytes its work plan counts, read plus
// written: pack reads d + 1 whole rows of every page and writes the file's dictionaries, build reads those and writes whole pages
static thread_local double kb_agents_ms[2] = {0.0, 0.0};
static thread_local uint64_t kb_agents_bytes[2] = {0, 0};
extern "C" int kb_agents_kernel_times(double ms[2], uint64_t bytes[2]) {
    if (!ms || !bytes) return RS_EINVAL;
    for (int i = 0; i < 2; ++i) {
        ms[i] = kb_agents_ms[i];
        bytes[i] = kb_agents_bytes[i];
    }
    return RS_OK;
}
static void kb_agents_timed(kb_agents_plan& pl, int which, uint64_t bytes) {  // after the stream was waited for
    float ms = 0.f;
    if (pl.e0 && pl.e1 && hipEventElapsedTime(&ms, pl.e0, pl.e1) == hipSuccess) {
        kb_agents_ms[which] = (double)ms;
        kb_agents_bytes[which] = bytes;
    }
}

static int kb_agents_scan(kb_handle* k, kb_agents_plan& pl, kb::AgentArgs& a, int nd) {
    HIPCHK(k, hipMalloc((void**)&pl.d_base, sizeof(uint64_t) * (2 * ((size_t)nd + 1) + 3)));
    a.n_dict = nd;
    a.pbase = pl.d_base;
    a.fbase = pl.d_base + nd + 1;
    a.total = pl.d_base + 2 * ((size_t)nd + 1);
    HIPCHK(k, hipMemsetAsync(a.total, 0, sizeof(uint64_t) * 3, k->stream));
    hipLaunchKernelGGL(kb::agents_count_kernel, dim3((unsigned)((nd + 255) / 256)), dim3(256), 0, k->stream, a);
    hipLaunchKernelGGL(kb::fork_scan_kernel, dim3(1), dim3(1024), 0, k->stream, a.pbase, nd, a.total);
    hipLaunchKernelGGL(kb::fork_scan_kernel, dim3(1), dim3(1024), 0, k->stream, a.fbase, nd, a.total + 1);
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(pl.tops, a.total, sizeof pl.tops, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    return RS_OK;
}

static int kb_export_plan(kb_handle* src, const int32_t* src_index, int32_t n, kb_agents_plan& pl, kb::AgentArgs& a, kb_agents_layout* L,
                          const char* who) {
    int rc = kb_fork_check(nullptr, src, src_index, n, &src->err, who);
    if (rc != RS_OK) return rc;
    if (n > KB_AGENTS_MAX) {
        src->err = std::string(who) + ": more agents than one file holds";
        return RS_EINVAL;
    }
    HIPCHK(src, hipSetDevice(src->device));
    if (src->side) HIPCHK(src, hipStreamSynchronize(src->side));  // (the test build's side stream: behind its queued work too)
    HIPCHK(src, hipMalloc((void**)&pl.d_index, sizeof(int32_t) * (size_t)n));
    HIPCHK(src, hipMemcpyAsync(pl.d_index, src_index, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, src->stream));
    memset(&a, 0, sizeof a);
    a.D = src->D;
    a.K = src->K;
    a.index = pl.d_index;
    a.pack = 1;
    a.prev = src->d_prev_state;
    a.hits = src->d_hits;
    if ((rc = kb_agents_scan(src, pl, a, n * src->cfg.n_slices)) != RS_OK) return rc;
    *L = kb_agents_layout_of((uint64_t)n, (uint64_t)src->cfg.n_slices, (uint64_t)src->cfg.n_prbs, (uint64_t)src->nv, pl.tops[1] - 64);
    return RS_OK;
}

extern "C" int kb_export_bytes(kb_handle* src, const int32_t* src_index, int32_t n, uint64_t* bytes) {
    if (!src || !src_index || !bytes || n <= 0) return RS_EINVAL;
    kb_agents_plan pl;
    kb::AgentArgs a;
    kb_agents_layout L;
    const int rc = kb_export_plan(src, src_index, n, pl, a, &L, "kb_export_bytes");
    if (rc != RS_OK) return rc;
    *bytes = L.bytes;
    return RS_OK;
}

extern "C" int kb_export_agents(kb_handle* src, const int32_t* src_index, int32_t n, void* blob, uint64_t bytes) {
    if (!src || !src_index || !blob || n <= 0) return RS_EINVAL;
    kb_agents_plan pl;
    kb::AgentArgs a;
    kb_agents_layout L;
    int rc = kb_export_plan(src, src_index, n, pl, a, &L, "kb_export_agents");
    if (rc != RS_OK) return rc;
    if (bytes != L.bytes) {
        src->err = "kb_export_agents: the agents need " + std::to_string(L.bytes) + " bytes (kb_export_bytes), the blob has " + std::to_string(bytes);
        return RS_EINVAL;
    }
    HIPCHK(src, hipMalloc(&pl.d_blob, (size_t)bytes));
    HIPCHK(src, hipMemsetAsync(pl.d_blob, 0, (size_t)L.dict, src->stream));  // (the header's place and the tables' padding: zeros)
    a.F = kb_agents_tables(pl.d_blob, L);
    hipLaunchKernelGGL(kb::agents_tables_kernel, dim3((unsigned)((a.n_dict + 3) / 4)), dim3(256), 0, src->stream, a);
    const uint64_t n_chunks = (pl.tops[0] - 64) / KB_VEC;
    if (n_chunks) {
        const uint64_t grid = (n_chunks + 3) / 4;
        HIPCHK(src, hipEventCreate(&pl.e0));
        HIPCHK(src, hipEventCreate(&pl.e1));
        HIPCHK(src, hipEventRecord(pl.e0, src->stream));
        hipLaunchKernelGGL(kb::agents_pack_kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, src->stream, a);
        HIPCHK(src, hipEventRecord(pl.e1, src->stream));
    }
    HIPCHK(src, hipGetLastError());
    HIPCHK(src, hipMemcpyAsync(blob, pl.d_blob, (size_t)bytes, hipMemcpyDeviceToHost, src->stream));
    HIPCHK(src, hipStreamSynchronize(src->stream));
    kb_agents_timed(pl, 0, 8 * (pl.tops[2] + (pl.tops[1] - 64)));
    kb_agents_header h;
    memset(&h, 0, sizeof h);
    memcpy(h.magic, kKbAgentsMagic, 8);
    h.bytes = bytes;
    h.n_agents = n;
    h.n_slices = src->cfg.n_slices;
    h.n_prbs = src->cfg.n_prbs;
    h.capacity = src->cfg.capacity;
    for (int s = 0; s < src->cfg.n_slices; ++s) h.dims[s] = src->cfg.dims[s];
    h.alfa = src->cfg.alfa;
    h.acc_lo = src->cfg.acc_lo;
    h.acc_hi = src->cfg.acc_hi;
    h.gamma = src->cfg.gamma;
    h.eta = src->cfg.eta;
    h.dict_doubles = pl.tops[1] - 64;
    memcpy(blob, &h, sizeof h);
    h.hash = fnv1a((const char*)blob + KB_AGENTS_HASH_FROM, (size_t)(bytes - KB_AGENTS_HASH_FROM));
    memcpy(blob, &h, sizeof h);
    return RS_OK;
}

// ------------------------------------------------------------------ import
extern "C" int kb_import_agents(const void* blob, uint64_t bytes, int device, kb_handle** out) {
    if (!out) return RS_EINVAL;
    *out = nullptr;
    kb_config c;
    int rc = kb_agents_info(blob, bytes, &c, nullptr);
    if (rc != RS_OK) return rc;
    kb_handle* d = nullptr;
    auto fail = [&](int code, const std::string& why) {
        kb_nohandle_err = "kb_import_agents: " + why;
        kb_destroy(d);
        return code;
    };
    rc = kb_create_impl(&c, device, &d, (unsigned long long)c.pool_bytes / 8);
    if (rc != RS_OK) return fail(rc, "creating the inference-only handle: " + (d ? d->err : std::string()));
    kb_agents_plan pl;
    hipError_t e;
    if ((e = hipMalloc(&pl.d_blob, (size_t)bytes)) != hipSuccess || (e = hipMalloc((void**)&pl.d_bad, sizeof(int32_t))) != hipSuccess ||
        (e = hipMemcpyAsync(pl.d_blob, blob, (size_t)bytes, hipMemcpyHostToDevice, d->stream)) != hipSuccess ||
        (e = hipMemsetAsync(pl.d_bad, 0, sizeof(int32_t), d->stream)) != hipSuccess)
        return fail(RS_EHIP, hipGetErrorString(e));
    kb_agents_header h;
    memcpy(&h, blob, sizeof h);
    const kb_agents_layout L = kb_agents_layout_of((uint64_t)h.n_agents, (uint64_t)h.n_slices, (uint64_t)h.n_prbs, (uint64_t)d->nv, h.dict_doubles);
    kb::AgentArgs a;
    memset(&a, 0, sizeof a);
    a.D = d->D;
    a.K = d->K;
    a.F = kb_agents_tables(pl.d_blob, L);
    a.prev = d->d_prev_state;
    a.hits = d->d_hits;
    a.bad = pl.d_bad;
    if ((rc = kb_agents_scan(d, pl, a, d->n_dict)) != RS_OK) return fail(rc, d->err);
    if (pl.tops[0] != d->D.pool_doubles || pl.tops[1] - 64 != h.dict_doubles)  // (kb_agents_info summed the same sizes)
        return fail(RS_EINVAL, "the sizes on the device do not add up to the file's");
    if ((rc = kb_restart(d)) != RS_OK) return fail(rc, d->err);
    hipLaunchKernelGGL(kb::agents_tables_kernel, dim3((unsigned)((a.n_dict + 3) / 4)), dim3(256), 0, d->stream, a);
    const uint64_t n_chunks = (pl.tops[0] - 64) / KB_VEC;
    if (n_chunks) {
        const uint64_t grid = (n_chunks + 3) / 4;
        if ((e = hipEventCreate(&pl.e0)) != hipSuccess || (e = hipEventCreate(&pl.e1)) != hipSuccess ||
            (e = hipEventRecord(pl.e0, d->stream)) != hipSuccess)
            return fail(RS_EHIP, hipGetErrorString(e));
        hipLaunchKernelGGL(kb::agents_build_kernel, dim3((unsigned)(grid < 16384 ? grid : 16384)), dim3(256), 0, d->stream, a);
        if ((e = hipEventRecord(pl.e1, d->stream)) != hipSuccess) return fail(RS_EHIP, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kb::agents_finish_kernel, dim3((unsigned)a.n_dict), dim3(256), 0, d->stream, a);
    int32_t bad = 0;
    if ((e = hipGetLastError()) != hipSuccess || (e = hipMemcpyAsync(&bad, pl.d_bad, sizeof bad, hipMemcpyDeviceToHost, d->stream)) != hipSuccess ||
        (e = hipStreamSynchronize(d->stream)) != hipSuccess)
        return fail(RS_EHIP, hipGetErrorString(e));
    if (bad) return fail(RS_EINVAL, "a landmark coordinate or a coefficient is not finite");
    kb_agents_timed(pl, 1, 8 * ((pl.tops[1] - 64) + (pl.tops[0] - 64)));
    if (d->h_seen) d->h_seen[0] = d->h_seen[1] = 0;
    d->gemm_fresh = false;
    d->big_par = 0;
    d->is_reset = true;
    *out = d;
    return RS_OK;
}
