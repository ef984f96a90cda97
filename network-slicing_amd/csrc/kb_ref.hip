// kb_ref.hip -- deployment by reference (kb_deploy_ref): the replicas of an agent share ONE read-only copy of its dictionaries.
// #included by rs_api.hip after kb_prune.hip: it uses the agent handle, the fork (kb_fork.hip) and the scoring routines of
// kb_kbrl.hip, and changes none of their kernels.
//
// A by-reference handle owns a STORE -- an ordinary inference-only handle (kb_deploy) of the DISTINCT agents its replicas name --
// and, per replica, what kb_deploy copies per replica: control state, tie-break stream, previous observation, flag word.  A
// per-task table maps (replica, slice) to its dictionary in the store.
//
// THE KERNEL WRITES NOTHING INTO A DICTIONARY'S PAGES.  The scoring kernels of kb_kbrl.hip leave D0 and E of "the state being
// processed" in the dictionary's own rows (KB_ROW_D0, KB_ROW_E), so a dictionary serves one state at a time.  select_ref_kernel
// keeps D0 / E of every (replica, landmark) in registers, the landmarks that take the direct evaluation in the replica's own list
// (K.dlist of the by-reference handle), and where add_direct_terms would read the rows back (more than KB_DLIST listed landmarks)
// it forms D0 / E again from the coordinates by the same operations -- the same bits.  That is what makes any number of
// workgroups on one dictionary at once safe, and what lets the store's pages stay byte for byte what kb_deploy wrote.
//
// Work unit: a GROUP -- one dictionary and up to sixteen of the tasks that reference it, the sixteen columns of one
// v_mfma_f64_16x16x4 product (a column's bits do not depend on what the other fifteen hold: select_gemm_kernel puts sixteen
// learners there, this kernel sixteen states of one learner).  Wave w of the workgroup's four bins the landmarks for replicas
// 4 w .. 4 w + 3: a chunk's rows are loaded ONCE into registers and used for the wave's four states, every replica's W[a] summed
// exactly as bin_pass sums it (increasing j within a segment of KB_BIN_SEG chunks, one ds_add_f64 per chunk; the segments' sums in
// order from zero), straight into the W^T operand of the product in LDS -- no K.Wg round trip.  Then the product
// (toeplitz_product: select_gemm_kernel's loop), the direct terms, the row of F, the tie scan and the action per replica
// (select_commit), all as select_gemm_kernel does them: every replica's F, flags, action, margin, draws and counters are bit for
// bit what the copy-deployed handle computes for a private copy of the dictionary and the same state.

#include <algorithm>

namespace kb {

#define KB_REF_GROUP (2 + KB_SEL_WAVES)  // int32 per group: dictionary (of the store), tasks in the group, their ids

struct RefArgs {
    KbDev D;             // the by-reference handle
    KbState K;           // its per-task arrays: control state, tie-break stream, F / fstate / fver / fdirect / dlist, statistics
    KbState Ks;          // the store: m, shell, pool, f32bad, ver of the distinct dictionaries -- READ ONLY
    const float* state;  // [n_envs][nv]
    const int32_t* group;  // [gridDim.x][KB_REF_GROUP]
};

struct RefLds {
    double G2[512];
    double Wt[256 * KB_WT_LD];  // W^T[a][replica]
    union {
        double Wseg[KB_SEL_WAVES][256];  // the segment in progress of a dictionary of more than KB_BIN_SEG chunks, per replica
        double Fs[KB_SEL_WAVES][256];    // F[replica][candidate], once the binning is over
    };
    double x[KB_SEL_WAVES][KB_DMAX];
    int task[KB_SEL_WAVES], res[KB_SEL_WAVES];
};

// select_gemm_kernel's product loop and its scan of a learner's row, statement for statement: A CHANGE TO EITHER IS MADE IN BOTH
// PLACES (kb_kbrl.hip points here).  They are not shared with that kernel as functions: with them moved out of its body it kept
// its VGPR count, scratch size and occupancy, but its instruction stream changed (other register assignments around the
// accumulators, in a kernel whose MFMA loop has been brittle before), and the hot kernel of the learning path stays the code
// that was measured.  The copy-twin tests (tests/test_gpu_deploy_ref.py) hold the two to the same bits.
// F = T W^T for sixteen columns of W^T (LDS, KB_WT_LD doubles between its rows): wave wv's candidate tiles wv, wv + 4, wv + 8,
// wv + 12 (16 candidates each), ONE chain of v_mfma_f64_16x16x4 over a = 0 .. KA - 1 per tile.  A column's bits depend on that
// column alone: sixteen learners there, sixteen states against one dictionary here.
__device__ __forceinline__ void toeplitz_product(const double* Wt, const double* G2, int wv, int lane, int KA, kb_f64x4 (&acc)[4]) {
    const int li = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (kb_f64x4){0.0, 0.0, 0.0, 0.0};
    const double* Wb = Wt + kq * KB_WT_LD + li;      // B operand: W^T[a0 + kq][learner li]
    const double* Ga = G2 + 256 + kq - (16 * wv + li);  // A operand of tile t: T[16 (w + 4 t) + li][a0 + kq] = G2[256 + a - c]
    // (all four tiles unconditionally -- a tile past the last candidate costs its MFMAs and is never stored; a wave-uniform
    // "if (tile < nt)" around each MFMA made the compiler park the accumulators in VGPRs and move them through the same
    // eight AGPRs around every instruction: 340 cycles per MFMA instead of 64)
    for (int a0 = 0; a0 < KA; a0 += 4) {
        const double b = Wb[a0 * KB_WT_LD];
        double ta[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) ta[t] = Ga[a0 - 64 * t];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ta[t], b, acc[t], 0, 0, 0);
    }
}

// the row of F of one learner, by ONE wave: the first accepted candidate in order, exact ties drawing (kbrl_control.py:54-61,
// kernel.py:26-27), the action with its security margin, the two statistics counters
__device__ __forceinline__ void select_commit(const KbDev& D, const KbState& K, int task, int env, int s, int m, int offset,
                                              const double (&f)[4]) {
    const int n = D.n_prbs, lane = threadIdx.x & 63;
    int found = -1;
    uint64_t n_scored = 0;
    if (m > 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (64 * g <= n && found < 0) {
                const int c = 64 * g + lane;
                const int c1 = 64 * g + 63 < n ? 64 * g + 63 : n;
                n_scored += (uint64_t)(c1 - 64 * g + 1);
                unsigned long long cand = __ballot(c <= n && f[g] >= 0.0);  // positive, or a tie to be drawn
                while (cand) {  // walk the (rare) exact ties in order; each consumes one draw (kernel.py:26-27)
                    const int ll = __builtin_ctzll(cand);
                    const double fl = readlane_f64(f[g], ll);
                    if (fl > 0.0) { found = 64 * g + ll; break; }
                    int dr = 0;
                    if (lane == 0) dr = tie_draw(K, task, env, s);
                    dr = __builtin_amdgcn_readfirstlane(dr);
                    if (dr == 1) { found = 64 * g + ll; break; }
                    cand &= cand - 1;
                }
            }
        }
    }
    if (lane == 0) {
        const uint64_t n_pred = found >= 0 ? (uint64_t)found + 1 : (uint64_t)n + 1;
        int act, margin = 0;
        if (found >= 0) {
            int a = n < found + offset ? n : found + offset;
            margin = a - found;
            act = a;
        } else {
            act = n;
        }
        K.action[env * D.S + s] = act;
        K.margins[env * D.S + s] = margin;
        unsigned long long* st = (unsigned long long*)(K.stats + (size_t)task * 4);
        atomicAdd(&st[0], (unsigned long long)n_pred);  // (no return value: nothing waits for it)
        atomicAdd(&st[3], (unsigned long long)(n_scored * (uint64_t)m));
    }
}

// bin_one_chunk (kb_kbrl.hip: a change to its conditions or its listing is made here too) for a dictionary that is not this
// state's to write: D0 / E stay in registers, W[a] (`stride` doubles between its
// entries) takes coeff_j E_j with one ds_add_f64 for the chunk, the landmarks that take the direct evaluation are listed from
// position ndir on -- the same conditions, the same order
__device__ __forceinline__ void ref_bin_chunk(const KbDev& D, const ChunkRows<2>& R, const double* P, int lane, int cnt, int d,
                                              const double* x, double* Wacc, int stride, double* dlist, int& flags, int& ndir) {
    const double d0 = chunk_d0(R, P, lane, d, x);
    const double E = rs_exp_nonpos(-D.gamma * d0);
    const bool offg = lane < cnt && R.a < 0;
    const bool direct = offg || (lane < cnt && !(E >= KB_E_TINY) && E > 0.0);
    const unsigned long long dmask = __ballot(direct);
    if (dmask) {
        flags |= 1 | (__ballot(offg) != 0ull ? 2 : 0);
        const int pos = ndir + __builtin_popcountll(dmask & ((1ull << lane) - 1ull));
        if (direct && pos < KB_DLIST) {
            dlist[3 * pos] = R.co;
            dlist[3 * pos + 1] = P[(d - 1) * KB_CH + lane];
            dlist[3 * pos + 2] = d0;
        }
        ndir += __builtin_popcountll(dmask);
    }
    const double w = R.co * E;
    if (lane < cnt && !direct && R.a >= 0 && w != 0.0) unsafeAtomicAdd(Wacc + R.a * stride, w);  // ds_add_f64
}

__global__ __launch_bounds__(256) void select_ref_kernel(RefArgs A) {
    extern __shared__ __align__(16) unsigned char ref_lds_raw[];
    RefLds& sm = *reinterpret_cast<RefLds*>(ref_lds_raw);
    const KbDev& D = A.D;
    const KbState& K = A.K;
    const KbState& Ks = A.Ks;
    const int n = D.n_prbs;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int32_t* G = A.group + (size_t)blockIdx.x * KB_REF_GROUP;
    const int dict = G[0], cnt = G[1];
    const int s = dict % D.S, d = D.dims[s] + 1;
    const uint64_t* sh = shells_of(D, Ks, dict);
    const uint64_t shv = shell_vector(D, sh);
    const int m = Ks.m[dict];
    const bool f32 = KB_F32_ROWS && d - 1 == 10 && Ks.f32bad[dict] == 0;
    if (threadIdx.x < KB_SEL_WAVES) {
        sm.task[threadIdx.x] = (int)threadIdx.x < cnt ? G[2 + threadIdx.x] : -1;
        sm.res[threadIdx.x] = 0;
    }
    for (int k = threadIdx.x; k < 512; k += blockDim.x) sm.G2[k] = K.gtab[k < 256 ? 256 - k : k - 256];
    for (int i = threadIdx.x; i < 256 * KB_WT_LD; i += blockDim.x) sm.Wt[i] = 0.0;  // (a column without a replica stays zero)
    {
        const int r = threadIdx.x >> 4, q = threadIdx.x & 15;
        const int t = r < cnt ? G[2 + r] : -1;
        sm.x[r][q] = t >= 0 && q < d - 1 ? (double)A.state[(size_t)(t / D.S) * D.nv + D.off[s] + q] : 0.0;
    }
    __syncthreads();
    // ---- W^T: wave w bins the landmarks for replicas 4 w .. 4 w + 3, a chunk's rows in registers for all of them
    const int r0 = 4 * wv;
    const int nrep = cnt - r0 < 4 ? cnt - r0 : 4;
    if (m >= 2 && nrep > 0) {
        const int nch = (m + 63) >> 6;
        const bool segd = nch > KB_BIN_SEG;  // (one segment: summed in place, as bin_pass does)
        int flags[4] = {0, 0, 0, 0}, ndir[4] = {0, 0, 0, 0};
        for (int b0 = 0; b0 < nch; b0 += KB_BIN_SEG) {
            const int b1 = b0 + KB_BIN_SEG < nch ? b0 + KB_BIN_SEG : nch;
            if (segd) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nrep) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) sm.Wseg[r0 + q][lane + 64 * k] = 0.0;
                    }
                bin_wave_sync<false>();
            }
            ChunkRows<2> R, Rn;
            load_chunk<2>(page_of(Ks, sh, shv, b0), lane, d, Rn, f32);
            for (int b = b0; b < b1; ++b) {
                const double* P = page_of(Ks, sh, shv, b);
                R = Rn;
                if (b + 1 < b1) load_chunk<2>(page_of(Ks, sh, shv, b + 1), lane, d, Rn, f32);
                const int c = m - 64 * b < 64 ? m - 64 * b : 64;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nrep)  // (wave-uniform)
                        ref_bin_chunk(D, R, P, lane, c, d, sm.x[r0 + q], segd ? sm.Wseg[r0 + q] : sm.Wt + r0 + q, segd ? 1 : KB_WT_LD,
                                      K.dlist + (size_t)sm.task[r0 + q] * (KB_DLIST * 3), flags[q], ndir[q]);
            }
            if (segd) {
                bin_wave_sync<false>();  // (the LDS executes a wave's instructions in order)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nrep) {
#pragma unroll
                        for (int k = 0; k < 4; ++k) sm.Wt[(lane + 64 * k) * KB_WT_LD + r0 + q] += sm.Wseg[r0 + q][lane + 64 * k];
                    }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nrep && lane == 0) {
                const int r = flags[q] | (ndir[q] << 8);
                sm.res[r0 + q] = r;
                K.fdirect[sm.task[r0 + q]] = r;
            }
    } else if (m < 2 && nrep > 0 && lane < nrep) {
        K.fdirect[sm.task[r0 + lane]] = 0;
    }
    __syncthreads();
    // ---- F = T W^T: wave w owns the candidate tiles w, w + 4, w + 8, w + 12 of all sixteen replicas
    if (m >= 2) {  // (uniform over the workgroup: one dictionary)
        const int nt = n / 16 + 1, KA = (n + 4) & ~3;
        const int li = lane & 15, kq = lane >> 4;
        kb_f64x4 acc[4];
        toeplitz_product(sm.Wt, sm.G2, wv, lane, KA, acc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (wv + 4 * t < nt) {
#pragma unroll
                for (int v = 0; v < 4; ++v) sm.Fs[li][16 * (wv + 4 * t) + kq + 4 * v] = acc[t][v];
            }
        }
    }
    __syncthreads();
    // ---- per replica: the row of F, the first accepted candidate; wave w takes replicas w, w + 4, ...
    for (int l = wv; l < cnt; l += 4) {
        const int task = sm.task[l];
        const int env = task / D.S;
        const int offset = K.security[env * D.S + s];
        double f[4];
        if (m >= 2) {
            // (past n_prbs nobody looks: zeros there, not what the area held as Wseg where no tile stored anything)
#pragma unroll
            for (int g = 0; g < 4; ++g) f[g] = 64 * g + lane <= n ? sm.Fs[l][64 * g + lane] : 0.0;
            const int direct = sm.res[l];
            if (direct)
                add_direct_terms<4, true>(D, Ks, sh, m, d, 0, n / 64 + 1, direct, K.dlist + (size_t)task * (KB_DLIST * 3), f, sm.x[l], f32);
        } else if (m == 1) {
            score_single<4, 2>(D, Ks, sh, d, sm.x[l], 0, f);
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) f[g] = 0.0;
        }
        {
            double* F = K.F + (size_t)task * 256;
#pragma unroll
            for (int g = 0; g < 4; ++g) F[64 * g + lane] = f[g];
            if (lane < d - 1) K.fstate[(size_t)task * 16 + lane] = A.state[(size_t)env * D.nv + D.off[s] + lane];
            if (lane == 0) K.fver[task] = Ks.ver[dict];
        }
        select_commit(D, K, task, env, s, m, offset, f);
    }
}

// What is private to a replica, from its source agent: the per-agent and per-learner words of kb_fork.hip's gather, without a dictionary
struct RefGatherArgs {
    KbDev Dd;
    KbState Kd, Ks;
    const int32_t* index;  // [Dd.n_envs] source agent of every replica
    const float* prev_s;
    float* prev_d;
    int32_t* hits_d;
};
__global__ __launch_bounds__(256) void ref_gather_kernel(RefGatherArgs a) {
    const KbDev& D = a.Dd;
    const int lane = threadIdx.x & 63;
    const int jd = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (jd >= D.n_envs * D.S) return;
    const int j = jd / D.S, s = jd - j * D.S;
    const int r = a.index[j], sd = r * D.S + s;
    for (int c = lane; c < D.n_prbs; c += 64) a.Kd.acc[(size_t)jd * D.n_prbs + c] = a.Ks.acc[(size_t)sd * D.n_prbs + c];
    if (lane == 0) {
        gather_task_words(a.Kd, a.Ks, a.hits_d, jd, sd);
        a.Kd.m[jd] = 0;  // (the handle's own tables hold no dictionary: the map leads to the store)
        a.Kd.kf_owner[jd] = -1;
    }
    if (s == 0) gather_agent_words(D, a.Kd, a.Ks, a.prev_d, a.prev_s, j, r, lane);
    if (jd == 0 && lane == 0) a.Kd.pool_top[0] = 64ull;
}

}  // namespace kb

// what a by-reference handle keeps beside its per-replica state
struct kb_ref_state {
    kb_handle* store = nullptr;         // inference-only handle of the distinct agents: the dictionaries
    std::vector<int32_t> dict_of_task;  // [T] dictionary of the store behind (replica, slice)
    int32_t* d_group = nullptr;         // [n_groups][KB_REF_GROUP]
    int32_t* d_index = nullptr;         // [n_envs] source agent of every replica (the gather's argument)
    int n_groups = 0;
};

static void kb_ref_release(kb_handle* k) {
    kb_ref_state* r = k->ref;
    if (!r) return;
    if (r->d_group) (void)hipFree(r->d_group);
    if (r->d_index) (void)hipFree(r->d_index);
    if (r->store) kb_destroy(r->store);
    delete r;
    k->ref = nullptr;
}
static kb_handle* kb_ref_store(kb_handle* k) { return k->ref->store; }
static int kb_ref_dict(kb_handle* k, size_t task) { return k->ref->dict_of_task[task]; }

// the scoring of launch_select for a by-reference handle: one fused kernel, a workgroup per group
static int kb_ref_select(kb_handle* k, const float* d_state) {
    kb_ref_state* r = k->ref;
    kb::RefArgs a;
    a.D = k->D;
    a.K = k->K;
    a.Ks = r->store->K;
    a.state = d_state;
    a.group = r->d_group;
    hipLaunchKernelGGL(kb::select_ref_kernel, dim3((unsigned)r->n_groups), dim3(256), sizeof(kb::RefLds), k->stream, a);
    return RS_OK;
}

extern "C" int kb_deploy_ref(kb_handle* src, const int32_t* src_index, int32_t n, kb_handle** out) {
    if (!src || !src_index || !out || n <= 0) return RS_EINVAL;
    *out = nullptr;
    int rc = kb_fork_check(nullptr, src, src_index, n, &src->err, "kb_deploy_ref");
    if (rc != RS_OK) return rc;
    const int S = src->cfg.n_slices;
    // the distinct agents, in increasing order: the store's replicas
    std::vector<int32_t> uniq(src_index, src_index + n);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int U = (int)uniq.size();
    std::vector<int32_t> slot((size_t)src->cfg.n_envs, -1);
    for (int u = 0; u < U; ++u) slot[(size_t)uniq[u]] = u;
    kb_handle* store = nullptr;
    rc = kb_deploy(src, uniq.data(), U, &store);  // (ordered after src's queued work, src's later work after its gather)
    if (rc != RS_OK) return rc;
    std::vector<int32_t> m((size_t)U * S);
    hipError_t e = hipMemcpyAsync(m.data(), store->K.m, sizeof(int32_t) * m.size(), hipMemcpyDeviceToHost, store->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(store->stream);  // (the store is complete from here on: nothing ever writes it again)
    if (e != hipSuccess) {
        src->err = std::string("kb_deploy_ref: reading the store's sizes: ") + hipGetErrorString(e);
        kb_destroy(store);
        return RS_EHIP;
    }
    kb_config c = src->cfg;
    c.n_envs = n;
    c.pool_bytes = 64 * 8;
    kb_handle* d = nullptr;
    rc = kb_create_impl(&c, src->device, &d, 64);  // (its own pool is the 64-double preamble: the dictionaries are the store's)
    if (rc != RS_OK) {
        src->err = std::string("kb_deploy_ref: creating the by-reference handle: ") + (d ? d->err : "");
        kb_destroy(d);
        kb_destroy(store);
        return rc;
    }
    kb_ref_state* r = new kb_ref_state();
    d->ref = r;
    r->store = store;
    auto fail = [&](int code, const std::string& why) {
        src->err = "kb_deploy_ref: " + why;
        kb_destroy(d);
        return code;
    };
    // the map, and the group table: per dictionary its tasks in increasing id, cut into groups of sixteen (the last one ragged);
    // the dictionaries with the most landmarks first -- their workgroups are the long ones
    const size_t T = (size_t)n * S;
    r->dict_of_task.resize(T);
    std::vector<std::vector<int32_t>> tasks((size_t)U * S);
    for (int j = 0; j < n; ++j)
        for (int s = 0; s < S; ++s) {
            const int dict = slot[(size_t)src_index[j]] * S + s;
            r->dict_of_task[(size_t)j * S + s] = dict;
            tasks[(size_t)dict].push_back(j * S + s);
        }
    std::vector<int32_t> order((size_t)U * S);
    for (size_t i = 0; i < order.size(); ++i) order[i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t p, int32_t q) { return m[(size_t)p] > m[(size_t)q]; });
    std::vector<int32_t> groups;
    for (int32_t dict : order) {
        const std::vector<int32_t>& t = tasks[(size_t)dict];
        for (size_t i0 = 0; i0 < t.size(); i0 += KB_SEL_WAVES) {
            const size_t cnt = t.size() - i0 < KB_SEL_WAVES ? t.size() - i0 : KB_SEL_WAVES;
            groups.push_back(dict);
            groups.push_back((int32_t)cnt);
            for (size_t i = 0; i < KB_SEL_WAVES; ++i) groups.push_back(i < cnt ? t[i0 + i] : -1);
        }
    }
    r->n_groups = (int)(groups.size() / KB_REF_GROUP);
    if ((e = hipSetDevice(src->device)) != hipSuccess || (e = hipMalloc((void**)&r->d_group, sizeof(int32_t) * groups.size())) != hipSuccess ||
        (e = hipMalloc((void**)&r->d_index, sizeof(int32_t) * (size_t)n)) != hipSuccess ||
        (e = hipMemcpy(r->d_group, groups.data(), sizeof(int32_t) * groups.size(), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(r->d_index, src_index, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipFuncSetAttribute((const void*)kb::select_ref_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(kb::RefLds))) !=
            hipSuccess)
        return fail(RS_EHIP, hipGetErrorString(e));
    // the per-replica state, on the new handle's stream behind src's queued work; src's later work behind the gather
    if ((rc = stream_after(d, &d->ev_fork_in, src->stream, d->stream)) != RS_OK) return fail(rc, d->err);
    kb::RefGatherArgs a;
    memset(&a, 0, sizeof a);
    a.Dd = d->D;
    a.Kd = d->K;
    a.Ks = src->K;
    a.index = r->d_index;
    a.prev_s = src->d_prev_state;
    a.prev_d = d->d_prev_state;
    a.hits_d = d->d_hits;
    hipLaunchKernelGGL(kb::ref_gather_kernel, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, d->stream, a);
    if ((e = hipGetLastError()) != hipSuccess) return fail(RS_EHIP, hipGetErrorString(e));
    if ((rc = stream_after(d, &d->ev_fork_out, d->stream, src->stream)) != RS_OK) return fail(rc, d->err);
    d->is_reset = true;
    *out = d;
    return RS_OK;
}
