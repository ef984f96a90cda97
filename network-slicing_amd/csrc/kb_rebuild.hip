// kb_rebuild.hip -- kb_fork_rebuild: kb_fork for sources that hold no Kinv (kb_deploy, kb_import_agents).  The destination's
// Kinv is rebuilt on the device by replaying the insertions in slot order.
// #included by rs_api.hip after kb_agents.hip: it uses the agent handle, kb_fork.hip's transfer sequence (scan, tables kernel, work
// line, checks) and the forceinline pieces of Projectron.update (kb_kbrl.hip).
//
// THE RULE.  Kinv changes only when a landmark is inserted (a projection touches coefficients), and the insertion of landmark j
// is a function of landmarks 0 .. j alone: the kernel column of l_j against l_0 .. l_{j-1}, d* = Kinv K_f, delta = max(1 -
// K_f . d*, 0) and old + (d_i d_j) / delta with d*_j = -1.  Every one of these sums has one shape whatever kernel forms it
// (kernel_column_full, matvec_tri_tiles / matvec_tri_tiles_lds + combine, wave_dot256_rows, rank1_units), so replaying steps
// j = 1 .. m - 1 over landmarks that were never reordered gives the source's Kinv bit for bit.  Over any other slot order (a
// pruned dictionary, a host-packed one) the same recurrence still yields the landmarks' inverse Gram matrix; a delta below eta
// then only says that the Projectron would not have inserted in this order.
//
// THE REPLAY.  Steps below KB_RB_SMALL run in one launch, a workgroup per dictionary looping j in the kernel
// (rebuild_small_kernel) -- every dictionary's first KB_RB_SMALL steps, so no dictionary is small "all the way" on a lone
// workgroup.  From there on the dictionaries advance together, one step per round, three launches as wide as the chip:
//   rebuild_matvec_kernel   the partial sums of d* of every active dictionary (m > j), tiles laid end to end
//   rebuild_finish_kernel   per dictionary: d*, delta, min_delta, the -1, the error word; then the kernel column of step j + 1
//   rebuild_rank1_kernel    Kinv's rank-1 update, units laid end to end
// All active dictionaries of round j have the same work (the triangle of j landmarks), so with the dictionaries listed by
// decreasing size the round's work line is (first n_act of the list) x (tiles of j): a wave finds its stretch by one division.
// The host knows the sizes from the fork's one wait, so it sizes every launch and counts tiles and units from that plan; there
// is no host wait between rounds.

#include <cfloat>
#include <algorithm>

#define KB_RB_SMALL KB_SMALL_M  // steps below this many landmarks are replayed by rebuild_small_kernel

namespace kb {

struct RebuildArgs {
    KbDev D;               // destination
    KbState K;
    int32_t n_dict;
    int32_t j;             // the round: landmark j is inserted into the dictionary of landmarks 0 .. j - 1
    int32_t n_act;         // dictionaries of the round: the first n_act of `list`
    const int32_t* list;   // dictionaries of more than KB_RB_SMALL landmarks, by decreasing size
    double* delta;         // [n_dict] the round's delta, from rebuild_finish_kernel to rebuild_rank1_kernel
    double* min_delta;     // [n_dict] the smallest delta met
    int32_t* bad;          // [n_dict] 1: a step met a delta that is not finite or not above zero; the dictionary stopped there
    int32_t* nbad;         // [2] how many, the first
};

// what the host reads in the fork's one wait besides the scan's total: the destination dictionaries' sizes
__global__ __launch_bounds__(256) void rebuild_sizes_kernel(XferArgs a, int32_t* m_out) {
    const int jd = blockIdx.x * blockDim.x + threadIdx.x;
    if (jd < a.n_dict) m_out[jd] = a.Ks.m[fork_src_dict(a, jd)];
}

// Shell gather of a destination that stores Kinv from a source whose shells need not: the work line with every shell cut in
// two -- its vector page comes from the source's shell, its Kinv tiles and their partial-sum areas are zeroed.
__global__ __launch_bounds__(256) void rebuild_pages_kernel(XferArgs a) {
    const int lane = threadIdx.x & 63;
    line_walk(a.base, a.n_dict, a.Dd.tri, KbCutPage(), [&](int jd, int b, uint64_t in, uint64_t p, uint64_t seg) {
        const uint64_t so = in < KB_VEC ? src_shell(a, fork_src_dict(a, jd), b, KB_VEC) : 0ull;
        if (so) wave_copy(a.Kd.pool + p, a.Ks.pool + so + in, seg, lane);
        else wave_zero(a.Kd.pool + p, seg, lane);
    });
}

// landmark j of the dictionary -> x[0 .. d - 1] (LDS), for the whole block
__device__ __forceinline__ void rebuild_stage(const KbState& K, const uint64_t* sh, int j, int d, double* x) {
    __syncthreads();
    if ((int)threadIdx.x < d) x[threadIdx.x] = vec_page(K, sh, j >> 6)[threadIdx.x * KB_CH + (j & 63)];
    __syncthreads();
}

// delta of step j from the K_f and d* rows, as finish_update forms it: the float32 product below two landmarks, else
// wave_dot256_rows by the first wave.  Every thread of the block returns it.
__device__ __forceinline__ double rebuild_delta(const KbState& K, const uint64_t* sh, int j, double* red) {
    double dot;
    if (j == 1) {
        const float kf0 = (float)*vec_at(K, sh, KB_ROW_KF, 0);
        const float ds = (float)*vec_at(K, sh, KB_ROW_DS, 0);
        dot = (double)(float)(ds * kf0);
    } else {
        if (threadIdx.x < 64) {
            const double v = wave_dot256_rows(K, sh, KB_ROW_DS, KB_ROW_KF, j);
            if (threadIdx.x == 0) red[0] = v;
        }
        __syncthreads();
        dot = red[0];
        __syncthreads();
    }
    const double delta = 1.0 - dot;  // Kii = k(x, x) = 1
    return delta > 0.0 ? delta : 0.0;
}

__device__ __forceinline__ bool rebuild_delta_ok(double delta) { return delta > 0.0 && delta <= DBL_MAX; }

// thread 0 of the dictionary's block
__device__ __forceinline__ void rebuild_mark_bad(const RebuildArgs& a, int dict) {
    a.bad[dict] = 1;
    atomicAdd(&a.nbad[0], 1);
    atomicMin(&a.nbad[1], dict);
}

// Steps 0 .. min(m, KB_RB_SMALL) - 1 of every dictionary, a workgroup each; for the dictionaries that go on in the rounds,
// the kernel column of their first round.  Also restarts the cache of the last kb_predict (the replay uses its rows).
__global__ __launch_bounds__(256) void rebuild_small_kernel(RebuildArgs a) {
    const KbDev& D = a.D;
    const KbState& K = a.K;
    __shared__ double x[KB_DMAX];
    __shared__ double red[2];
    __shared__ double slabs[4][8 * KB_SLAB_LD];
    for (int dict = blockIdx.x; dict < a.n_dict; dict += gridDim.x) {
        const int m = K.m[dict];
        const int d = D.dims[dict % D.S] + 1;
        const uint64_t* sh = shells_of(D, K, dict);
        if (threadIdx.x == 0) {
            a.min_delta[dict] = 1.0;
            a.bad[dict] = 0;
            K.m_last[dict] = -1;
            K.kf_owner[dict] = -1;
        }
        if (m == 0) continue;  // (block-uniform)
        if (threadIdx.x == 0) kinv_tile_lo(K, sh, 0, 0)[0] = 1.0;
        __syncthreads();
        const int je = m < KB_RB_SMALL ? m : KB_RB_SMALL;
        double mind = 1.0;
        bool bad = false;
        for (int j = 1; j < je; ++j) {
            rebuild_stage(K, sh, j, d, x);
            kernel_column_full(D, K, sh, j, d, x, x[d - 1]);
            if (j == 1) {  // Kinv is the 1-element float32 array [1 / Kii]; K_f is float32 (apply_update)
                if (threadIdx.x == 0) *vec_at(K, sh, KB_ROW_DS, 0) = (double)(1.0f * (float)*vec_at(K, sh, KB_ROW_KF, 0));
                __syncthreads();
            } else {
                // (the heavy kernels' form of the triangle mat-vec -- same bits as matvec_tri_colsum, kb_kbrl.hip -- because inlining
                // matvec_tri_colsum here as well changed update_heavy_kernel's register allocation)
                const int nb = (j + 63) >> 6, nt = nb * (nb + 1) / 2;
                for (int t = threadIdx.x >> 6; t < nt; t += blockDim.x >> 6) matvec_tri_tiles_lds(K, sh, j, t, t + 1, slabs[threadIdx.x >> 6]);
                __syncthreads();
                matvec_tri_combine_wide(K, sh, j);
            }
            const double delta = rebuild_delta(K, sh, j, red);
            mind = (j == 1 || delta < mind) ? delta : mind;
            if (!rebuild_delta_ok(delta)) {
                bad = true;
                break;
            }
            if (threadIdx.x == 0) *vec_at(K, sh, KB_ROW_DS, j) = -1.0;
            __syncthreads();
            rank1_units(K, sh, j, delta, 1, threadIdx.x >> 6, blockDim.x >> 6);
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            a.min_delta[dict] = mind;
            if (bad) rebuild_mark_bad(a, dict);
        }
        if (!bad && m > KB_RB_SMALL) {
            rebuild_stage(K, sh, KB_RB_SMALL, d, x);
            kernel_column_full(D, K, sh, KB_RB_SMALL, d, x, x[d - 1]);
        }
        __syncthreads();
    }
}

// (the rounds' work lines are uniform, n_act x per units: a wave's share by wave_share, kb_kbrl.hip, its slots by division)
__global__ __launch_bounds__(256, KB_MV_OCC) void rebuild_matvec_kernel(RebuildArgs a) {
    __shared__ double slabs[4][8 * KB_SLAB_LD];
    const long long nb = (a.j + 63) >> 6, nt = nb * (nb + 1) / 2;
    long long lo, hi;
    wave_share((long long)a.n_act * nt, &lo, &hi);
    while (lo < hi) {
        const long long slot = lo / nt, t0 = lo - slot * nt;
        const long long t1 = hi - slot * nt < nt ? hi - slot * nt : nt;
        const int dict = a.list[slot];
        if (!a.bad[dict]) matvec_tri_tiles_lds(a.K, shells_of(a.D, a.K, dict), a.j, (int)t0, (int)t1, slabs[threadIdx.x >> 6]);
        lo = slot * nt + t1;
    }
}

__global__ __launch_bounds__(256) void rebuild_finish_kernel(RebuildArgs a) {
    const KbDev& D = a.D;
    const KbState& K = a.K;
    __shared__ double x[KB_DMAX];
    __shared__ double red[2];
    const int dict = a.list[blockIdx.x];
    if (a.bad[dict]) return;
    const int m = K.m[dict], j = a.j;
    const int d = D.dims[dict % D.S] + 1;
    const uint64_t* sh = shells_of(D, K, dict);
    matvec_tri_combine_wide(K, sh, j);
    const double delta = rebuild_delta(K, sh, j, red);
    const bool ok = rebuild_delta_ok(delta);
    if (threadIdx.x == 0) {
        if (delta < a.min_delta[dict]) a.min_delta[dict] = delta;
        a.delta[dict] = delta;
        if (ok) *vec_at(K, sh, KB_ROW_DS, j) = -1.0;
        else rebuild_mark_bad(a, dict);
    }
    if (!ok || j + 1 >= m) return;
    rebuild_stage(K, sh, j + 1, d, x);
    kernel_column_full(D, K, sh, j + 1, d, x, x[d - 1]);
}

__global__ __launch_bounds__(256) void rebuild_rank1_kernel(RebuildArgs a) {
    const long long nb1 = (a.j + 1 + 63) >> 6, nu = nb1 * (nb1 + 1) / 2 * 4;
    long long lo, hi;
    wave_share((long long)a.n_act * nu, &lo, &hi);
    while (lo < hi) {
        const long long slot = lo / nu, u0 = lo - slot * nu;
        const long long u1 = hi - slot * nu < nu ? hi - slot * nu : nu;
        const int dict = a.list[slot];
        if (!a.bad[dict]) rank1_units(a.K, shells_of(a.D, a.K, dict), a.j, a.delta[dict], 1, (int)u0, 1, (int)u1);
        lo = slot * nu + u1;
    }
}

}  // namespace kb

// what kb_fork_rebuild keeps behind its destination, outside the saved regions (created by the first call)
struct kb_rebuild_state {
    int32_t *d_m = nullptr, *d_list = nullptr, *d_bad = nullptr, *d_nbad = nullptr;
    double *d_delta = nullptr, *d_min = nullptr;
    int32_t *h_m = nullptr, *h_list = nullptr, *h_nbad = nullptr;  // pinned
    uint64_t work[4] = {0, 0, 0, 0};
    bool have = false;   // a replay ran: d_min holds its result
    EventSpans spans;    // kernel timing: one pair around the replay
    double last_ms = 0.0;
};

static void kb_rebuild_release(kb_handle* k) {
    kb_rebuild_state* r = k->rebuild;
    if (!r) return;
    void* ds[] = {r->d_m, r->d_list, r->d_bad, r->d_nbad, r->d_delta, r->d_min};
    for (void* d : ds)
        if (d) (void)hipFree(d);
    void* hs[] = {r->h_m, r->h_list, r->h_nbad};
    for (void* h : hs)
        if (h) (void)hipHostFree(h);
    r->spans.release();
    delete r;
    k->rebuild = nullptr;
}

static int kb_rebuild_prepare(kb_handle* k) {
    if (k->rebuild) return RS_OK;
    kb_rebuild_state* r = new kb_rebuild_state();
    k->rebuild = r;  // (kb_destroy frees whatever was allocated)
    const size_t nd = (size_t)k->n_dict;
    HIPCHK(k, hipMalloc((void**)&r->d_m, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&r->d_list, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&r->d_bad, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&r->d_nbad, sizeof(int32_t) * 2));
    HIPCHK(k, hipMalloc((void**)&r->d_delta, sizeof(double) * nd));
    HIPCHK(k, hipMalloc((void**)&r->d_min, sizeof(double) * nd));
    HIPCHK(k, hipHostMalloc((void**)&r->h_m, sizeof(int32_t) * nd, hipHostMallocDefault));
    HIPCHK(k, hipHostMalloc((void**)&r->h_list, sizeof(int32_t) * nd, hipHostMallocDefault));
    HIPCHK(k, hipHostMalloc((void**)&r->h_nbad, sizeof(int32_t) * 2, hipHostMallocDefault));
    return RS_OK;
}

// kb_fork_core's sequence with the shells gathered page by page and Kinv replayed behind them.  Two host waits: the scan's
// total (with the sizes), and the result words.
static int kb_rebuild_core(kb_handle* dst, kb_handle* src, const int32_t* src_index) {
    const char* who = "kb_fork_rebuild";
    int rc;
    if ((rc = kb_xfer_enter(dst, src, src_index, who)) != RS_OK) return rc;
    if ((rc = kb_rebuild_prepare(dst)) != RS_OK) return rc;
    kb_rebuild_state* r = dst->rebuild;
    r->have = false;
    r->last_ms = 0.0;
    for (int q = 0; q < 4; ++q) r->work[q] = 0;
    const int ND = dst->n_dict;
    kb::XferArgs a = kb_xfer_args(dst, src, ND);
    uint64_t top;
    kb_xfer_launch(dst, kb::fork_count_kernel, a, (size_t)ND, 256);
    hipLaunchKernelGGL(kb::rebuild_sizes_kernel, dim3((unsigned)((ND + 255) / 256)), dim3(256), 0, dst->stream, a, r->d_m);
    HIPCHK(dst, hipMemcpyAsync(r->h_m, r->d_m, sizeof(int32_t) * (size_t)ND, hipMemcpyDeviceToHost, dst->stream));
    if ((rc = kb_xfer_scan_wait(dst, a, &top)) != RS_OK) return rc;
    a.empty = top > dst->D.pool_doubles ? 1 : 0;
    kb_xfer_launch(dst, kb::fork_tables_kernel, a, (size_t)ND, 4);
    HIPCHK(dst, hipGetLastError());
    if (a.empty) {
        if ((rc = kb_xfer_leave(dst, src)) != RS_OK) return rc;
        return kb_xfer_overflow(dst, who, top);
    }
    kb_xfer_launch_line(dst, kb::rebuild_pages_kernel, a, top);
    // the plan: the dictionaries that go on in the rounds by decreasing size (ties by index), and what the replay will stream
    int n_big = 0, max_m = 0;
    for (int jd = 0; jd < ND; ++jd) {
        if (r->h_m[jd] > KB_RB_SMALL) r->h_list[n_big++] = jd;
        max_m = std::max(max_m, (int)r->h_m[jd]);
    }
    std::sort(r->h_list, r->h_list + n_big, [&](int32_t p, int32_t q) { return r->h_m[p] != r->h_m[q] ? r->h_m[p] > r->h_m[q] : p < q; });
    {
        std::vector<uint64_t> tiles((size_t)max_m + 1, 0), units((size_t)max_m + 1, 0);  // of steps 1 .. m - 1, by m
        for (int m = 2; m <= max_m; ++m) {
            const int j = m - 1;
            const uint64_t nb = (uint64_t)(j + 63) >> 6, nb1 = (uint64_t)(j + 1 + 63) >> 6;
            tiles[m] = tiles[m - 1] + (j >= 2 ? nb * (nb + 1) / 2 : 0);
            units[m] = units[m - 1] + nb1 * (nb1 + 1) / 2 * 4;
        }
        for (int jd = 0; jd < ND; ++jd) {
            r->work[0] += tiles[(size_t)r->h_m[jd]];
            r->work[1] += units[(size_t)r->h_m[jd]];
            r->work[3] += r->h_m[jd] > 0 ? 1 : 0;
        }
        r->work[2] = max_m > KB_RB_SMALL ? (uint64_t)(max_m - KB_RB_SMALL) : 0;
    }
    if (n_big) HIPCHK(dst, hipMemcpyAsync(r->d_list, r->h_list, sizeof(int32_t) * (size_t)n_big, hipMemcpyHostToDevice, dst->stream));
    r->h_nbad[0] = 0;
    r->h_nbad[1] = 0x7fffffff;
    HIPCHK(dst, hipMemcpyAsync(r->d_nbad, r->h_nbad, sizeof(int32_t) * 2, hipMemcpyHostToDevice, dst->stream));
    kb::RebuildArgs ra;
    memset(&ra, 0, sizeof ra);
    ra.D = dst->D;
    ra.K = dst->K;
    ra.n_dict = ND;
    ra.list = r->d_list;
    ra.delta = r->d_delta;
    ra.min_delta = r->d_min;
    ra.bad = r->d_bad;
    ra.nbad = r->d_nbad;
    r->spans.on = dst->spans.on;
    r->spans.reset();
    hipEvent_t e_end;
    HIPCHK(dst, r->spans.begin(dst->stream, 0, &e_end));
    hipLaunchKernelGGL(kb::rebuild_small_kernel, dim3((unsigned)ND), dim3(256), 0, dst->stream, ra);
    int n_act = n_big;
    for (int j = KB_RB_SMALL; j < max_m; ++j) {
        while (n_act > 0 && r->h_m[r->h_list[n_act - 1]] <= j) --n_act;
        ra.j = j;
        ra.n_act = n_act;
        const long long nb = (j + 63) >> 6, nb1 = (j + 1 + 63) >> 6;
        const long long tiles = (long long)n_act * (nb * (nb + 1) / 2), units = (long long)n_act * (nb1 * (nb1 + 1) / 2) * 4;
        const long long g_mv = std::min<long long>((tiles + 3) / 4, dst->mv_grid), g_r1 = std::min<long long>((units + 3) / 4, dst->r1_grid);
        hipLaunchKernelGGL(kb::rebuild_matvec_kernel, dim3((unsigned)g_mv), dim3(256), 0, dst->stream, ra);
        hipLaunchKernelGGL(kb::rebuild_finish_kernel, dim3((unsigned)n_act), dim3(256), 0, dst->stream, ra);
        hipLaunchKernelGGL(kb::rebuild_rank1_kernel, dim3((unsigned)g_r1), dim3(256), 0, dst->stream, ra);
    }
    if (e_end) HIPCHK(dst, hipEventRecord(e_end, dst->stream));
    HIPCHK(dst, hipGetLastError());
    HIPCHK(dst, hipMemcpyAsync(r->h_nbad, r->d_nbad, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, dst->stream));
    HIPCHK(dst, hipStreamSynchronize(dst->stream));
    r->have = true;
    const int n_bad = r->h_nbad[0], first = r->h_nbad[1];
    if (n_bad) {  // as after an overflow: the control state of the sources and empty dictionaries
        a.empty = 1;
        kb_xfer_launch(dst, kb::fork_tables_kernel, a, (size_t)ND, 4);
        HIPCHK(dst, hipGetLastError());
    }
    if ((rc = kb_xfer_leave(dst, src)) != RS_OK) return rc;
    if (n_bad) {
        const int S = dst->cfg.n_slices;
        dst->err = std::string(who) + ": the replay of " + std::to_string(n_bad) + " dictionaries met a delta that is not finite or not above zero, first " +
                   "agent " + std::to_string(first / S) + " slice " + std::to_string(first % S) +
                   " (a repeated landmark?); the destination was left reset with empty dictionaries";
        return RS_ESTATE;
    }
    return RS_OK;
}

extern "C" int kb_fork_rebuild(kb_handle* dst, kb_handle* src, const int32_t* src_index) {
    if (!dst || !src || !src_index) return RS_EINVAL;
    if (dst == src) {
        dst->err = "kb_fork_rebuild: source and destination must be different handles";
        return RS_EINVAL;
    }
    int rc = kb_fork_check(dst, src, src_index, dst->cfg.n_envs, &dst->err, "kb_fork_rebuild");
    if (rc != RS_OK) return rc;
    if (dst->frozen) {
        dst->err = "kb_fork_rebuild: the destination is an inference-only handle (kb_deploy): it has no room for Kinv; create a learning handle (kb_create)";
        return RS_ESTATE;
    }
    return kb_rebuild_core(dst, src, src_index);
}

extern "C" int kb_get_rebuild(kb_handle* k, double* min_delta, uint64_t work[4]) {
    if (!k || !min_delta || !work) return RS_EINVAL;
    kb_rebuild_state* r = k->rebuild;
    if (!r || !r->have) {
        k->err = "kb_get_rebuild: no kb_fork_rebuild into this handle has replayed yet";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipMemcpyAsync(min_delta, r->d_min, sizeof(double) * (size_t)k->n_dict, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    for (int q = 0; q < 4; ++q) work[q] = r->work[q];
    return RS_OK;
}

extern "C" int kb_rebuild_time_ms(kb_handle* k, double* ms) {
    if (!k || !ms) return RS_EINVAL;
    *ms = 0.0;
    kb_rebuild_state* r = k->rebuild;
    if (!r) return RS_OK;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    HIPCHK(k, r->spans.drain([&](int, double t) { r->last_ms = t; }));
    *ms = r->last_ms;
    return RS_OK;
}
