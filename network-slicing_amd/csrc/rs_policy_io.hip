// rs_policy_io.hip -- the device-resident policy interface: rs_step_device and what goes with it (rs_get_device_view,
// rs_stream_join, rs_set_action_table, rs_report_*, rs_device_copy).
// #included by rs_api.hip after the handle and the step path: it uses both and changes neither.
//
// A policy that lives on the same GPU (a torch module, a hand-written kernel) hands its actions over as a device pointer and
// reads the observations in place.  One step is   front kernel -> launch_step -> back kernel   on the handle's stream, ordered
// against the caller's stream by two events; the host waits for nothing and nothing crosses PCIe.
//   front: decode the caller's rows (PRBs as they are / ReportWrapper's simplex / a row of the action table), validate them
//          as rs_step does on the host, write the handle's action buffer and the row sums, count refused rows;
//   back:  obs_norm = clip(obs, -0.5, 1.5) - 0.5, the violations per replica, one column of the report histories.
// None of the buffers below is a region of the saved state (h->regions) or known to rs_fork.

namespace rs {

struct FrontArgs {
    const RsDev* D;
    int32_t kind;
    const void* in;           // [n_envs][n_act] int32 / [n_envs][n_act + 1] float / [n_envs] int64
    const int32_t* table;     // [n_table][n_act]
    int32_t n_table;
    int32_t* actions;         // [n_envs][n_act]: the buffer the step kernels read
    int32_t* resources;       // [n_envs] row sums of what was written
    unsigned long long* rejected;
    int32_t* cursor;          // report histories: steps begun since rs_reset / rs_report_begin (at most steps + 1)
    int32_t hist_steps;
};

// One lane per replica row (at most 9 entries).
// The simplex rule is ranslice.report.simplex_to_prbs on a C-contiguous float32 array, operation for operation in float64:
// a_i = |x_i| widened exactly, t = sum a_i in numpy's order for a contiguous axis (pairwise_sum of numpy's add loop: below 8
// entries left to right from 0.0; from 8 entries on eight accumulators r_k = a_k combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the remaining entries added left to right), t = 1 when the sum is 0, PRBs_i = floor((n_prbs * a_i) / t).
// Built with -ffp-contract=off; the f64 divide is the IEEE one.
__global__ __launch_bounds__(256) void policy_front_kernel(FrontArgs a) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.D->n_envs, S = a.D->n_act, n_prbs = a.D->n_prbs;
    if (r == 0 && a.cursor && *a.cursor <= a.hist_steps) *a.cursor += 1;  // (no lane of this kernel reads it)
    if (r >= N) return;
    int32_t row[8];
    bool ok = true;
    if (a.kind == RS_ACT_PRBS) {
        const int32_t* in = (const int32_t*)a.in + (size_t)r * S;
        for (int s = 0; s < S; ++s) row[s] = in[s];
    } else if (a.kind == RS_ACT_SHARES) {
        const float* in = (const float*)a.in + (size_t)r * (S + 1);
        const int W = S + 1;
        double v[9];
        for (int s = 0; s < W; ++s) v[s] = fabs((double)in[s]);
        double t;
        if (W < 8) {
            t = 0.0;
            for (int s = 0; s < W; ++s) t = t + v[s];
        } else {
            t = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
            for (int s = 8; s < W; ++s) t = t + v[s];
        }
        if (t == 0.0) t = 1.0;
        for (int s = 0; s < S; ++s) {
            const double q = floor(((double)n_prbs * v[s]) / t);
            // (NaN and infinite shares have no integer image: the row is refused)
            if (q >= 0.0 && q <= 2147483647.0) row[s] = (int32_t)q;
            else {
                row[s] = 0;
                ok = false;
            }
        }
    } else {
        const int64_t idx = ((const int64_t*)a.in)[r];
        ok = idx >= 0 && idx < (int64_t)a.n_table;
        const int32_t* in = a.table + (size_t)(ok ? idx : 0) * S;
        for (int s = 0; s < S; ++s) row[s] = ok ? in[s] : 0;
    }
    long long tot = 0;
    for (int s = 0; s < S; ++s) {
        ok = ok && row[s] >= 0;
        tot += row[s];
    }
    ok = ok && tot <= (long long)n_prbs;
    if (!ok) atomicAdd(a.rejected, 1ull);
    int32_t* out = a.actions + (size_t)r * S;
    for (int s = 0; s < S; ++s) out[s] = ok ? row[s] : 0;
    a.resources[r] = ok ? (int32_t)tot : 0;
}

struct BackArgs {
    const RsDev* D;
    const float* obs;         // [n_envs][n_vars]
    float* obs_norm;
    const int32_t* viol;      // [n_envs][n_act]
    const double* reward;
    const int32_t* resources;
    int32_t* total_viol;      // [n_envs]
    const int32_t* cursor;
    int32_t hist_steps;
    int16_t* h_viol;          // [n_envs][hist_steps]
    double* h_reward;
    int16_t* h_res;
};

__device__ __forceinline__ float policy_norm(float x) {  // np.clip(x, -0.5, 1.5) - 0.5 in float32 (a NaN stays one)
    const float c = x < -0.5f ? -0.5f : (x > 1.5f ? 1.5f : x);
    return c - 0.5f;
}

__global__ __launch_bounds__(256) void policy_back_kernel(BackArgs a) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nth = (size_t)gridDim.x * blockDim.x;
    const int N = a.D->n_envs, S = a.D->n_act;
    const size_t n = (size_t)N * a.D->n_vars, n4 = n / 4;
    const float4* __restrict__ src = (const float4*)a.obs;
    float4* __restrict__ dst = (float4*)a.obs_norm;
    for (size_t i = tid; i < n4; i += nth) {
        float4 v = src[i];
        v.x = policy_norm(v.x);
        v.y = policy_norm(v.y);
        v.z = policy_norm(v.z);
        v.w = policy_norm(v.w);
        dst[i] = v;
    }
    for (size_t i = n4 * 4 + tid; i < n; i += nth) a.obs_norm[i] = policy_norm(a.obs[i]);
    const int col = a.cursor ? *a.cursor - 1 : -1;  // (the front kernel of this step moved the cursor)
    const bool rec = a.h_viol && col >= 0 && col < a.hist_steps;
    for (size_t r = tid; r < (size_t)N; r += nth) {
        int tv = 0;
        for (int s = 0; s < S; ++s) tv += a.viol[r * S + s];
        a.total_viol[r] = tv;
        if (rec) {
            const size_t o = r * (size_t)a.hist_steps + (size_t)col;
            a.h_viol[o] = (int16_t)tv;
            a.h_reward[o] = a.reward[r];
            a.h_res[o] = (int16_t)a.resources[r];
        }
    }
}

}  // namespace rs

struct PolicyIo {
    int32_t* in_prbs = nullptr;
    float* in_shares = nullptr;
    int64_t* in_index = nullptr;
    int32_t* resources = nullptr;
    float* obs_norm = nullptr;
    int32_t* total_viol = nullptr;
    unsigned long long* rejected = nullptr;
    int32_t* cursor = nullptr;
    int32_t* table = nullptr;
    int32_t n_table = 0;
    int32_t hist_steps = 0;
    int16_t* h_viol = nullptr;
    double* h_reward = nullptr;
    int16_t* h_res = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::vector<void*> allocs;
};

template <class T>
static int pio_alloc(rs_handle* h, T** p, size_t n) {
    void* q = nullptr;
    const size_t bytes = sizeof(T) * (n ? n : 1);
    HIPCHK(h, guarded_malloc(&q, bytes, &h->guarded));   // (guard bands in the test build; never a region of the saved state)
    HIPCHK(h, hipMemsetAsync(q, 0, bytes, h->stream));
    if (!guards_on()) h->pio->allocs.push_back(q);
    *p = (T*)q;
    return RS_OK;
}

static int pio_create(rs_handle* h) {
    PolicyIo* p = h->pio;
    const size_t N = (size_t)h->cfg.n_envs, S = (size_t)h->n_slices;
    int rc;
    if ((rc = pio_alloc(h, &p->in_prbs, N * S)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->in_shares, N * (S + 1))) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->in_index, N)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->resources, N)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->obs_norm, N * h->n_vars)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->total_viol, N)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->rejected, 1)) != RS_OK) return rc;
    if ((rc = pio_alloc(h, &p->cursor, 1)) != RS_OK) return rc;
    HIPCHK(h, hipEventCreateWithFlags(&p->ev_in, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&p->ev_out, hipEventDisableTiming));
    return RS_OK;
}

static void policy_io_release(rs_handle* h);

static int pio_ensure(rs_handle* h) {
    if (h->pio) return RS_OK;
    HIPCHK(h, hipSetDevice(h->device));
    h->pio = new PolicyIo();
    const int rc = pio_create(h);
    if (rc != RS_OK) policy_io_release(h);  // (all or nothing: a later call tries again)
    return rc;
}

static void pio_free_history(PolicyIo* p) {
    if (p->h_viol) (void)hipFree(p->h_viol);
    if (p->h_reward) (void)hipFree(p->h_reward);
    if (p->h_res) (void)hipFree(p->h_res);
    p->h_viol = p->h_res = nullptr;
    p->h_reward = nullptr;
    p->hist_steps = 0;
}

static void policy_io_release(rs_handle* h) {
    PolicyIo* p = h->pio;
    if (!p) return;
    pio_free_history(p);
    if (p->table) (void)hipFree(p->table);
    for (void* q : p->allocs) (void)hipFree(q);
    if (p->ev_in) (void)hipEventDestroy(p->ev_in);
    if (p->ev_out) (void)hipEventDestroy(p->ev_out);
    delete p;
    h->pio = nullptr;
}

// rs_reset: the refusal counter restarts and the report cursor goes back to column 0 (ReportWrapper.reset keeps the
// recorded columns too)
static int policy_io_on_reset(rs_handle* h) {
    PolicyIo* p = h->pio;
    if (!p) return RS_OK;
    HIPCHK(h, hipMemsetAsync(p->rejected, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemsetAsync(p->cursor, 0, sizeof(int32_t), h->stream));
    return RS_OK;
}

extern "C" int rs_get_device_view(rs_handle* h, rs_device_view* out) {
    if (!h || !out) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    int rc = pio_ensure(h);
    if (rc != RS_OK) return rc;
    const PolicyIo* p = h->pio;
    memset(out, 0, sizeof *out);
    out->device = h->device;
    out->n_envs = h->cfg.n_envs;
    out->n_slices = h->n_slices;
    out->n_vars = h->n_vars;
    out->stream = (void*)h->stream;
    out->in_prbs = p->in_prbs;
    out->in_shares = p->in_shares;
    out->in_index = p->in_index;
    out->actions = h->d_actions;
    out->resources = p->resources;
    out->obs = h->d_obs;
    out->obs_norm = p->obs_norm;
    out->reward = h->d_reward;
    out->labels = h->d_labels;
    out->violations = h->d_viol;
    out->total_violations = p->total_viol;
    out->rejected = (int64_t*)p->rejected;
    return RS_OK;
}

extern "C" int rs_step_device(rs_handle* h, int kind, const void* actions_device, void* caller_stream) {
    if (!h || !actions_device) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    if (kind != RS_ACT_PRBS && kind != RS_ACT_SHARES && kind != RS_ACT_INDEX) {
        h->err = "rs_step_device: unknown action kind";
        return RS_EINVAL;
    }
    if (h->n_slices > 8) {
        h->err = "rs_step_device: at most 8 action entries per replica";
        return RS_EINVAL;
    }
    if (!h->is_reset) {
        h->err = "rs_step_device: call rs_reset first";
        return RS_ESTATE;
    }
    int rc = pio_ensure(h);
    if (rc != RS_OK) return rc;
    PolicyIo* p = h->pio;
    if (kind == RS_ACT_INDEX && !p->table) {
        h->err = "rs_step_device: RS_ACT_INDEX needs an action table (rs_set_action_table)";
        return RS_ESTATE;
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (h->hint_auto) {  // the allocations are not in sight of the host: the instance of the on-device script (a hint, same results)
        const int want = auto_hint(h);
        if (want != h->block_hint) {
            h->block_hint = want;
            drop_graph(h);
        }
    }
    hipStream_t cs = (hipStream_t)caller_stream;
    const bool foreign = cs != h->stream;
    if (foreign && (rc = stream_after(h, &p->ev_in, cs, h->stream)) != RS_OK) return rc;
    const unsigned nb = (unsigned)((h->cfg.n_envs + 255) / 256);
    rs::FrontArgs f;
    f.D = h->ddev;
    f.kind = kind;
    f.in = actions_device;
    f.table = p->table;
    f.n_table = p->n_table;
    f.actions = h->d_actions;
    f.resources = p->resources;
    f.rejected = p->rejected;
    f.cursor = p->cursor;
    f.hist_steps = p->hist_steps;
    hipLaunchKernelGGL(rs::policy_front_kernel, dim3(nb), dim3(256), 0, h->stream, f);
    if ((rc = launch_step(h)) != RS_OK) return rc;  // (forks to and joins its side streams on h->stream)
    rs::BackArgs b;
    b.D = h->ddev;
    b.obs = h->d_obs;
    b.obs_norm = p->obs_norm;
    b.viol = h->d_viol;
    b.reward = h->d_reward;
    b.resources = p->resources;
    b.total_viol = p->total_viol;
    b.cursor = p->cursor;
    b.hist_steps = p->hist_steps;
    b.h_viol = p->h_viol;
    b.h_reward = p->h_reward;
    b.h_res = p->h_res;
    const size_t quads = ((size_t)h->cfg.n_envs * h->n_vars + 3) / 4;
    size_t blocks = (quads + 255) / 256;
    if (blocks < nb) blocks = nb;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(rs::policy_back_kernel, dim3((unsigned)blocks), dim3(256), 0, h->stream, b);
    HIPCHK(h, hipGetLastError());
    return foreign ? stream_after(h, &p->ev_out, h->stream, cs) : RS_OK;
}

extern "C" int rs_stream_join(rs_handle* h, void* caller_stream) {
    if (!h) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    hipStream_t cs = (hipStream_t)caller_stream;
    if (cs == h->stream) return RS_OK;
    int rc = pio_ensure(h);
    if (rc != RS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return stream_after(h, &h->pio->ev_out, h->stream, cs);
}

extern "C" int rs_set_action_table(rs_handle* h, const int32_t* table, int32_t n_actions) {
    if (!h || !table || n_actions <= 0) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    int rc = pio_ensure(h);
    if (rc != RS_OK) return rc;
    PolicyIo* p = h->pio;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // (steps in flight may read the old table)
    if (p->table) (void)hipFree(p->table);
    p->table = nullptr;
    p->n_table = 0;
    const size_t bytes = sizeof(int32_t) * (size_t)n_actions * h->n_slices;
    HIPCHK(h, hipMalloc((void**)&p->table, bytes));
    HIPCHK(h, hipMemcpy(p->table, table, bytes, hipMemcpyHostToDevice));
    p->n_table = n_actions;
    return RS_OK;
}

static int pio_new_history(rs_handle* h, int32_t steps, int16_t** v, double** rw, int16_t** rs_) {
    const size_t n = (size_t)h->cfg.n_envs * (size_t)steps;
    HIPCHK(h, hipMalloc((void**)v, sizeof(int16_t) * (n ? n : 1)));
    HIPCHK(h, hipMalloc((void**)rw, sizeof(double) * (n ? n : 1)));
    HIPCHK(h, hipMalloc((void**)rs_, sizeof(int16_t) * (n ? n : 1)));
    if (n) {
        HIPCHK(h, hipMemsetAsync(*v, 0, sizeof(int16_t) * n, h->stream));
        HIPCHK(h, hipMemsetAsync(*rw, 0, sizeof(double) * n, h->stream));
        HIPCHK(h, hipMemsetAsync(*rs_, 0, sizeof(int16_t) * n, h->stream));
    }
    return RS_OK;
}

extern "C" int rs_report_begin(rs_handle* h, int32_t steps) {
    if (!h || steps < 0) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    int rc = pio_ensure(h);
    if (rc != RS_OK) return rc;
    PolicyIo* p = h->pio;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    pio_free_history(p);
    if ((rc = pio_new_history(h, steps, &p->h_viol, &p->h_reward, &p->h_res)) != RS_OK) return rc;
    p->hist_steps = steps;
    HIPCHK(h, hipMemsetAsync(p->cursor, 0, sizeof(int32_t), h->stream));
    return RS_OK;
}

extern "C" int rs_report_extend(rs_handle* h, int32_t eval_steps) {
    if (!h || eval_steps < 0) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    PolicyIo* p = h->pio;
    if (!p || !p->h_viol) {
        h->err = "rs_report_extend: no report history (rs_report_begin)";
        return RS_ESTATE;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int32_t old = p->hist_steps, now = old + eval_steps;
    const size_t N = (size_t)h->cfg.n_envs;
    int16_t *v = nullptr, *r = nullptr;
    double* w = nullptr;
    int rc = pio_new_history(h, now, &v, &w, &r);
    if (rc != RS_OK) return rc;
    if (old > 0) {
        HIPCHK(h, hipMemcpy2DAsync(v, sizeof(int16_t) * now, p->h_viol, sizeof(int16_t) * old, sizeof(int16_t) * old, N, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpy2DAsync(w, sizeof(double) * now, p->h_reward, sizeof(double) * old, sizeof(double) * old, N, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpy2DAsync(r, sizeof(int16_t) * now, p->h_res, sizeof(int16_t) * old, sizeof(int16_t) * old, N, hipMemcpyDeviceToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(p->cursor, &old, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));  // cursor := steps
    HIPCHK(h, hipStreamSynchronize(h->stream));
    pio_free_history(p);
    p->h_viol = v;
    p->h_reward = w;
    p->h_res = r;
    p->hist_steps = now;
    return RS_OK;
}

extern "C" int rs_report_fetch(rs_handle* h, int16_t* violation, double* reward, int16_t* resources, int32_t* n_recorded) {
    if (!h) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    PolicyIo* p = h->pio;
    if (!p || !p->h_viol) {
        h->err = "rs_report_fetch: no report history (rs_report_begin)";
        return RS_ESTATE;
    }
    HIPCHK(h, hipSetDevice(h->device));
    const size_t n = (size_t)h->cfg.n_envs * (size_t)p->hist_steps;
    int32_t cur = 0;
    if (violation && n) HIPCHK(h, hipMemcpyAsync(violation, p->h_viol, sizeof(int16_t) * n, hipMemcpyDeviceToHost, h->stream));
    if (reward && n) HIPCHK(h, hipMemcpyAsync(reward, p->h_reward, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (resources && n) HIPCHK(h, hipMemcpyAsync(resources, p->h_res, sizeof(int16_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(&cur, p->cursor, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (n_recorded) *n_recorded = cur < p->hist_steps ? cur : p->hist_steps;
    return RS_OK;
}

extern "C" int rs_device_copy(rs_handle* h, void* dst, const void* src, uint64_t bytes, int to_device) {
    if (!h || (bytes && (!dst || !src))) return RS_EINVAL;
    if (lanes_close(h) != RS_OK) return RS_EHIP;
    HIPCHK(h, hipSetDevice(h->device));
    if (bytes == 0) return RS_OK;
    HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, h->stream));
    // a host source that is not pinned has been staged when the call returns; a host destination is complete after the wait
    if (!to_device) HIPCHK(h, hipStreamSynchronize(h->stream));
    return RS_OK;
}
