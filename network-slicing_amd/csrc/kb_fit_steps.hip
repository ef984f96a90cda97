// kb_fit_steps.hip -- kb_fit for logs of control steps: the log (state, action, SLA labels) is staged as it was recorded and the
// sample augmentation of kbrl_control.py:103-112 runs on the device, next to the loop that consumes it.  #included by rs_api.hip
// after kb_fit.hip: it uses kb_fit's sample step (fit_decide, fit_rule, fit_epilogue), its host framing (kb_fit_can_learn, kb_fit_list,
// kb_fit_open / kb_fit_close, FitStage), counters and timing, and predict_column_steps of kb_kbrl.hip beside predict_column; it
// changes none of their kernels.
//
// A logged step of a learner stands for up to n_prbs + 1 samples that differ only in their last coordinate: label +1 at allocation
// a gives (state, a / n_prbs), ..., (state, n_prbs / n_prbs), label -1 gives (state, 0), ..., (state, a / n_prbs) -- what
// ranslice.kbrl_dev.augmented_samples writes out as rows of 16 doubles for kb_fit.  fit_steps_kernel generates them in place:
// one 256-thread workgroup per (listed agent, slice), persistent over the agent's rows of the launch, and per sample fit_learner's
// sequence -- the kernel column and f, the tie draw on an exact f == 0 against a populated dictionary, the rule -- by the same
// device functions (in Projectron++ mode kb_set_fit_steps_batch replaces that launch by persistent workgroups that take the learners
// from a ticket: kb_fit_steps_batch.hip).  The one difference is where the kernel column's distances come from.  predict_column sums dist over the
// coordinates in order, the allocation last; the sum over the state coordinates is therefore the same double for every candidate
// of a step, and it is formed once per landmark and step (steps_prefix, kept in LDS for the first KB_STEPS_PRE landmarks and
// formed again per sample beyond them) instead of once per landmark and sample.  The library is built without contraction or
// reassociation, so prefix + t t is the double predict_column's chain ends with, and every f, delta, coefficient and Kinv entry
// is bit for bit kb_fit's on augmented_samples of the same rows.  A landmark inserted in the middle of a row gets its prefix by
// the same chain, from the coordinates the insertion stored.  In Projectron++ mode the loop runs as fit_steps_plus_kernel.
//
// The chip-wide rounds of kb_fit_wide.hip are not used here: kb_set_fit_wide / kb_set_fit_wide_plus have no effect on
// kb_fit_steps, and kb_fit_wide_info keeps describing the last kb_fit.

namespace kb {

struct StepsArgs {
    KbDev D;
    KbState K;
    const int32_t* agent;      // [n]
    const long long* first;    // [n + 1] log rows of agent i
    const float* state;        // [rows][nv]
    const int32_t* action;     // [rows][S]
    const int32_t* labels;     // [rows][S]
    long long from;            // this launch teaches rows first[i] + from .. first[i] + from + chunk - 1 of every agent
    int chunk;
    double* f_at;              // [rows][S] each
    int32_t* y_at;
    int32_t* changed;
    int32_t* grown;
    int32_t* m_after;
    unsigned long long* work;  // [0..3] samples, mistakes, insertions, kernel evaluations of the call
};

// The persistent loop of one learner over its agent's log rows, once per update rule as fit_learner is.  `pre`: the calling
// kernel's KB_STEPS_PRE doubles of LDS for the state-coordinate prefixes.
template <int ALG>
__device__ __forceinline__ void fit_steps_learner(const StepsArgs& A, Lds& sm, double* pre) {
    const KbDev& D = A.D;
    const KbState& K = A.K;
    const int i = blockIdx.x / D.S, s = blockIdx.x - i * D.S;
    const long long r0 = A.first[i] + A.from;
    const long long r1 = A.first[i + 1] < r0 + A.chunk ? A.first[i + 1] : r0 + A.chunk;
    if (r0 >= r1) return;
    const int env = A.agent[i], task = env * D.S + s;
    const int dt = task;  // (per-replica dictionaries only: kb_fit_steps refuses shared ones)
    const uint64_t* sh = shells_of(D, K, dt);
    const int d = D.dims[s] + 1, n = D.n_prbs;
    int m = K.m[dt];
    FitCounts c = {0, 0, 0, 0};
    double f = 0.0;
    for (long long r = r0; r < r1; ++r) {
        const size_t o = (size_t)r * D.S + s;
        const int y = A.labels[o];
        if (y == 0) {  // (block-uniform) this learner skips the row
            if (threadIdx.x == 0) {
                A.f_at[o] = 0.0;
                A.y_at[o] = 0;
                A.changed[o] = 0;
                A.grown[o] = 0;
                A.m_after[o] = m;
            }
            continue;
        }
        const int act = A.action[o];
        __syncthreads();  // (the previous row's readers of sm.x and pre are done)
        if ((int)threadIdx.x < d - 1) sm.x[threadIdx.x] = (double)A.state[(size_t)r * D.nv + D.off[s] + threadIdx.x];
        if ((int)threadIdx.x == d - 1) sm.x[d - 1] = (double)act / (double)n;
        __syncthreads();
        // the state-coordinate prefixes of the row: thread t forms, and later reads, the entries j = t, t + 256, ...
        for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);
        const int m0 = m;
        const int a0 = y > 0 ? act : 0, a1 = y > 0 ? n : act;
        // f at the logged allocation, before the row's first sample.  Label +1: that IS the first sample, whose f is taken below
        double f_at = 0.0;
        if (y < 0 && m > 0) f_at = predict_column_steps<false>(D, K, sh, d, m, sm.x, pre, sm);
        int row_mist = 0, row_grow = 0;
        for (int a = a0; a <= a1; ++a) {
            __syncthreads();  // (the previous sample's readers of sm.x are done; an inserted landmark's prefix is in place)
            if (threadIdx.x == 0) sm.x[d - 1] = (double)a / (double)n;
            __syncthreads();
            f = predict_column_steps<true>(D, K, sh, d, m, sm.x, pre, sm);
            (void)fit_decide(K, task, env, s, m, &f, sm);  // (the tie draws as in kb_fit; the summaries keep f alone)
            if (y > 0 && a == a0) f_at = f;
            c.evals += (unsigned long long)m;
            int branch;
            double delta;
            const int m_new = fit_rule<ALG>(D, K, dt, env, m, d, sm.x, y, f, sm, &branch, &delta, &row_mist, &row_grow);
            // a landmark inserted inside the row: its prefix by the same chain, from the coordinates the insertion stored, formed
            // by the thread that reads it (finish_update ended with a barrier behind its stores)
            if (m_new > m && m < KB_STEPS_PRE && (int)threadIdx.x == (m & 255)) pre[m] = steps_prefix(K, sh, d, m, sm.x);
            m = m_new;
        }
        c.samples += (unsigned long long)(a1 - a0 + 1);
        c.mistakes += (unsigned long long)row_mist;
        c.insertions += (unsigned long long)row_grow;
        if (threadIdx.x == 0) {
            A.f_at[o] = f_at;
            A.y_at[o] = m0 > 0 ? (f_at > 0.0 ? 1 : (f_at < 0.0 ? -1 : 0)) : 0;
            A.changed[o] = row_mist;
            A.grown[o] = row_grow;
            A.m_after[o] = m;
        }
    }
    if (c.samples == 0) return;  // every row of the launch skipped: the learner is not touched at all
    if (threadIdx.x == 0) {
        K.m[dt] = m;
        fit_epilogue(K, task, f, A.work, &c);
    }
}

__global__ __launch_bounds__(256) void fit_steps_kernel(StepsArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    fit_steps_learner<KB_ALG_PROJECTRON>(A, sm, pre);
}

__global__ __launch_bounds__(256) void fit_steps_plus_kernel(StepsArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    fit_steps_learner<KB_ALG_PROJECTRON_PLUS>(A, sm, pre);
}

}  // namespace kb

// kb_set_fit_steps_batch (kb_fit_steps_batch.hip): its counters start over with a call; one chunk of the call's learners, grouped
static int kb_fit_steps_batch_open(kb_handle* k);
static int launch_fit_steps_batch(kb_handle* k, const kb::StepsArgs& a, int32_t learners);

extern "C" int kb_fit_steps(kb_handle* k, const int32_t* agent, int32_t n, const int64_t* first, const float* state,
                            const int32_t* action, const int32_t* labels, int32_t chunk, double* f_at, int32_t* y_at,
                            int32_t* changed, int32_t* grown, int32_t* m_after) {
    if (!k) return RS_EINVAL;
    if (!k->is_reset) {
        k->err = "kb_fit_steps: call kb_reset first";
        return RS_ESTATE;
    }
    int rc = kb_fit_can_learn(k, "kb_fit_steps");
    if (rc != RS_OK) return rc;
    if (n < 0 || chunk < 0 || (n > 0 && (!agent || !first))) {
        k->err = "kb_fit_steps: n or chunk is negative, or agent / first is NULL";
        return RS_EINVAL;
    }
    if (n == 0) return RS_OK;
    const int32_t S = k->D.S, nv = k->D.nv, P = k->D.n_prbs;
    if ((rc = kb_fit_list(k, "kb_fit_steps", "agent", "agent", "rows", agent, n, k->D.n_envs)) != RS_OK) return rc;
    if (first[0] != 0) {
        k->err = "kb_fit_steps: first[0] must be 0";
        return RS_EINVAL;
    }
    int64_t rows = 0;
    if ((rc = kb_fit_ranges(k, "kb_fit_steps", first, n, &rows)) != RS_OK) return rc;
    if (rows == 0) return RS_OK;
    if (!state || !action || !labels) {
        k->err = "kb_fit_steps: state, action or labels is NULL";
        return RS_EINVAL;
    }
    const size_t R = (size_t)rows, RS = R * (size_t)S;
    for (size_t o = 0; o < RS; ++o) {
        const int32_t lab = labels[o];
        if (lab != 1 && lab != -1 && lab != 0) {
            k->err = "kb_fit_steps: labels[" + std::to_string(o / (size_t)S) + "][" + std::to_string(o % (size_t)S) + "] = " + std::to_string(lab) + " is none of +1, -1, 0";
            return RS_EINVAL;
        }
        if (lab != 0 && (action[o] < 0 || action[o] > P)) {
            k->err = "kb_fit_steps: action[" + std::to_string(o / (size_t)S) + "][" + std::to_string(o % (size_t)S) + "] = " + std::to_string(action[o]) + " lies outside 0 .. " + std::to_string(P);
            return RS_EINVAL;
        }
    }
    int64_t longest = 0;
    for (int32_t i = 0; i < n; ++i) longest = std::max<int64_t>(longest, first[i + 1] - first[i]);
    if (chunk == 0) chunk = std::max<int32_t>(1, KB_FIT_CHUNK / (P + 1));  // about kb_fit's default in samples of one learner
    if ((rc = kb_fit_open(k)) != RS_OK) return rc;  // (d_work[8..11], kb_fit_wide_info, stay the last kb_fit's)
    if ((rc = kb_fit_steps_batch_open(k)) != RS_OK) return rc;
    kb_fit_state* p = k->fit;
    std::vector<long long> rel((size_t)n + 1);
    for (int32_t i = 0; i <= n; ++i) rel[(size_t)i] = (long long)first[i];
    kb::StepsArgs a;
    memset(&a, 0, sizeof a);
    a.D = k->D;
    a.K = k->K;
    a.chunk = chunk;
    a.work = p->d_work;
    // the log as it was recorded: rows x (4 nv + 8 S) bytes in, rows x S x 24 bytes of summaries out
    int32_t *d_agent = nullptr, *d_action = nullptr, *d_labels = nullptr;
    long long* d_first = nullptr;
    float* d_state = nullptr;
    FitStage st;
    HIPCHK(k, st.alloc([&](FitStage& s) {
        a.agent = d_agent = s.take<int32_t>((size_t)n);
        a.first = d_first = s.take<long long>((size_t)n + 1);
        a.state = d_state = s.take<float>(R * (size_t)nv);
        a.action = d_action = s.take<int32_t>(RS);
        a.labels = d_labels = s.take<int32_t>(RS);
        a.y_at = s.take<int32_t>(RS);
        a.changed = s.take<int32_t>(RS);
        a.grown = s.take<int32_t>(RS);
        a.m_after = s.take<int32_t>(RS);
        a.f_at = s.take<double>(RS);
    }));
    HIPCHK(k, hipMemcpyAsync(d_agent, agent, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_first, rel.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_state, state, sizeof(float) * R * (size_t)nv, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_action, action, sizeof(int32_t) * RS, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_labels, labels, sizeof(int32_t) * RS, hipMemcpyHostToDevice, k->stream));
    const unsigned grid = (unsigned)n * (unsigned)S;
    for (int64_t from = 0; from < longest; from += chunk) {  // (no launch runs longer than `chunk` rows of one agent)
        a.from = (long long)from;
        hipEvent_t e;
        HIPCHK(k, p->fit_spans.begin(k->stream, 0, &e));
        if (k->alg == KB_ALG_PROJECTRON_PLUS && k->fsb.width > 0)  // (kb_set_fit_steps_batch: `width` candidates of a row per pass over Kinv)
            (void)launch_fit_steps_batch(k, a, n * S);
        else if (k->alg == KB_ALG_PROJECTRON_PLUS)
            hipLaunchKernelGGL(kb::fit_steps_plus_kernel, dim3(grid), dim3(256), 0, k->stream, a);
        else
            hipLaunchKernelGGL(kb::fit_steps_kernel, dim3(grid), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
    }
    HIPCHK(k, hipGetLastError());
    if (f_at) HIPCHK(k, hipMemcpyAsync(f_at, a.f_at, sizeof(double) * RS, hipMemcpyDeviceToHost, k->stream));
    if (y_at) HIPCHK(k, hipMemcpyAsync(y_at, a.y_at, sizeof(int32_t) * RS, hipMemcpyDeviceToHost, k->stream));
    if (changed) HIPCHK(k, hipMemcpyAsync(changed, a.changed, sizeof(int32_t) * RS, hipMemcpyDeviceToHost, k->stream));
    if (grown) HIPCHK(k, hipMemcpyAsync(grown, a.grown, sizeof(int32_t) * RS, hipMemcpyDeviceToHost, k->stream));
    if (m_after) HIPCHK(k, hipMemcpyAsync(m_after, a.m_after, sizeof(int32_t) * RS, hipMemcpyDeviceToHost, k->stream));
    return kb_fit_close(k);
}
