// kb_control_plus.hip -- KBRL_Control.update_control (kbrl_control.py:83-112) for ProjectronPlus learners: the closed control loop
// in Projectron++ mode, behind kb_set_control_plus.  #included by rs_api.hip after kb_fit_steps.hip: it uses
// control_bookkeeping and CtlArgs of kb_kbrl.hip, kb_fit's sample step (fit_decide, fit_rule, fit_epilogue) and the cached-prefix
// column of kb_fit_steps (steps_prefix, predict_column_steps); it changes none of their kernels.
//
// Projectron's update phase scores every candidate of the step at once and stops at "no mistake", which nine learners in ten
// reach at once.  Under the margin rule every candidate with not (y f >= 1) costs a mat-vec and may move every coefficient, so no
// score outlives the candidate it was formed for: the step IS fit_steps_learner's row -- one 256-thread workgroup per learner,
// the candidates in the reference's order, each through predict_column_steps<true>, fit_decide and fit_rule<PROJECTRON_PLUS> --
// with its row taken from the device-resident step (the state the action was taken in, the action, the labels) and
// update_control's bookkeeping between the read-only column at the executed allocation and the first candidate.  Every f,
// delta, coefficient and Kinv entry is therefore bit for bit what kb_fit_steps leaves in Projectron++ mode for the same row.

namespace kb {

struct CtlPlusArgs {
    CtlArgs C;
    unsigned long long* work;  // [4] samples, samples that changed a dictionary, insertions, kernel evaluations since the switch was set
};

__global__ __launch_bounds__(256) void control_plus_kernel(CtlPlusArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    const KbDev& D = A.C.D;
    const KbState& K = A.C.K;
    const int task = blockIdx.x;  // (grid = n_envs x S; per-replica dictionaries only: the task names the dictionary too)
    const int env = task / D.S, s = task - env * D.S;
    const int dt = task;
    const uint64_t* sh = shells_of(D, K, dt);
    const int d = D.dims[s] + 1, n = D.n_prbs;
    int m = K.m[dt];
    const int act = A.C.action[task];
    const int y = A.C.labels[task] == 1 ? 1 : -1;
    stage_state(D, A.C.state, env, s, d, sm);
    if ((int)threadIdx.x == d - 1) sm.x[d - 1] = (double)act / (double)n;
    __syncthreads();
    // the state-coordinate prefixes of the step: thread t forms, and later reads, the entries j = t, t + 256, ...
    for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);

    // ---- update_control's first predict (kbrl_control.py:88): f at the executed allocation, by kb_fit_steps's f_at chain, read-only
    double f0 = 0.0;
    if (m > 0) f0 = predict_column_steps<false>(D, K, sh, d, m, sm.x, pre, sm);
    // its decision: the sign, an exact 0 against a populated dictionary draws (fit_decide; an empty dictionary answers 0)
    const int y_pred = fit_decide(K, task, env, s, m, &f0, sm);
    // the hit, the accuracy table under K.margins / K.adjusted, the security factor, hits (kbrl_control.py:89-101):
    // control_bookkeeping is a one-wave routine, so wave 0 runs it -- on the decision, which it takes as a non-zero f0 (no draw
    // of its own, no barrier inside)
    if (threadIdx.x < 64) (void)control_bookkeeping(D, K, task, env, s, m, (double)y_pred, y, A.C.hits, sm);

    // ---- sample augmentation (kbrl_control.py:102-112), in the reference's order, every candidate through the margin rule
    const int a0 = y > 0 ? act : 0, a1 = y > 0 ? n : act;
    FitCounts c = {0, 0, 0, 0};
    int row_mist = 0, row_grow = 0, row_matvec = 0;
    double f = 0.0;
    for (int a = a0; a <= a1; ++a) {
        __syncthreads();  // (the previous sample's readers of sm.x are done; an inserted landmark's prefix is in place)
        if (threadIdx.x == 0) sm.x[d - 1] = (double)a / (double)n;
        __syncthreads();
        f = predict_column_steps<true>(D, K, sh, d, m, sm.x, pre, sm);
        (void)fit_decide(K, task, env, s, m, &f, sm);
        c.evals += (unsigned long long)m;
        int branch;
        double delta;
        const int m_new = fit_rule<KB_ALG_PROJECTRON_PLUS>(D, K, dt, env, m, d, sm.x, y, f, sm, &branch, &delta, &row_mist, &row_grow);
        // a landmark inserted inside the step: its prefix by the same chain, formed by the thread that reads it
        if (m_new > m && m < KB_STEPS_PRE && (int)threadIdx.x == (m & 255)) pre[m] = steps_prefix(K, sh, d, m, sm.x);
        row_matvec += branch != 0;  // (branches 1-4 formed d* = Kinv K_f: the mat-vec)
        m = m_new;
    }
    c.samples = (unsigned long long)(a1 - a0 + 1);
    c.mistakes = (unsigned long long)row_mist;
    c.insertions = (unsigned long long)row_grow;
    if (threadIdx.x == 0) {
        K.m[dt] = m;
        fit_epilogue(K, task, f, A.work, &c);
        // whatever select_action left for this learner describes another dictionary, or another K_f row: no stored scores (the
        // versions moved with every change; this holds for a step that changed nothing, too)
        K.fver[task] = -1;
        // kb_get_repair_work's work[6]: the samples of this mode that ran the mat-vec (what batching them would act on)
        if (row_matvec) atomicAdd(&K.hv_work[6], (unsigned long long)row_matvec);
    }
}

}  // namespace kb

static void kb_control_plus_release(kb_handle* k) {
    if (k->d_ctl_work) (void)hipFree(k->d_ctl_work);
    k->d_ctl_work = nullptr;
}

// the update phase of a closed-loop step in Projectron++ mode: one launch (launch_update_control times it as span 0)
static int launch_control_plus(kb_handle* k, const kb::CtlArgs& c) {
    kb::CtlPlusArgs a;
    a.C = c;
    a.work = k->d_ctl_work;
    hipLaunchKernelGGL(kb::control_plus_kernel, dim3((unsigned)k->T), dim3(256), 0, k->stream, a);
    return RS_OK;
}

/* Whether the closed control loop learns in Projectron++ mode (ranslice.h): host state of the handle, beside the
   algorithm.  It has an effect only while the handle is in Projectron++ mode. */
extern "C" int kb_set_control_plus(kb_handle* k, int32_t on) {
    if (!k) return RS_EINVAL;
    if (on != 0 && on != 1) {
        k->err = "kb_set_control_plus: on = " + std::to_string(on) + " (0: the control loop refuses Projectron++ mode, the default; 1: it learns by the margin rule)";
        return RS_EINVAL;
    }
    const int refused = kb_refuse_non_learning(k, "kb_set_control_plus", "kb_update_control");
    if (refused != RS_OK) return refused;
    if (on && !k->d_ctl_work) {  // (here, not at the first launch: that may be inside a stream capture)
        HIPCHK(k, hipSetDevice(k->device));
        HIPCHK(k, hipMalloc((void**)&k->d_ctl_work, sizeof(unsigned long long) * 4));
        HIPCHK(k, hipMemsetAsync(k->d_ctl_work, 0, sizeof(unsigned long long) * 4, k->stream));
    }
    if (k->control_plus != on) {  // (a captured loop carries the update phase it was captured with)
        const int rc = kb_retire_graph(k);
        if (rc != RS_OK) return rc;
    }
    k->control_plus = on;
    return RS_OK;
}

extern "C" int kb_get_control_plus(kb_handle* k, int32_t* on) {
    if (!k || !on) return RS_EINVAL;
    *on = k->control_plus;
    return RS_OK;
}
