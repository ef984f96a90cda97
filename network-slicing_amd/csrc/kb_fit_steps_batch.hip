// kb_fit_steps_batch.hip -- kb_fit_steps in Projectron++ mode with ONE pass over Kinv for a group of a row's candidates, behind
// kb_set_fit_steps_batch.  #included by rs_api.hip after kb_control_plus_batch.hip: it is fit_steps_learner's row
// loop (kb_fit_steps.hip) around plus_group_walk, the walk control_plus_batch_kernel runs on a control step's row, and it changes
// none of that file's, kb_fit_steps's, kb_fit's or kb_kbrl.hip's kernels.
//
// A log row is a control step's row without the bookkeeping: the same candidates a0 .. a1, in the same order, against the same
// learner.  §8m's argument holds row by row -- only an insertion changes the landmarks or Kinv, so the d* of the next `width`
// candidates are formed from one read of the stored triangle, and f, d*, delta, every coefficient and every Kinv entry are the
// doubles the one-by-one walk forms.  A group never spans rows: the next row has other state coordinates.  What the row loop adds
// to the walk is fit_steps_learner's: rows of label 0 are skipped, the five summaries are written per row, and the learner's
// counters are added once, after its last row of the launch (stated as ONE loop with a row per trip: see the kernel).  f_at is formed in front of the walk for both labels
// (predict_column_steps<false> at the logged allocation, as control_plus_batch_kernel forms f0): for label +1 that is the first
// candidate's f -- the same landmarks, coefficients, prefixes and order of sums, the float32 product at m == 1 included -- and
// fit_decide leaves f alone while m > 0.
//
// Scratch.  As in §8m every workgroup has an arena of 2 x width x max_landmarks doubles, a launch has at most KB_CPB_ARENAS
// persistent workgroups, and they take the learners (listed agent i, slice s) = (t / S, t % S) from a ticket the last workgroup to
// leave sets back: a call makes one launch per chunk on one stream, and every launch finds the ticket at zero.  The scratch is this
// setter's own (not kb_set_control_plus_batch's), sized for the handle:
//     scratch_bytes = KB_CPB_HEAD + min(n_envs x S, KB_CPB_ARENAS) x 2 x width x max_landmarks x 8
// The kernel adds nothing to K.hv_work (kb_fit_steps does not count repair work) and writes no control state.

namespace kb {

struct StepsBatchArgs {
    StepsArgs S;
    unsigned long long* bwork;  // [8] kb_fit_steps_batch_info
    int32_t* ticket;            // [2]
    double* arena;              // [gridDim.x][2][W][max_m]
    int32_t max_m, T;           // T: learners of the call, n x S
};

template <int W>
__global__ __launch_bounds__(256, 2) void fit_steps_batch_kernel(StepsBatchArgs B) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    __shared__ BatchLds<W> bs;
    const StepsArgs& A = B.S;
    const KbDev& D = A.D;
    const KbState& K = A.K;
    double* kfA = B.arena + (size_t)blockIdx.x * 2 * (size_t)W * (size_t)B.max_m;
    double* dsA = kfA + (size_t)W * (size_t)B.max_m;
    BatchWork bw;
#pragma unroll
    for (int q = 0; q < 8; ++q) bw.w[q] = 0;
    // ONE loop, a row per trip, as control_plus_batch_kernel's has a learner per trip; the learner in hand (t), its next row and its
    // last (r, r1), its size and its counters are carried from trip to trip in scalar registers -- each is the same word in every
    // lane, and is said to be (readfirstlane).  As a row loop inside a learner loop the kernel kept what depends on the learner
    // alone in vector registers over the whole walk: 124 B per lane of scratch at width 4 and 372 B at width 8, with the walk
    // standing once (control_plus_batch_kernel's 0 B and 196 B are the measure).
    int t = -1, m = 0;
    long long r = 0, r1 = 0;
    FitCounts c = {0, 0, 0, 0};
    double f = 0.0;
    for (;;) {
        if (r >= r1) {  // (block-uniform) the learner's rows of the launch are done, or none is in hand yet: close it, take the next
            if (c.samples != 0 && threadIdx.x == 0) {  // (every row skipped: the learner is not touched at all)
                const int i = t / D.S, task = A.agent[i] * D.S + (t - i * D.S);
                K.m[task] = m;
                fit_epilogue(K, task, f, A.work, &c);
            }
            __syncthreads();  // (the previous learner's readers of sm, pre and bs are done)
            if (threadIdx.x == 0) bs.task = atomicAdd(&B.ticket[0], 1);
            __syncthreads();
            t = __builtin_amdgcn_readfirstlane(bs.task);
            if (t >= B.T) break;
            const int i = t / D.S;
            r = A.first[i] + A.from;
            r1 = A.first[i + 1] < r + A.chunk ? A.first[i + 1] : r + A.chunk;
            m = K.m[A.agent[i] * D.S + (t - i * D.S)];
            c = {0, 0, 0, 0};
            f = 0.0;
            continue;  // (no row of this launch: the next trip takes the next ticket)
        }
        // ---- row r of learner t: fit_steps_learner's row
        const int i = t / D.S, s = t - i * D.S;
        const int env = A.agent[i], task = env * D.S + s;
        const int dt = task;  // (per-replica dictionaries only: kb_fit_steps refuses shared ones)
        const uint64_t* sh = shells_of(D, K, dt);
        const int d = D.dims[s] + 1, n = D.n_prbs;
        const size_t o = (size_t)r * D.S + s;
        const size_t so = (size_t)r * D.nv + D.off[s];
        ++r;
        const int y = A.labels[o];
        if (y == 0) {  // this learner skips the row
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
        if ((int)threadIdx.x < d - 1) sm.x[threadIdx.x] = (double)A.state[so + threadIdx.x];
        if ((int)threadIdx.x == d - 1) sm.x[d - 1] = (double)act / (double)n;
        __syncthreads();
        // the state-coordinate prefixes of the row: thread j forms, and later reads, the entries j, j + 256, ...
        for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);
        const int a0 = y > 0 ? act : 0, a1 = y > 0 ? n : act;
        // f at the logged allocation, before the row's first sample (for label +1 the first sample's f), written at once
        {
            double f_at = 0.0;
            if (m > 0) f_at = predict_column_steps<false>(D, K, sh, d, m, sm.x, pre, sm);
            if (threadIdx.x == 0) {
                A.f_at[o] = f_at;
                A.y_at[o] = m > 0 ? (f_at > 0.0 ? 1 : (f_at < 0.0 ? -1 : 0)) : 0;
            }
        }
        FitCounts cr = {0, 0, 0, 0};  // (of the row: at most n_prbs + 1 candidates of at most `capacity` landmarks each, far below 2^31)
        int row_mist = 0, row_grow = 0, row_matvec = 0;
        f = plus_group_walk<W>(D, K, dt, task, env, s, sh, d, y, a0, a1, &m, pre, sm, bs, kfA, dsA, B.max_m, &cr, &row_mist, &row_grow,
                               &row_matvec, &bw);
        m = __builtin_amdgcn_readfirstlane(m);
        row_mist = __builtin_amdgcn_readfirstlane(row_mist);
        row_grow = __builtin_amdgcn_readfirstlane(row_grow);
        c.samples += (unsigned long long)(a1 - a0 + 1);
        c.mistakes += (unsigned long long)row_mist;
        c.insertions += (unsigned long long)row_grow;
        c.evals += (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)cr.evals);
        if (threadIdx.x == 0) {
            A.changed[o] = row_mist;
            A.grown[o] = row_grow;
            A.m_after[o] = m;
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (bw.w[q]) atomicAdd(&B.bwork[q], bw.w[q]);
        // the last workgroup to leave sets the ticket back for the next launch (every other one has drawn its last ticket)
        __threadfence();
        if (atomicAdd(&B.ticket[1], 1) == (int)gridDim.x - 1) {
            atomicExch(&B.ticket[0], 0);
            atomicExch(&B.ticket[1], 0);
        }
    }
}

}  // namespace kb

// a kb_fit_steps call opens: kb_fit_steps_batch_info describes this call
static int kb_fit_steps_batch_open(kb_handle* k) {
    if (k->fsb.d) HIPCHK(k, hipMemsetAsync(k->fsb.d, 0, sizeof(unsigned long long) * 8, k->stream));
    return RS_OK;
}

// one chunk of a kb_fit_steps call in Projectron++ mode, grouped: one launch over the call's n x S learners
static int launch_fit_steps_batch(kb_handle* k, const kb::StepsArgs& s, int32_t learners) {
    kb::StepsBatchArgs a;
    a.S = s;
    // (no agent is listed twice, so learners <= n_envs x S and every workgroup's arena lies inside the scratch)
    const unsigned grid = kb_arena_args(&a, k->fsb, learners);
    kb_by_width(k->fsb.width, [&](auto w) {
        hipLaunchKernelGGL(kb::fit_steps_batch_kernel<decltype(w)::value>, dim3(grid), dim3(256), 0, k->stream, a);
    });
    return RS_OK;
}

/* How kb_fit_steps walks a row's candidates in Projectron++ mode (ranslice.h): host state of the handle beside alg.
   kb_set_control_plus_batch without a captured loop to retire: kb_fit_steps is in none. */
extern "C" int kb_set_fit_steps_batch(kb_handle* k, int32_t width, int32_t max_landmarks) {
    if (!k) return RS_EINVAL;
    int rc = kb_check_width(k, "kb_set_fit_steps_batch", width, "candidates of a row share one pass over Kinv");
    if (rc == RS_OK && width != 0) rc = kb_check_max_landmarks(k, "kb_set_fit_steps_batch", max_landmarks);
    if (rc == RS_OK) rc = kb_refuse_non_learning(k, "kb_set_fit_steps_batch", "kb_fit_steps");
    if (rc != RS_OK) return rc;
    if (width == 0) max_landmarks = 0;
    HIPCHK(k, hipSetDevice(k->device));
    return kb_arena_set(k, &k->fsb, width, max_landmarks);
}

extern "C" int kb_get_fit_steps_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes) {
    if (!k || !width || !max_landmarks || !scratch_bytes) return RS_EINVAL;
    *width = k->fsb.width;
    *max_landmarks = k->fsb.max;
    *scratch_bytes = k->fsb.bytes;
    return RS_OK;
}

extern "C" int kb_fit_steps_batch_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    return kb_read_words(k, k->fsb.d, 8, work);
}
