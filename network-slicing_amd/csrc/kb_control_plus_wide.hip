// kb_control_plus_wide.hip -- the closed control loop in Projectron++ mode with the passes over Kinv of its LARGE learners spread
// over the chip, behind kb_set_control_plus_wide.  #included by rs_api.hip after kb_control_plus_batch.hip: it adds
// kernels of its own (cpw_*), shares device functions with that file (plus_group_walk, BatchLds, BatchWork), kb_fit.hip
// (fit_decide, fit_epilogue), kb_fit_steps.hip's column chain in kb_kbrl.hip (steps_prefix, predict_column_steps) and the work line
// of kb_kbrl.hip (block_scan1024, stretch_of / walk_stretch, finish_update(..., defer_rank1 = true), margin_update, rank1_units),
// and changes none of their kernels.  With the switch off launch_update_control launches control_plus_batch_kernel itself.
//
// control_plus_batch_kernel gives a learner's whole row to ONE workgroup: every pass d* = Kinv K_f of a group of candidates, O(m^2),
// is streamed by four waves while the rest of the chip has nothing to do once the small learners are through.  Here the learners that
// hold min_landmarks .. min(max_landmarks, the batch setting's max_landmarks) at the start of the update phase -- in task order the first KB_CPW_SLOTS of them; the others
// stay on the batch kernel's row -- take a SLOT each (a record and an arena for a group's K_f and d* columns, always eight wide)
// and advance in ROUNDS of plain launches on the agent's stream:
//   cpw_list_kernel      which learners are heavy, their slots (one workgroup; block_scan1024 over the tasks)
//   cpw_rows_kernel<W>   control_plus_batch_kernel's row for everybody: the state, f0 at the executed allocation, fit_decide,
//                        control_bookkeeping; a light learner then walks its row (plus_group_walk<W>) and ends it, a heavy one
//                        stops behind the head with its cursor at a0
//   cpw_walk_kernel<W>   once in front of the rounds: forms every heavy learner's first group that needs a pass
//   `rounds` times:
//     cpw_plan_kernel(0)   the output blocks of the learners with a group waiting laid end to end: n_b units of n_b tiles each
//     cpw_pass_kernel<W>   every wave the units of an equal stretch of that line: d* of the group's columns, arena to arena
//     cpw_walk_kernel<W>   one workgroup per slot: the group's members in order through the margin rule (plus_group_walk's
//                          step 5); an insertion ends the group behind itself and the learner's round (its delta and old m are
//                          queued); else the next groups' columns and scores, the skip rule, until a group needs a pass (its
//                          columns stay in the arena for the next round) or the row ends (the row's epilogue)
//     cpw_plan_kernel(1)   the 16-row units of the learners that inserted, end to end
//     cpw_rank1_kernel     rank1_units over equal stretches
//   cpw_finish_kernel<W> one workgroup per heavy row that is still open: plus_group_walk<W> from the cursor to a1, the epilogue.
//                        (Every round ends with its own rank-1 launch, so no rank-1 update is ever pending here.)  A learner whose
//                        insertion took it past that limit is left to this kernel, which walks it in the batch kernel's arena
//                        with the batch kernel's max_landmarks: grouped or one by one exactly as the batch kernel would.
// NO kernel waits for another, polls or spins; one with nothing to do returns at once; nothing on the host waits.  Every hand-off
// crosses a kernel boundary on one stream.  So the results cannot depend on `rounds`, and a captured loop carries the sequence.
//
// THE BITS are control_plus_batch_kernel's at the same width.  Groups begin and end where its groups do (a group is never split
// over two launches of the walk kernel, so `dirty` is a register); when a member is walked Kinv and the landmarks are what they were
// when its group was formed; a unit's sums are batch_matvec's whatever wave forms them (cpw_unit restates the body of its loop);
// the deferred rank-1 forms every entry as old + (d_i d_j) / delta whatever the stretch; pre[] is formed again per launch by
// steps_prefix's chain; everything per candidate is the same device function called in the same order, and the tie stream and the
// counters live in global memory and are touched in candidate order.  The batch counters (kb_control_plus_batch_info) count a
// group, its pass, tiles and columns when its d* is CONSUMED: a group the last round left waiting is formed again by the finisher
// and counted there, once.
//
// Scratch, all of it allocated by the setter (T = n_envs x n_slices learners, slots = min(T, KB_CPW_SLOTS)):
//     scratch_bytes = KB_CPW_HEAD + slots x KB_CPW_REC + 2 x (slots + 1) x 8 + 8 x ceil(T / 2) + slots x 2 x KB_CPB_W x max_landmarks x 8
// (KB_CPW_HEAD = 128: work[8] and the count of heavy rows; KB_CPW_REC = 256: a slot's record; the two work lines; the learners'
// slot numbers; the arenas.)  It is apart from K.heavy / hv_*, which belong to Projectron's queue and select_action's list.

namespace kb {

#define KB_CPW_SLOTS 1024  // heavy learners of an update phase, each with a record and an arena
#define KB_CPW_HEAD 128    // bytes in front of the records: work[8], the count of heavy rows
#define KB_CPW_REC 256     // bytes of a slot's record

struct CpwRec {
    int32_t task, state;  // state: 0 the row is done, 1 open, 2 open and left to the finisher (m > max_landmarks)
    int32_t p, a0, a1;    // the cursor (the next candidate), the row's first and last candidate
    int32_t m, y;
    int32_t g;            // candidates p .. p + g - 1 have their K_f columns in the arena and wait for d* (0: none)
    int32_t grew, gm;     // an insertion of this round waits for its rank-1 update; the size before it
    int32_t row_mist, row_grow, row_matvec, unused;
    FitCounts c;
    double f;             // the last walked candidate's f
    double delta;         // the pending insertion's
    double fs[KB_CPB_W];  // the waiting group's scores
    char pad[KB_CPW_REC - 14 * 4 - 32 - 16 - 8 * KB_CPB_W];
};
static_assert(sizeof(CpwRec) == KB_CPW_REC, "a slot's record");

struct CpwArgs {
    CtlBatchArgs B;            // the batch kernel's arguments: the light learners' rows
    unsigned long long* info;  // [8] kb_control_plus_wide_info
    int32_t* hdr;              // [0] heavy rows of this update phase
    CpwRec* rec;               // [slots]
    long long* mvbase;         // [slots + 1] the pass line
    long long* r1base;         // [slots + 1] the rank-1 line
    int32_t* slot_of;          // [T] a learner's slot, -1: light
    double* arena;             // [slots][2][KB_CPB_W][wmax]
    int32_t wmin, wmax, slots;
};

// the largest dictionary the rounds walk: the slot's arena holds wmax landmarks, and the batch kernel groups up to its own
// max_landmarks (B.max_m) -- beyond that its walk goes one by one, and so must this one, or the batch counters would differ
__device__ __forceinline__ int cpw_limit(const CpwArgs& A) { return A.wmax < A.B.max_m ? A.wmax : A.B.max_m; }

__global__ __launch_bounds__(1024) void cpw_list_kernel(CpwArgs A) {
    __shared__ long long sc[1][1024];
    const KbState& K = A.B.C.K;
    const int T = A.B.T;
    long long carry = 0;
    for (int base = 0; base < T; base += 1024) {
        const int i = base + (int)threadIdx.x;
        int w = 0;
        if (i < T) {
            const int m = K.m[i];
            w = m >= A.wmin && m <= cpw_limit(A);
        }
        long long incl[1] = {w};
        block_scan1024(incl, sc);
        if (i < T) {
            const long long slot = carry + incl[0] - 1;
            const bool take = w && slot < A.slots;
            A.slot_of[i] = take ? (int32_t)slot : -1;
            if (take) A.rec[slot].task = i;
        }
        carry += sc[0][1023];
    }
    if (threadIdx.x == 0) {
        const long long count = carry < A.slots ? carry : A.slots;
        A.hdr[0] = (int32_t)count;
        A.info[0] += (unsigned long long)count;
        A.info[1] += (unsigned long long)(carry - count);
        A.info[7] += 1;
    }
}

// control_plus_batch_kernel with one more statement: a heavy learner leaves its row behind the head (a change there is made here too)
template <int W>
__global__ __launch_bounds__(256, 2) void cpw_rows_kernel(CpwArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    __shared__ BatchLds<W> bs;
    const KbDev& D = A.B.C.D;
    const KbState& K = A.B.C.K;
    double* kfA = A.B.arena + (size_t)blockIdx.x * 2 * (size_t)W * (size_t)A.B.max_m;
    double* dsA = kfA + (size_t)W * (size_t)A.B.max_m;
    BatchWork bw;
#pragma unroll
    for (int q = 0; q < 8; ++q) bw.w[q] = 0;
    for (;;) {
        __syncthreads();  // (the previous learner's readers of sm, pre and bs are done)
        if (threadIdx.x == 0) bs.task = atomicAdd(&A.B.ticket[0], 1);
        __syncthreads();
        const int task = bs.task;
        if (task >= A.B.T) break;
        const int env = task / D.S, s = task - env * D.S;
        const int dt = task;  // (per-replica dictionaries only: the task names the dictionary too)
        const uint64_t* sh = shells_of(D, K, dt);
        const int d = D.dims[s] + 1, n = D.n_prbs;
        int m = K.m[dt];
        const int act = A.B.C.action[task];
        const int y = A.B.C.labels[task] == 1 ? 1 : -1;
        stage_state(D, A.B.C.state, env, s, d, sm);
        if ((int)threadIdx.x == d - 1) sm.x[d - 1] = (double)act / (double)n;
        __syncthreads();
        for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);

        // ---- update_control's first predict, its decision and its bookkeeping: control_plus_kernel's
        double f0 = 0.0;
        if (m > 0) f0 = predict_column_steps<false>(D, K, sh, d, m, sm.x, pre, sm);
        const int y_pred = fit_decide(K, task, env, s, m, &f0, sm);
        if (threadIdx.x < 64) (void)control_bookkeeping(D, K, task, env, s, m, (double)y_pred, y, A.B.C.hits, sm);

        const int a0 = y > 0 ? act : 0, a1 = y > 0 ? n : act;
        const int slot = A.slot_of[task];
        if (slot >= 0) {  // ---- a heavy learner: the rounds walk its row
            if (threadIdx.x == 0) {
                CpwRec& R = A.rec[slot];
                R.state = 1;
                R.p = a0;
                R.a0 = a0;
                R.a1 = a1;
                R.m = m;
                R.y = y;
                R.g = 0;
                R.grew = 0;
                R.gm = 0;
                R.row_mist = R.row_grow = R.row_matvec = 0;
                R.c = {0, 0, 0, 0};
                R.f = 0.0;
                R.delta = 0.0;
            }
            continue;
        }
        // ---- sample augmentation, in the reference's order, group by group
        FitCounts c = {0, 0, 0, 0};
        int row_mist = 0, row_grow = 0, row_matvec = 0;
        const double f = plus_group_walk<W>(D, K, dt, task, env, s, sh, d, y, a0, a1, &m, pre, sm, bs, kfA, dsA, A.B.max_m, &c, &row_mist,
                                            &row_grow, &row_matvec, &bw);
        c.samples = (unsigned long long)(a1 - a0 + 1);
        c.mistakes = (unsigned long long)row_mist;
        c.insertions = (unsigned long long)row_grow;
        if (threadIdx.x == 0) {
            K.m[dt] = m;
            fit_epilogue(K, task, f, A.B.work, &c);
            K.fver[task] = -1;
            if (row_matvec) atomicAdd(&K.hv_work[6], (unsigned long long)row_matvec);
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (bw.w[q]) atomicAdd(&A.B.bwork[q], bw.w[q]);
        // the last workgroup to leave sets the ticket back for the next launch (every other one has drawn its last ticket)
        __threadfence();
        if (atomicAdd(&A.B.ticket[1], 1) == (int)gridDim.x - 1) {
            atomicExch(&A.B.ticket[0], 0);
            atomicExch(&A.B.ticket[1], 0);
        }
    }
}

// which = 0: the pass line (per learner with a group waiting n_b units of n_b tiles each, counted in tiles) -> mvbase; 1: the rank-1
// line (16-row units of the learners that inserted) -> r1base.  One workgroup, as heavy_plan_kernel; at most KB_CPW_SLOTS slots.
__global__ __launch_bounds__(1024) void cpw_plan_kernel(CpwArgs A, int which) {
    __shared__ long long sc[1][1024];
    const int count = A.hdr[0], slot = threadIdx.x;
    long long* base_out = which ? A.r1base : A.mvbase;
    if (count == 0) {  // (the wide kernels look at the count first; the line is kept whole all the same)
        if (threadIdx.x == 0) base_out[0] = 0;
        return;
    }
    long long w = 0;
    if (slot < count) {
        const CpwRec& R = A.rec[slot];
        if (which == 0 && R.state == 1 && R.g > 0) {
            const long long nb = (R.m + 63) >> 6;
            w = nb * nb;
            atomicAdd(&A.info[2], 1ull);
            atomicAdd(&A.info[3], (unsigned long long)(nb * (nb + 1) / 2));
        }
        if (which == 1 && R.grew == 1) {
            const long long nb1 = (R.gm + 1 + 63) >> 6;
            w = nb1 * (nb1 + 1) / 2 * 4;
            atomicAdd(&A.info[4], (unsigned long long)w);
        }
    }
    long long incl[1] = {w};
    block_scan1024(incl, sc);
    if (slot < count) base_out[slot] = incl[0] - w;
    if (threadIdx.x == 0) base_out[count] = sc[0][1023];
}

// ONE output block b of d* = Kinv K_f for the g columns kf[w * ld + j] of a group, into ds[w * ld + j]: the body of batch_matvec's
// loop over b, operand for operand (a change there is made here too) -- the row of tiles in increasing b_j from zero, the column of
// tiles in increasing b_i, ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), the sum of the two.  One wave; ts / kc are its own.
template <int W>
__device__ __forceinline__ void cpw_unit(const KbState& K, const uint64_t* sh, int m, int g, const double* kf, double* ds, int ld, int b,
                                         double (*ts)[64], double (*kc)[64]) {
    const int nb = (m + 63) >> 6, lane = threadIdx.x & 63;
    const int cl = lane >> 3, sg = lane & 7;
    const int rows_b = m - 64 * b < 64 ? m - 64 * b : 64;
    // ---- its row of tiles, increasing b_j, from zero: tpart[r] = sum_c T[r][c] K_f[64 b_j + c]
    for (int bj = 0; bj < b; ++bj) {
        const double* Tp = kinv_tile_lo(K, sh, b, bj);
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < g) kc[w][lane] = kf[(size_t)w * ld + 64 * bj + lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (int x = 0; x < 8; ++x) {
            if (8 * x >= rows_b) break;  // (wave-uniform; the last row block of the dictionary)
            double tv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) tv[k] = Tp[(8 * x + cl) * 64 + sg + 8 * k];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (w < g) {  // (wave-uniform)
                    double ta = 0.0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) ta = __builtin_fma(tv[k], kc[w][sg + 8 * k], ta);
                    ta += __shfl_xor(ta, 1);
                    ta += __shfl_xor(ta, 2);
                    ta += __shfl_xor(ta, 4);
                    if (sg == 0) ts[w][8 * x + cl] = (bj == 0 ? 0.0 : ts[w][8 * x + cl]) + ta;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // (read before the next tile's column block overwrites them)
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // ---- its column of tiles, increasing b_i: dpart[c] = sum_r T[r][c] K_f[64 b_i + r]
    double dsum[W];
#pragma unroll
    for (int w = 0; w < W; ++w) dsum[w] = 0.0;
    for (int br = b; br < nb; ++br) {
        const double* Tp = kinv_tile_lo(K, sh, br, b);
        const int rows = m - 64 * br < 64 ? m - 64 * br : 64;
        double kfr[W];
#pragma unroll
        for (int w = 0; w < W; ++w) kfr[w] = (w < g && 64 * br + lane < m) ? kf[(size_t)w * ld + 64 * br + lane] : 0.0;
        double acc[W][8];
#pragma unroll
        for (int w = 0; w < W; ++w) {
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[w][u] = 0.0;
        }
        for (int x = 0; x < 8; ++x) {
            if (8 * x >= rows) break;  // (wave-uniform)
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = 8 * x + u < rows ? Tp[(8 * x + u) * 64 + lane] : 0.0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                if (w < g) {
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        if (8 * x + u < rows) acc[w][u] = __builtin_fma(v[u], readlane_f64(kfr[w], 8 * x + u), acc[w][u]);
                }
            }
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const double part = ((acc[w][0] + acc[w][1]) + (acc[w][2] + acc[w][3])) + ((acc[w][4] + acc[w][5]) + (acc[w][6] + acc[w][7]));
            dsum[w] = br == b ? part : dsum[w] + part;
        }
    }
    // the wave's own row sums, written by the lanes sg == 0 and read by lane = entry
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (64 * b + lane < m) {
#pragma unroll
        for (int w = 0; w < W; ++w)
            if (w < g) ds[(size_t)w * ld + 64 * b + lane] = dsum[w] + (b == 0 ? 0.0 : ts[w][lane]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();  // (read before the next unit overwrites them)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the pass, chip-wide: a wave takes the units whose first tile lies in its stretch of the line (a learner's unit u begins at tile
// u n_b of the learner's n_b n_b), as heavy_matvec_kernel's square storage counts them
template <int W>
__global__ __launch_bounds__(256) void cpw_pass_kernel(CpwArgs A) {
    __shared__ double tsum[4][W][64];
    __shared__ double kcol[4][W][64];
    const int count = A.hdr[0];
    if (count == 0) return;
    const KbDev& D = A.B.C.D;
    const KbState& K = A.B.C.K;
    const int wv = threadIdx.x >> 6;
    walk_stretch(A.mvbase, count, [&](int slot, long long a, long long b) {
        const CpwRec& R = A.rec[slot];
        const int m = R.m, g = R.g;
        const long long nb = (m + 63) >> 6;
        const int u0 = (int)((a + nb - 1) / nb), u1 = (int)((b + nb - 1) / nb);
        double* kf = A.arena + (size_t)slot * 2 * KB_CPB_W * (size_t)A.wmax;
        double* ds = kf + (size_t)KB_CPB_W * (size_t)A.wmax;
        const uint64_t* sh = shells_of(D, K, R.task);
        for (int u = u0; u < u1; ++u) cpw_unit<W>(K, sh, m, g, kf, ds, A.wmax, u, tsum[wv], kcol[wv]);
    });
}

// the row's epilogue: what control_plus_batch_kernel's thread 0 does behind the walk (a change there is made here too)
__device__ __forceinline__ void cpw_epilogue(const KbState& K, int task, int m, double f, unsigned long long* work, FitCounts* c, int a0,
                                             int a1, int row_mist, int row_grow, int row_matvec) {
    c->samples = (unsigned long long)(a1 - a0 + 1);
    c->mistakes = (unsigned long long)row_mist;
    c->insertions = (unsigned long long)row_grow;
    K.m[task] = m;
    fit_epilogue(K, task, f, work, c);
    K.fver[task] = -1;
    if (row_matvec) atomicAdd(&K.hv_work[6], (unsigned long long)row_matvec);
}

// the walk, one workgroup per slot: plus_group_walk's statements (a change there is made here too) cut where a group waits for its
// pass.  First the members of the group whose d* has arrived, then -- unless one of them inserted -- the next groups' columns and
// scores and the skip rule, until a group needs a pass or the row ends.
template <int W>
__global__ __launch_bounds__(256) void cpw_walk_kernel(CpwArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    __shared__ double red[W][4];
    __shared__ double gf[W];
    const int slot = blockIdx.x;
    if (slot >= A.hdr[0]) return;
    CpwRec& R = A.rec[slot];
    if (R.state != 1) {  // (done, or the finisher's; the previous round's rank-1 update has been made)
        if (threadIdx.x == 0) R.grew = 0;
        return;
    }
    const KbDev& D = A.B.C.D;
    const KbState& K = A.B.C.K;
    const int task = R.task, env = task / D.S, s = task - env * D.S;
    const int dt = task;
    const uint64_t* sh = shells_of(D, K, dt);
    const int d = D.dims[s] + 1, n = D.n_prbs;
    const int a0 = R.a0, a1 = R.a1, y = R.y, ld = A.wmax;
    int m = R.m, p = R.p, g = R.g;
    FitCounts c = R.c;
    int row_mist = R.row_mist, row_grow = R.row_grow, row_matvec = R.row_matvec;
    double f = R.f;
    double* kf = A.arena + (size_t)slot * 2 * KB_CPB_W * (size_t)ld;
    double* ds = kf + (size_t)KB_CPB_W * (size_t)ld;
    if ((int)threadIdx.x < g) gf[threadIdx.x] = R.fs[threadIdx.x];
    stage_state(D, A.B.C.state, env, s, d, sm);
    __syncthreads();
    for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);
    BatchWork bw;
#pragma unroll
    for (int q = 0; q < 8; ++q) bw.w[q] = 0;
    int grew = 0, gm = 0;
    double gdelta = 0.0;

    if (g > 0) {
        // ---- the group p .. p + g - 1, its d* in the arena: counted now that it is used
        const int nb = (m + 63) >> 6;
        bw.w[0] += 1;
        bw.w[2] += 1;
        bw.w[3] += (unsigned long long)(nb * (nb + 1) / 2);
        bw.w[4] += (unsigned long long)g;
        bool dirty = false;  // a coefficient has moved since the group's scores were formed
        int gi = 0;
        while (gi < g) {
            // ---- candidate p: its f
            if (dirty) {  // the same products with the coefficients as they are, summed again
                double ps = 0.0;
                for (int j = threadIdx.x; j < m; j += 256) ps += kf[(size_t)gi * ld + j] * *vec_at(K, sh, KB_ROW_CO, j);
                f = block_sum(ps, sm);
            } else {
                f = gf[gi];
            }
            (void)fit_decide(K, task, env, s, m, &f, sm);
            c.evals += (unsigned long long)m;
            // ---- the rule (apply_update_plus): y f >= 1 nothing; <= 0 Projectron's update; in between the margin rule
            const double margin = (double)y * f;
            int branch = 0, m_new = m;
            double delta = 0.0;
            if (!(margin >= 1.0)) {
                __syncthreads();  // (the previous candidate's readers of the rows and of sm.x are done)
                for (int j = threadIdx.x; j < m; j += 256) {
                    double* P = vec_page(K, sh, j >> 6);
                    const int l = j & 63;
                    P[KB_ROW_KF * KB_CH + l] = kf[(size_t)gi * ld + j];
                    P[KB_ROW_DS * KB_CH + l] = ds[(size_t)gi * ld + j];
                }
                if (threadIdx.x == 0) sm.x[d - 1] = (double)p / (double)n;
                __syncthreads();
                const double t_last = sm.x[d - 1];
                if (margin <= 0.0)  // (the rank-1 update of an insertion is left to cpw_rank1_kernel)
                    [[clang::always_inline]] m_new = finish_update(D, K, dt, env, m, d, sm.x, t_last, grid_index(t_last, n), y, sm, &branch, &delta, nullptr, true);
                else
                    m_new = margin_update(D, K, sh, dt, m, y, margin, sm, &branch, &delta);
                if (branch >= 1 && branch <= 3) row_mist += 1;  // (fit_rule's counters)
                if (branch == 2 && m_new > m) row_grow += 1;
                row_matvec += 1;  // (branches 1-4: the candidate used a d*)
                if (branch == 1 || branch == 3) dirty = true;
            }
            ++gi;
            ++p;
            if (m_new > m) {  // it ends the group behind itself, and the learner's round
                bw.w[5] += (unsigned long long)(g - gi);
                grew = 1;
                gm = m;
                gdelta = delta;
                m = m_new;
                break;
            }
        }
        g = 0;
    }
    int state = 1;
    if (!grew) {
        while (p <= a1) {
            // ---- the group p .. p + g - 1: its K_f columns by predict_column_steps's chain, its scores in predict_column_steps's order
            g = a1 - p + 1 < W ? a1 - p + 1 : W;
            __syncthreads();  // (the previous group's readers of the arena, red and gf are done)
            double ps[W];
#pragma unroll
            for (int w = 0; w < W; ++w) ps[w] = 0.0;
            for (int j = threadIdx.x; j < m; j += 256) {
                const double* P = vec_page(K, sh, j >> 6);
                const int l = j & 63;
                const double base = j < KB_STEPS_PRE ? pre[j] : steps_prefix(K, sh, d, j, sm.x);
                const double lam = P[(d - 1) * KB_CH + l], co = P[KB_ROW_CO * KB_CH + l];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w < g) {  // (block-uniform)
                        const double x_last = (double)(p + w) / (double)n;
                        double dist = base;
                        double t = lam - x_last;
                        dist += t * t;
                        const double k = rs_exp(-D.gamma * dist);
                        kf[(size_t)w * ld + j] = k;
                        ps[w] += k * co;
                    }
                }
            }
            // block_sum, per column: the butterfly per wave, the four wave totals in order
            const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                double v = ps[w];
                for (int dd = 32; dd >= 1; dd >>= 1) v += __shfl_xor(v, dd);
                if (lane == 0) red[w][wv] = v;
            }
            __syncthreads();
            if ((int)threadIdx.x < W) {
                double t = 0.0;
                for (int w4 = 0; w4 < 4; ++w4) t += red[threadIdx.x][w4];
                gf[threadIdx.x] = t;
            }
            __syncthreads();
            // ---- the skip rule: nobody inside the margin -> the first candidate writes nothing, so the second one's f stands, and so on
            bool any = false;
            for (int w = 0; w < g; ++w) any = any || !((double)y * gf[w] >= 1.0);
            if (any) break;  // its columns wait in the arena for the next round's pass
            bw.w[0] += 1;
            bw.w[1] += 1;
            for (int w = 0; w < g; ++w) {
                f = gf[w];
                (void)fit_decide(K, task, env, s, m, &f, sm);  // (y f >= 1: f != 0, no draw)
                c.evals += (unsigned long long)m;
            }
            p += g;
            g = 0;
        }
    } else if (p <= a1 && m > cpw_limit(A)) {
        state = 2;  // past the rounds' limit: the finisher walks the rest as the batch kernel would
    }
    if (threadIdx.x == 0) {
        if (p > a1) {
            cpw_epilogue(K, task, m, f, A.B.work, &c, a0, a1, row_mist, row_grow, row_matvec);
            state = 0;
        }
        R.state = state;
        R.p = p;
        R.m = m;
        R.g = g;
        R.grew = grew;
        R.gm = gm;
        R.delta = gdelta;
        R.row_mist = row_mist;
        R.row_grow = row_grow;
        R.row_matvec = row_matvec;
        R.c = c;
        R.f = f;
        if (g > 0) {
            for (int w = 0; w < g; ++w) R.fs[w] = gf[w];
        }
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (bw.w[q]) atomicAdd(&A.B.bwork[q], bw.w[q]);
    }
}

__global__ __launch_bounds__(256) void cpw_rank1_kernel(CpwArgs A) {
    const int count = A.hdr[0];
    if (count == 0) return;
    const KbDev& D = A.B.C.D;
    const KbState& K = A.B.C.K;
    walk_stretch(A.r1base, count, [&](int slot, long long u0, long long u1) {
        const CpwRec& R = A.rec[slot];
        rank1_units(K, shells_of(D, K, R.task), R.gm, R.delta, D.tri, (int)u0, 1, (int)u1);
    });
}

// the finisher: whatever row the rounds have left open, one workgroup each, by the batch kernel's own walk from the cursor -- in
// the batch kernel's own arena (workgroup j's: the rows kernel, which has the same number of them, is done) with its own
// max_landmarks, so that a dictionary is grouped or taken one by one here exactly where control_plus_batch_kernel would
template <int W>
__global__ __launch_bounds__(256, 2) void cpw_finish_kernel(CpwArgs A) {
    __shared__ Lds sm;
    __shared__ double pre[KB_STEPS_PRE];
    __shared__ BatchLds<W> bs;
    const int slot = blockIdx.x;
    if (slot >= A.hdr[0]) return;
    CpwRec& R = A.rec[slot];
    if (R.state == 0) return;
    const KbDev& D = A.B.C.D;
    const KbState& K = A.B.C.K;
    const int task = R.task, env = task / D.S, s = task - env * D.S;
    const int dt = task;
    const uint64_t* sh = shells_of(D, K, dt);
    const int d = D.dims[s] + 1;
    const int p0 = R.p, a0 = R.a0, a1 = R.a1, y = R.y, ld = A.B.max_m;
    int m = R.m;
    FitCounts c = R.c;
    int row_mist = R.row_mist, row_grow = R.row_grow, row_matvec = R.row_matvec;
    double* kf = A.B.arena + (size_t)blockIdx.x * 2 * (size_t)W * (size_t)ld;
    double* ds = kf + (size_t)W * (size_t)ld;
    stage_state(D, A.B.C.state, env, s, d, sm);
    __syncthreads();
    for (int j = threadIdx.x; j < m && j < KB_STEPS_PRE; j += 256) pre[j] = steps_prefix(K, sh, d, j, sm.x);
    BatchWork bw;
#pragma unroll
    for (int q = 0; q < 8; ++q) bw.w[q] = 0;
    const double f = plus_group_walk<W>(D, K, dt, task, env, s, sh, d, y, p0, a1, &m, pre, sm, bs, kf, ds, ld, &c, &row_mist, &row_grow,
                                        &row_matvec, &bw);
    if (threadIdx.x == 0) {
        cpw_epilogue(K, task, m, f, A.B.work, &c, a0, a1, row_mist, row_grow, row_matvec);
        R.state = 0;
        R.g = 0;
        atomicAdd(&A.info[5], 1ull);
        atomicAdd(&A.info[6], (unsigned long long)(a1 - p0 + 1));
#pragma unroll
        for (int q = 0; q < 8; ++q)
            if (bw.w[q]) atomicAdd(&A.B.bwork[q], bw.w[q]);
    }
}

}  // namespace kb

static void kb_control_plus_wide_release(kb_handle* k) {
    if (k->d_cpw) (void)hipFree(k->d_cpw);
    k->d_cpw = nullptr;
    k->cpw_bytes = 0;
}

static uint64_t kb_cpw_slots(const kb_handle* k) { return (uint64_t)(k->T < KB_CPW_SLOTS ? k->T : KB_CPW_SLOTS); }

static uint64_t kb_control_plus_wide_bytes(const kb_handle* k, int32_t max_landmarks) {
    const uint64_t slots = kb_cpw_slots(k), T = (uint64_t)k->T;
    return KB_CPW_HEAD + slots * KB_CPW_REC + 2 * (slots + 1) * 8 + 8 * ((T + 1) / 2) +
           slots * 2 * KB_CPB_W * (uint64_t)max_landmarks * sizeof(double);
}

// whether the update phase of a Projectron++ control step goes through the rounds (launch_update_control asks)
static bool kb_control_plus_wide_on(const kb_handle* k) { return k->cpw_min > 0 && k->cpb.width > 0 && k->d_cpw && k->cpb.d; }

template <int W>
static void kb_cpw_launch(kb_handle* k, const kb::CpwArgs& a) {
    const unsigned rows = (unsigned)(k->T < KB_CPB_ARENAS ? k->T : KB_CPB_ARENAS), slots = (unsigned)a.slots;
    hipLaunchKernelGGL(kb::cpw_list_kernel, dim3(1), dim3(1024), 0, k->stream, a);
    hipLaunchKernelGGL(kb::cpw_rows_kernel<W>, dim3(rows), dim3(256), 0, k->stream, a);
    hipLaunchKernelGGL(kb::cpw_walk_kernel<W>, dim3(slots), dim3(256), 0, k->stream, a);
    for (int r = 0; r < k->cpw_rounds; ++r) {
        hipLaunchKernelGGL(kb::cpw_plan_kernel, dim3(1), dim3(1024), 0, k->stream, a, 0);
        hipLaunchKernelGGL(kb::cpw_pass_kernel<W>, dim3((unsigned)k->cpw_grid[W == 2 ? 0 : W == 4 ? 1 : 2]), dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::cpw_walk_kernel<W>, dim3(slots), dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::cpw_plan_kernel, dim3(1), dim3(1024), 0, k->stream, a, 1);
        hipLaunchKernelGGL(kb::cpw_rank1_kernel, dim3((unsigned)k->r1_grid), dim3(256), 0, k->stream, a);
    }
    hipLaunchKernelGGL(kb::cpw_finish_kernel<W>, dim3(slots), dim3(256), 0, k->stream, a);
}

// the update phase of a closed-loop step in Projectron++ mode, grouped, the large learners by rounds (launch_update_control times
// the whole sequence as span 0)
static int launch_control_plus_wide(kb_handle* k, const kb::CtlArgs& c) {
    kb::CpwArgs a;
    a.B.C = c;
    a.B.work = k->d_ctl_work;
    (void)kb_arena_args(&a.B, k->cpb, k->T);
    const uint64_t slots = kb_cpw_slots(k), T = (uint64_t)k->T;
    char* q = k->d_cpw;
    a.info = (unsigned long long*)q;
    a.hdr = (int32_t*)(q + 64);
    q += KB_CPW_HEAD;
    a.rec = (kb::CpwRec*)q;
    q += slots * KB_CPW_REC;
    a.mvbase = (long long*)q;
    q += (slots + 1) * 8;
    a.r1base = (long long*)q;
    q += (slots + 1) * 8;
    a.slot_of = (int32_t*)q;
    q += 8 * ((T + 1) / 2);
    a.arena = (double*)q;
    a.wmin = k->cpw_min;
    a.wmax = k->cpw_max;
    a.slots = (int32_t)slots;
    kb_by_width(k->cpb.width, [&](auto w) { kb_cpw_launch<decltype(w)::value>(k, a); });
    return RS_OK;
}

/* Which learners of the closed control loop's Projectron++ update phase have their passes over Kinv spread over the chip
   (ranslice.h): host state of the handle beside the batch width.  All device scratch is allocated here -- the first
   launch may be inside a stream capture. */
extern "C" int kb_set_control_plus_wide(kb_handle* k, int32_t min_landmarks, int32_t max_landmarks, int32_t rounds) {
    if (!k) return RS_EINVAL;
    if (min_landmarks != 0) {
        const int rc = kb_check_max_landmarks(k, "kb_set_control_plus_wide", max_landmarks);
        if (rc != RS_OK) return rc;
        if (min_landmarks < 2 || min_landmarks > max_landmarks) {
            k->err = "kb_set_control_plus_wide: min_landmarks = " + std::to_string(min_landmarks) +
                     " (0 turns the rounds off, the default; else 2 .. max_landmarks = " + std::to_string(max_landmarks) +
                     ": a single landmark's float32 regime stays on the batch kernel's row)";
            return RS_EINVAL;
        }
        if (rounds < 1 || rounds > 256) {
            k->err = "kb_set_control_plus_wide: rounds = " + std::to_string(rounds) + " (1 .. 256 rounds enqueued per update phase)";
            return RS_EINVAL;
        }
    }
    const int refused = kb_refuse_non_learning(k, "kb_set_control_plus_wide", "kb_update_control");
    if (refused != RS_OK) return refused;
    if (min_landmarks == 0) max_landmarks = rounds = 0;
    HIPCHK(k, hipSetDevice(k->device));
    const bool changed = k->cpw_min != min_landmarks || k->cpw_max != max_landmarks || k->cpw_rounds != rounds;
    // (a captured loop carries the update phase and the scratch it was captured with; whatever runs on the stream still uses them)
    if (changed) {
        const int rc = kb_retire_graph(k);
        if (rc != RS_OK) return rc;
    }
    HIPCHK(k, hipStreamSynchronize(k->stream));
    if (k->cpw_max != max_landmarks) {
        kb_control_plus_wide_release(k);
        k->cpw_min = k->cpw_max = k->cpw_rounds = 0;
        if (max_landmarks) {
            const uint64_t bytes = kb_control_plus_wide_bytes(k, max_landmarks);
            HIPCHK(k, hipMalloc((void**)&k->d_cpw, (size_t)bytes));
            k->cpw_bytes = bytes;
        }
    }
    if (min_landmarks) {
        // one co-resident round of workgroups of the pass kernel, per width (as kb_create sizes the two Kinv-streaming kernels)
        int cus = 256, b = 0;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, k->device);
        k->cpw_grid[0] = k->cpw_grid[1] = k->cpw_grid[2] = 2048;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kb::cpw_pass_kernel<2>, 256, 0) == hipSuccess && b > 0) k->cpw_grid[0] = b * cus;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kb::cpw_pass_kernel<4>, 256, 0) == hipSuccess && b > 0) k->cpw_grid[1] = b * cus;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, kb::cpw_pass_kernel<8>, 256, 0) == hipSuccess && b > 0) k->cpw_grid[2] = b * cus;
    }
    // the counters since the switch was last set, and the count of heavy rows
    if (k->d_cpw) HIPCHK(k, hipMemsetAsync(k->d_cpw, 0, KB_CPW_HEAD, k->stream));
    k->cpw_min = min_landmarks;
    k->cpw_max = max_landmarks;
    k->cpw_rounds = rounds;
    return RS_OK;
}

extern "C" int kb_get_control_plus_wide(kb_handle* k, int32_t* min_landmarks, int32_t* max_landmarks, int32_t* rounds, uint64_t* scratch_bytes) {
    if (!k || !min_landmarks || !max_landmarks || !rounds || !scratch_bytes) return RS_EINVAL;
    *min_landmarks = k->cpw_min;
    *max_landmarks = k->cpw_max;
    *rounds = k->cpw_rounds;
    *scratch_bytes = k->cpw_bytes;
    return RS_OK;
}

extern "C" int kb_control_plus_wide_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    return kb_read_words(k, k->d_cpw, 8, work);
}
