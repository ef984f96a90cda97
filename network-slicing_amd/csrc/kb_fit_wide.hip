// kb_fit_wide.hip -- kb_fit's chip-wide rounds for learners that hold large dictionaries (kb_set_fit_wide).
// #included by rs_api.hip after kb_fit.hip.  It adds kernels of its own and shares only device functions with kb_kbrl.hip and
// kb_fit.hip: score_queries (kb_score's body), predict_column, fit_decide and fit_epilogue (fit_learner's decision and epilogue),
// block_scan1024 and walk_stretch (the work line of the repair rounds), matvec_tri_tiles_lds, matvec_tri_combine_wide,
// finish_update(..., defer_rank1 = true), margin_update and rank1_units.
//
// fit_learner runs a learner's samples on ONE workgroup; every mistake then costs an O(m^2) mat-vec and, when it inserts, an O(m^2)
// rank-1 update of Kinv that this workgroup streams alone.  Here a chunk's learners whose dictionaries hold min_landmarks or more
// at the start of the chunk (fit_wide_classify_kernel, on the device) advance together in ROUNDS of plain launches:
//   fit_wide_scan_kernel     f of the next `window` samples of every pending learner against its current dictionary (score_queries:
//                            predict_column's sums, KB_SCORE_Q samples per workgroup)
//   fit_wide_decide_kernel   per learner: the first sample of the window with f y <= 0.  Those before it are final (branch 0); the
//                            mistaken one gets predict_column (its kernel column into the K_f row) and, on f == 0, its tie draw.
//                            No mistake: the cursor moves past the window
//   fit_wide_plan_kernel     the tiles of the learners with a pending mistake laid end to end (prefix sums)
//   fit_wide_matvec_kernel   every wave an equal stretch of that line (walk_stretch): matvec_tri_tiles_lds
//   fit_wide_finish_kernel   per learner: matvec_tri_combine_wide, finish_update with the rank-1 update deferred; the sample's
//                            branch, delta and size; the cursor moves past the mistake
//   fit_wide_plan_kernel     the 16-row units of the learners that inserted, end to end
//   fit_wide_rank1_kernel    rank1_units over equal stretches
// What is left of a window after a mistake is stale (the dictionary changed): the next round scans again from the cursor.
// THE BITS are fit_learner's.  A sample that is no mistake changes nothing but the K_f row and f, so scoring samples ahead of the
// dictionary's next change gives them the f they would get one by one (score_queries is predict_column bit for bit:
// tests/test_gpu_fit.py); the mistaken sample runs predict_column itself; the tile order of the mat-vec does not matter (each tile's
// partial sums have a slot of their own) and the combine, finish_update and rank1_units are the functions apply_update's path
// calls or is held to (tests/test_gpu_update_chain.py).  Dictionaries here hold two landmarks or more (kb_set_fit_wide refuses 1),
// so the float32 regime of a single landmark stays with fit_learner.
// PROJECTRON++ (kb_set_fit_wide_plus; FitArgs.alg) goes through the same seven launches.  The decide kernel stops at the first sample
// that apply_update_plus would not answer with branch 0, not (y f >= 1) in its own expression; every such sample, mistake or
// margin, gets its mat-vec; the finish kernel forms margin = y f from the f the decide kernel left in F.f and continues a mistake
// with finish_update as above and a sample inside the margin with margin_update, apply_update_plus's own tail (kb_kbrl.hip):
// branch 3 moves the coefficients and bumps the version, branch 4 writes nothing.  Neither inserts, so the rank-1 line is empty for
// them.  After branch 4 the dictionary is what it was and the rest of the window's scores would still hold; they are NOT used
// again -- the next round scans from its cursor like any other, so a slot needs no window origin and the scan kernel no second
// mode (what the rescans cost is kb_fit_wide_info's work[3]; tests/fit_wide_plus_mirror.py's counters define it).
// NO kernel waits for another: every one ends whatever the others do, and one with nothing to do returns at once.  Every round
// moves each pending learner at least one sample on, so a chunk needs at most `chunk` rounds; the host enqueues KB_FIT_ROUNDS of
// them, reads back how many learners are done, and gives up with RS_EHIP if the bound is ever passed.  The rounds' state lives in
// the call's staged block (FitWide, kb_fit.hip): K.heavy / hv_*, the control loop's queue, are not touched.

namespace kb {

#define KB_FIT_WINDOW 64       // samples per learner a round scores ahead (kb_set_fit_wide's window = 0)
#define KB_FIT_WINDOW_MAX 256
#define KB_FIT_ROUNDS 8        // rounds enqueued between two looks at the "learners done" word

// which listed learners the rounds teach this chunk: those with samples in it whose dictionary holds min_m landmarks or more now.
// They are listed in the order of the call (slot = how many came before), with their cursors at the chunk's first row.
__global__ __launch_bounds__(1024) void fit_wide_classify_kernel(WideArgs A) {
    __shared__ long long sc[1][1024];
    const FitArgs& F = A.F;
    const FitWide& W = A.W;
    long long carry = 0;
    for (int base = 0; base < A.n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        long long r0 = 0, r1 = 0;
        int w = 0;
        if (i < A.n) {
            r0 = F.first[i] + F.from;
            r1 = F.first[i + 1] < r0 + F.chunk ? F.first[i + 1] : r0 + F.chunk;
            w = r0 < r1 && F.K.m[F.task[i]] >= W.min_m;
            W.mark[i] = w;
        }
        long long incl[1] = {w};
        block_scan1024(incl, sc);
        if (w) {
            const long long slot = carry + incl[0] - 1;
            W.list[slot] = i;
            W.cur[slot] = r0;
            W.end[slot] = r1;
            W.pend[slot] = 0;
            W.grew[slot] = 0;
        }
        carry += sc[0][1023];
    }
    if (threadIdx.x == 0) {
        W.hdr[0] = (int32_t)carry;
        W.hdr[1] = 0;
    }
}

// the learner of a slot is done with the chunk: fit_learner's epilogue (K.m is kept current by the finish kernel, the counters
// were added round by round; thread 0)
__device__ __forceinline__ void fit_wide_epilogue(const KbState& K, const FitWide& W, int task, double f) {
    fit_epilogue(K, task, f, nullptr, nullptr);
    atomicAdd(&W.hdr[1], 1);
}

__global__ __launch_bounds__(256) void fit_wide_scan_kernel(WideArgs A) {
    __shared__ double xs[KB_SCORE_Q][KB_DMAX];
    __shared__ double red[KB_SCORE_Q][4];
    __shared__ double k1[KB_SCORE_Q];
    const FitWide& W = A.W;
    const int j = blockIdx.x;
    const long long cur = W.cur[j], left = W.end[j] - cur;
    const long long q0 = (long long)blockIdx.y * KB_SCORE_Q;
    const long long span = left < W.window ? left : W.window;
    if (q0 >= span) return;  // (done with the chunk, or the window ends before this block)
    const int cnt = (int)(span - q0 < KB_SCORE_Q ? span - q0 : KB_SCORE_Q);
    score_queries(A.F.D, A.F.K, A.F.task[W.list[j]], cnt, A.F.x + (cur + q0) * KB_DMAX, W.wf + (size_t)j * W.window + q0, nullptr, xs,
                  red, k1);
}

__global__ __launch_bounds__(256) void fit_wide_decide_kernel(WideArgs A) {
    const FitArgs& F = A.F;
    const KbDev& D = F.D;
    const KbState& K = F.K;
    const FitWide& W = A.W;
    __shared__ Lds sm;
    const int j = blockIdx.x;
    const long long cur = W.cur[j], end = W.end[j];
    if (cur >= end) return;
    const int task = F.task[W.list[j]], env = task / D.S, s = task - env * D.S;
    const uint64_t* sh = shells_of(D, K, task);
    const int d = D.dims[s] + 1;
    const int m = K.m[task];
    const int cnt = (int)(end - cur < W.window ? end - cur : W.window);
    const double* wf = W.wf + (size_t)j * W.window;
    const bool plus = F.alg == KB_ALG_PROJECTRON_PLUS;  // (kb_set_fit_wide_plus: the margin rule's rounds)
    // the first sample of the window that fit_learner would not pass by: a mistake f y <= 0 (an exact tie is one), or an f without
    // a sign (never met: it would draw and update nothing).  Projectron++: the first that apply_update_plus would not answer with
    // branch 0, in its own words -- not (y f >= 1): a mistake, a sample inside the margin, or a NaN
    if (threadIdx.x == 0) sm.ired[1] = cnt;
    __syncthreads();
    double fw = 0.0;
    if ((int)threadIdx.x < cnt) {
        fw = wf[threadIdx.x];
        const bool stop = plus ? !((double)F.y[cur + threadIdx.x] * fw >= 1.0)
                               : fw * (double)F.y[cur + threadIdx.x] <= 0.0 || !(fw > 0.0 || fw < 0.0);
        if (stop) atomicMin(&sm.ired[1], (int)threadIdx.x);
    }
    __syncthreads();
    const int k = sm.ired[1];
    if ((int)threadIdx.x < k) {  // final: no update
        const long long r = cur + threadIdx.x;
        F.y_pred[r] = fw > 0.0 ? 1 : -1;
        F.f[r] = fw;
        F.branch[r] = 0;
        F.delta[r] = 0.0;
        F.m_after[r] = m;
    }
    long long at = cur + k, n_final = k;
    int pend = 0;
    double f_end = 0.0;  // f of the chunk's last sample, when this round reaches it
    if (k < cnt) {
        const long long r = cur + k;
        if (threadIdx.x < KB_DMAX) sm.x[threadIdx.x] = F.x[r * KB_DMAX + threadIdx.x];
        __syncthreads();
        double f = predict_column(D, K, sh, d, m, sm.x, sm);
        const int yp = fit_decide(K, task, env, s, m, &f, sm);
        if (threadIdx.x == 0) {
            F.y_pred[r] = yp;
            F.f[r] = f;
        }
        if (plus ? !((double)F.y[r] * f >= 1.0) : f * (double)F.y[r] <= 0.0) {
            pend = 1;  // the cursor stays on it: the finish kernel moves it on (and reads its f from F.f[r])
        } else {
            if (threadIdx.x == 0) {
                F.branch[r] = 0;
                F.delta[r] = 0.0;
                F.m_after[r] = m;
            }
            n_final += 1;
            at = r + 1;
            f_end = f;
        }
    } else if (at == end) {
        // the chunk's last sample was no mistake: its kernel column goes into the K_f row, as fit_learner's predict_column leaves it
        if (threadIdx.x < KB_DMAX) sm.x[threadIdx.x] = F.x[(end - 1) * KB_DMAX + threadIdx.x];
        __syncthreads();
        f_end = predict_column(D, K, sh, d, m, sm.x, sm);
    }
    if (threadIdx.x == 0) {
        W.cur[j] = at;
        W.pend[j] = pend;
        K.stats[(size_t)task * 4 + 0] += (unsigned long long)n_final;
        atomicAdd(&F.work[0], (unsigned long long)n_final);
        atomicAdd(&F.work[3], (unsigned long long)n_final * (unsigned long long)m);
        atomicAdd(&W.info[0], (unsigned long long)n_final);
        atomicAdd(&W.info[3], (unsigned long long)cnt * (unsigned long long)m);
        if (!pend && at == end) fit_wide_epilogue(K, W, task, f_end);
    }
}

// which = 0: the mat-vec line (tiles of the learners with a pending mistake) -> mvbase; 1: the rank-1 line (16-row units of the
// learners that inserted) -> r1base.  One workgroup, as heavy_plan_kernel.
__global__ __launch_bounds__(1024) void fit_wide_plan_kernel(WideArgs A, int which) {
    __shared__ long long sc[1][1024];
    const FitWide& W = A.W;
    long long* base_out = which ? W.r1base : W.mvbase;
    long long carry = 0;
    for (int base = 0; base < A.nw; base += 1024) {
        const int slot = base + (int)threadIdx.x;
        long long w = 0;
        if (slot < A.nw) {
            if (which == 0 && W.pend[slot] == 1) {
                const long long nb = (A.F.K.m[A.F.task[W.list[slot]]] + 63) >> 6;
                w = nb * (nb + 1) / 2;
            }
            if (which == 1 && W.grew[slot] == 1) {
                const long long nb1 = (W.gm[slot] + 1 + 63) >> 6;
                w = nb1 * (nb1 + 1) / 2 * 4;
            }
        }
        long long incl[1] = {w};
        block_scan1024(incl, sc);
        if (slot < A.nw) base_out[slot] = carry + incl[0] - w;
        carry += sc[0][1023];
    }
    if (threadIdx.x == 0) base_out[A.nw] = carry;
}

__global__ __launch_bounds__(256, KB_MV_OCC) void fit_wide_matvec_kernel(WideArgs A) {
    __shared__ double slabs[4][8 * KB_SLAB_LD];
    const KbDev& D = A.F.D;
    const KbState& K = A.F.K;
    const FitWide& W = A.W;
    walk_stretch(W.mvbase, A.nw, [&](int slot, long long a, long long b) {
        const int dict = A.F.task[W.list[slot]];
        matvec_tri_tiles_lds(K, shells_of(D, K, dict), K.m[dict], (int)a, (int)b, slabs[threadIdx.x >> 6]);
    });
}

__global__ __launch_bounds__(256) void fit_wide_finish_kernel(WideArgs A) {
    const FitArgs& F = A.F;
    const KbDev& D = F.D;
    const KbState& K = F.K;
    const FitWide& W = A.W;
    __shared__ Lds sm;
    const int j = blockIdx.x;
    if (threadIdx.x == 0) W.grew[j] = 0;  // the previous round's rank-1 update has been made
    if (W.pend[j] != 1) return;
    const long long r = W.cur[j];
    const int task = F.task[W.list[j]], env = task / D.S, s = task - env * D.S;
    const uint64_t* sh = shells_of(D, K, task);
    const int d = D.dims[s] + 1;
    const int m = K.m[task];
    if (threadIdx.x < KB_DMAX) sm.x[threadIdx.x] = F.x[r * KB_DMAX + threadIdx.x];
    __syncthreads();
    matvec_tri_combine_wide(K, sh, m);
    const int y = (int)F.y[r];
    const double t_last = sm.x[d - 1];
    int branch = 0;
    double delta = 0.0;
    // Projectron++: apply_update_plus behind its mat-vec -- margin = y f of the f the decide kernel left for this sample; a mistake
    // continues as Projectron's, a sample inside the margin with the margin rule (branches 3, 4: no insertion, no shell, and a
    // version bump only when the coefficients move).  The rounds hold m >= 2, so neither meets the float32 regime.
    const double margin = F.alg == KB_ALG_PROJECTRON_PLUS ? (double)y * F.f[r] : 0.0;
    int m_new;
    if (margin <= 0.0)
        m_new = finish_update(D, K, task, env, m, d, sm.x, t_last, grid_index(t_last, D.n_prbs), y, sm, &branch, &delta, nullptr, true);
    else
        m_new = margin_update(D, K, sh, task, m, y, margin, sm, &branch, &delta);
    if (threadIdx.x == 0) {
        const unsigned long long grow = branch == 2 && m_new > m ? 1 : 0;
        const unsigned long long mist = branch >= 1 && branch <= 3 ? 1 : 0;  // a mistake changed the dictionary: not branch 4
        F.branch[r] = branch;
        F.delta[r] = delta;
        F.m_after[r] = m_new;
        K.m[task] = m_new;
        if (grow) {
            W.grew[j] = 1;
            W.gm[j] = m;
            W.gdelta[j] = delta;
        }
        W.pend[j] = 0;
        W.cur[j] = r + 1;
        K.stats[(size_t)task * 4 + 0] += 1;
        K.stats[(size_t)task * 4 + 1] += mist;
        K.stats[(size_t)task * 4 + 2] += grow;
        atomicAdd(&F.work[0], 1ull);
        if (mist) atomicAdd(&F.work[1], 1ull);
        if (grow) atomicAdd(&F.work[2], 1ull);
        atomicAdd(&F.work[3], (unsigned long long)m);
        const unsigned long long nb = (unsigned long long)((m + 63) >> 6);
        atomicAdd(&W.info[0], 1ull);
        atomicAdd(&W.info[1], 1ull);
        atomicAdd(&W.info[2], nb * (nb + 1) / 2);
        if (r + 1 == W.end[j]) fit_wide_epilogue(K, W, task, F.f[r]);
    }
}

__global__ __launch_bounds__(256) void fit_wide_rank1_kernel(WideArgs A) {
    const KbDev& D = A.F.D;
    const KbState& K = A.F.K;
    const FitWide& W = A.W;
    walk_stretch(W.r1base, A.nw, [&](int slot, long long u0, long long u1) {
        const int dict = A.F.task[W.list[slot]];
        rank1_units(K, shells_of(D, K, dict), W.gm[slot], W.gdelta[slot], D.tri, (int)u0, 1, (int)u1);
    });
}

}  // namespace kb

static int kb_fit_wide_window(const kb_handle* k) { return k->fit_wide_window ? k->fit_wide_window : KB_FIT_WINDOW; }

// the rounds' arrays, behind kb_fit's own in the call's staged block (kb_fit's layout function calls this)
static void kb_fit_wide_take(kb_handle* k, FitStage& st, int32_t n, kb::FitWide* W) {
    const size_t N = (size_t)n;
    W->mark = st.take<int32_t>(N);
    W->list = st.take<int32_t>(N);
    W->pend = st.take<int32_t>(N);
    W->grew = st.take<int32_t>(N);
    W->gm = st.take<int32_t>(N);
    W->hdr = st.take<int32_t>(4);
    W->cur = st.take<long long>(N + 1);
    W->end = st.take<long long>(N + 1);
    W->mvbase = st.take<long long>(N + 1);
    W->r1base = st.take<long long>(N + 1);
    W->gdelta = st.take<double>(N);
    W->wf = st.take<double>(N * (size_t)kb_fit_wide_window(k));
    W->min_m = k->fit_wide_min;
    W->window = kb_fit_wide_window(k);
}

// the rounds of one chunk, behind its classification and its launch of fit_kernel: until every wide learner has consumed its samples
static int kb_fit_wide_rounds(kb_handle* k, kb::WideArgs& wa, int32_t chunk) {
    kb_fit_state* p = k->fit;
    if (!p->h_wide) HIPCHK(k, hipHostMalloc((void**)&p->h_wide, 4 * sizeof(int32_t), hipHostMallocDefault));
    volatile int32_t* hdr = p->h_wide;  // (pinned: the copy is one small transfer on the stream, then one wait)
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(p->h_wide, wa.W.hdr, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    wa.nw = hdr[0];
    if (wa.nw <= 0) return RS_OK;
    const unsigned qblocks = (unsigned)((wa.W.window + KB_SCORE_Q - 1) / KB_SCORE_Q);
    for (int32_t rounds = 0; hdr[1] < wa.nw;) {
        if (rounds >= chunk) {  // (every round moves every pending learner at least one sample on: this cannot happen)
            k->err = "kb_fit: the chip-wide rounds of a chunk did not end within " + std::to_string(chunk) + " rounds (" +
                     std::to_string(wa.nw - hdr[1]) + " of " + std::to_string(wa.nw) + " learners pending)";
            return RS_EHIP;
        }
        const int32_t batch = std::min<int32_t>(KB_FIT_ROUNDS, chunk - rounds);
        hipEvent_t e;
        HIPCHK(k, p->fit_spans.begin(k->stream, 0, &e));
        for (int32_t b = 0; b < batch; ++b) {
            hipLaunchKernelGGL(kb::fit_wide_scan_kernel, dim3((unsigned)wa.nw, qblocks), dim3(256), 0, k->stream, wa);
            hipLaunchKernelGGL(kb::fit_wide_decide_kernel, dim3((unsigned)wa.nw), dim3(256), 0, k->stream, wa);
            hipLaunchKernelGGL(kb::fit_wide_plan_kernel, dim3(1), dim3(1024), 0, k->stream, wa, 0);
            hipLaunchKernelGGL(kb::fit_wide_matvec_kernel, dim3((unsigned)k->mv_grid), dim3(256), 0, k->stream, wa);
            hipLaunchKernelGGL(kb::fit_wide_finish_kernel, dim3((unsigned)wa.nw), dim3(256), 0, k->stream, wa);
            hipLaunchKernelGGL(kb::fit_wide_plan_kernel, dim3(1), dim3(1024), 0, k->stream, wa, 1);
            hipLaunchKernelGGL(kb::fit_wide_rank1_kernel, dim3((unsigned)k->r1_grid), dim3(256), 0, k->stream, wa);
        }
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        HIPCHK(k, hipGetLastError());
        HIPCHK(k, hipMemcpyAsync(p->h_wide, wa.W.hdr, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, k->stream));
        HIPCHK(k, hipStreamSynchronize(k->stream));
        rounds += batch;
    }
    return RS_OK;
}

/* Which learners kb_fit teaches by chip-wide rounds (ranslice.h): host state of the handle, like kb_set_algorithm. */
extern "C" int kb_set_fit_wide(kb_handle* k, int32_t min_landmarks, int32_t window) {
    if (!k) return RS_EINVAL;
    if (min_landmarks < 0 || min_landmarks == 1) {
        k->err = "kb_set_fit_wide: min_landmarks = " + std::to_string(min_landmarks) +
                 " (0 turns the wide path off, 2 or more turns it on; a single landmark's float32 regime stays in the narrow path)";
        return RS_EINVAL;
    }
    if (window < 0 || window > KB_FIT_WINDOW_MAX) {
        k->err = "kb_set_fit_wide: window = " + std::to_string(window) + " (0: the default, else 1 .. " + std::to_string(KB_FIT_WINDOW_MAX) + ")";
        return RS_EINVAL;
    }
    const int rc = kb_fit_wide_can_set(k, "kb_set_fit_wide");
    if (rc != RS_OK) return rc;
    k->fit_wide_min = min_landmarks;
    k->fit_wide_window = window;
    return RS_OK;
}

extern "C" int kb_get_fit_wide(kb_handle* k, int32_t* min_landmarks, int32_t* window) {
    if (!k || !min_landmarks || !window) return RS_EINVAL;
    *min_landmarks = k->fit_wide_min;
    *window = k->fit_wide_window;
    return RS_OK;
}

/* Whether the rounds also teach in Projectron++ mode (ranslice.h): host state of the handle, beside kb_set_fit_wide's.
   It has an effect only while the handle is in Projectron++ mode and kb_set_fit_wide's min_landmarks is 2 or more. */
extern "C" int kb_set_fit_wide_plus(kb_handle* k, int32_t on) {
    if (!k) return RS_EINVAL;
    if (on != 0 && on != 1) {
        k->err = "kb_set_fit_wide_plus: on = " + std::to_string(on) + " (0: Projectron++ keeps the narrow path, the default; 1: the rounds teach it too)";
        return RS_EINVAL;
    }
    const int rc = kb_fit_wide_can_set(k, "kb_set_fit_wide_plus");
    if (rc != RS_OK) return rc;
    k->fit_wide_plus = on;
    return RS_OK;
}

extern "C" int kb_get_fit_wide_plus(kb_handle* k, int32_t* on) {
    if (!k || !on) return RS_EINVAL;
    *on = k->fit_wide_plus;
    return RS_OK;
}

extern "C" int kb_fit_wide_info(kb_handle* k, uint64_t work[4]) {
    if (!k || !work) return RS_EINVAL;
    return kb_read_words(k, k->fit ? k->fit->d_work + 8 : nullptr, 4, work);
}
