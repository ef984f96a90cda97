// kb_fit.hip -- the learner's own surface, batched: kb_fit teaches many learners their recorded sample sequences in one call,
// kb_score evaluates dictionaries on query sets without writing anything.  #included by rs_api.hip after kb_bridge.hip: it uses
// the agent handle and the Projectron routines of kb_kbrl.hip (predict_column, apply_update) and changes none of their kernels.
//
// kb_fit.  The sequence kb_predict(e, s, x_t); kb_update(e, s, x_t, y_t) over a learner's samples is sequentially dependent, so a
// LEARNER IS A WORKGROUP and the parallelism is across learners: fit_kernel runs one 256-thread workgroup per listed learner,
// persistent over the learner's samples of the launch.  Per sample it runs what the two one-sample kernels run, by the same
// functions on the same block size: predict_column (the kernel column into the K_f row, f), the decision (an exact tie with a
// populated dictionary draws from the learner's stream), the mistake test f y <= 0, apply_update.  Nothing in those functions
// depends on what ran before them in the same launch but the dictionary itself, which the one-sample kernels pass from launch to
// launch through the same global memory -- so every f, delta, coefficient and Kinv entry is bit for bit the one-by-one path's.
// (A dictionary of thousands of landmarks is taught at the pace of one workgroup here; kb_set_fit_wide hands such learners to
// chip-wide rounds, the heavy_* shape of update_control, with the same bits: kb_fit_wide.hip)  In Projectron++ mode (kb_set_algorithm) the same loop runs as its second
// instance, fit_plus_kernel: apply_update_plus in place of the mistake test and apply_update, as update_one_kernel does.
// The sample step is also stated as device functions, for kb_fit_steps.hip and kb_fit_wide.hip: fit_decide, fit_rule<ALG>,
// fit_epilogue.  The host framing of a fitting call stands once: kb_fit_can_learn, kb_fit_list, kb_fit_open / kb_fit_close, FitStage.
//
// kb_score.  f of kb_predict for many points, and nothing else: no K_f row, no cache, no counter, no tie draw.  score_kernel's
// workgroup takes one dictionary and KB_SCORE_Q of its queries, staged in LDS; thread t walks the landmarks j = t, t + 256, ...
// in increasing j, loads a landmark's coordinates and coefficient once and feeds Q accumulators with predict_column's
// operations in predict_column's order; each accumulator is then reduced as block_sum reduces.  A query's bits do not depend on
// the other queries of its block.  The kernel reads dictionaries through (KbDev, KbState) of whatever handle owns the pool, so it
// serves learning, copy-deployed, imported, by-reference (the store's pool) and shared-dictionary handles alike.

#include <algorithm>

namespace kb {

#define KB_SCORE_Q 8       // queries per workgroup of score_kernel: 8 distances + 8 sums in registers beside rs_exp's, no scratch
#define KB_FIT_CHUNK 256   // kb_fit's default: samples of one learner per launch

struct FitArgs {
    KbDev D;
    KbState K;
    const int32_t* task;       // [n]
    const long long* first;    // [n + 1] rows of learner i, relative to the staged block
    const double* x;           // [rows][KB_DMAX]
    const int8_t* y;           // [rows]
    long long from;            // this launch teaches rows first[i] + from .. first[i] + from + chunk - 1 of every learner
    int chunk;
    int32_t* y_pred;           // [rows] each
    double* f;
    int32_t* branch;
    double* delta;
    int32_t* m_after;
    unsigned long long* work;  // [0..3] samples, mistakes, insertions, kernel evaluations of the call
    int alg;                   // KB_ALG_* of the handle at the call: the instance kb_fit launches
    const int32_t* wide;       // [n] 1: the learner is taught this chunk by the rounds of kb_fit_wide.hip; NULL: the wide path is off
};

// ONE LEARNER'S SAMPLE STEP, shared by fit_steps_learner (kb_fit_steps.hip) and the chip-wide rounds (kb_fit_wide.hip): fit_decide,
// fit_rule and, when a learner is done with a launch, fit_epilogue.  All run on the whole 256-thread block.  They restate
// fit_learner's own step below statement for statement (a change there is made here too): built from these functions, fit_learner
// compiled to the same instructions under another register allocation, and fit_plus_kernel measured 0.4-0.6 % slower on a fleet of
// 20,480 learners, outside the parent's range (profiles/HISTORY.md) -- so fit_kernel and fit_plus_kernel keep the loop they had.

// Projectron.predict's decision (projectron.py:32-37) on the f just formed: its sign; an exact 0 against a populated dictionary
// draws from the learner's stream; an empty dictionary answers f = 0, y_pred = 0.  Every thread returns the same y_pred.
__device__ __forceinline__ int fit_decide(const KbState& K, int task, int env, int s, int m, double* f, Lds& sm) {
    int yp = 0;
    if (m > 0) {
        yp = *f > 0.0 ? 1 : (*f < 0.0 ? -1 : 0);
        if (yp == 0) {  // (block-uniform: every thread holds the same f)
            if (threadIdx.x == 0) sm.ired[0] = tie_draw(K, task, env, s);
            __syncthreads();
            yp = sm.ired[0];
            __syncthreads();
        }
    } else {
        *f = 0.0;
    }
    return yp;
}

// The update rule on the (f, K_f) just formed for the sample x (LDS) with label y.  Projectron.update (projectron.py:39-60): the
// mistake test f y <= 0, then apply_update.  ProjectronPlus.update (projectron.py:71-107): apply_update_plus on every sample; a
// mistake is a sample that changed the dictionary (branches 1-3).  Returns the new m; *branch and *delta as the rule leaves them
// (0, 0.0: no update); *mistakes and *insertions, the caller's counters, are advanced in place where the sample counts as one
// (returned as flags for the caller to add, they cost fit_steps_kernel two more moves per mistake).  ALG is a compile-time constant.
template <int ALG>
__device__ __forceinline__ int fit_rule(const KbDev& D, const KbState& K, int dict, int env, int m, int d, const double* x, int y, double f,
                                        Lds& sm, int* branch, double* delta, int* mistakes, int* insertions) {
    int m_new = m;
    *branch = 0;
    *delta = 0.0;
    if (ALG == KB_ALG_PROJECTRON_PLUS) {
        const double t_last = x[d - 1];
        m_new = apply_update_plus(D, K, dict, env, m, d, x, t_last, grid_index(t_last, D.n_prbs), y, f, sm, branch, delta);
        if (*branch >= 1 && *branch <= 3) *mistakes += 1;
        if (*branch == 2 && m_new > m) *insertions += 1;
    } else if (f * (double)y <= 0.0) {
        const double t_last = x[d - 1];
        m_new = apply_update(D, K, dict, env, m, d, x, t_last, grid_index(t_last, D.n_prbs), y, sm, branch, delta);
        *mistakes += 1;
        if (*branch == 2 && m_new > m) *insertions += 1;
    }
    return m_new;
}

struct FitCounts {  // what a launch counted for one learner
    unsigned long long samples, mistakes, insertions, evals;
};

// A learner is done with its samples of the launch (thread 0; per-replica dictionaries: task names the dictionary too).  `c` is NULL
// for the chip-wide rounds, which add their counters as they go.
__device__ __forceinline__ void fit_epilogue(const KbState& K, int task, double f, unsigned long long* work, const FitCounts* c) {
    K.f_last[task] = f;
    K.m_last[task] = -1;  // the cache of the last kb_predict is gone: kb_update answers RS_ESTATE until a new kb_predict
    K.kf_owner[task] = -1;
    if (!c) return;
    K.stats[(size_t)task * 4 + 0] += c->samples;
    K.stats[(size_t)task * 4 + 1] += c->mistakes;
    K.stats[(size_t)task * 4 + 2] += c->insertions;
    atomicAdd(&work[0], c->samples);
    atomicAdd(&work[1], c->mistakes);
    atomicAdd(&work[2], c->insertions);
    atomicAdd(&work[3], c->evals);
}

// The persistent loop of one learner, once per update rule: fit_kernel is the Projectron instance (ALG is a compile-time constant,
// so it holds none of the margin rule's code and its arithmetic is what it was before the rule existed), fit_plus_kernel the
// Projectron++ one -- apply_update_plus on every sample, which on a mistake runs apply_update's two steps.  The LDS block is
// declared by the kernels, as every kernel of kb_kbrl.hip declares its own.
template <int ALG>
__device__ __forceinline__ void fit_learner(const FitArgs& A, Lds& sm) {
    const KbDev& D = A.D;
    const KbState& K = A.K;
    const int i = blockIdx.x;
    const long long r0 = A.first[i] + A.from;
    const long long r1 = A.first[i + 1] < r0 + A.chunk ? A.first[i + 1] : r0 + A.chunk;
    if (r0 >= r1) return;
    if (A.wide && A.wide[i]) return;  // (kb_set_fit_wide: the rounds teach it this chunk)
    const int task = A.task[i], env = task / D.S, s = task - env * D.S;
    const int dt = task;  // (per-replica dictionaries only: kb_fit refuses shared ones)
    const uint64_t* sh = shells_of(D, K, dt);
    const int d = D.dims[s] + 1;
    int m = K.m[dt];
    unsigned long long n_mist = 0, n_grow = 0, n_eval = 0;
    double f = 0.0;
    for (long long r = r0; r < r1; ++r) {
        __syncthreads();  // (the previous sample's readers of sm.x are done)
        if (threadIdx.x < KB_DMAX) sm.x[threadIdx.x] = A.x[r * KB_DMAX + threadIdx.x];
        __syncthreads();
        // Projectron.predict (projectron.py:32-37)
        f = predict_column(D, K, sh, d, m, sm.x, sm);
        int yp = 0;
        if (m > 0) {
            yp = f > 0.0 ? 1 : (f < 0.0 ? -1 : 0);
            if (yp == 0) {  // (block-uniform: every thread holds the same f)
                if (threadIdx.x == 0) sm.ired[0] = tie_draw(K, task, env, s);
                __syncthreads();
                yp = sm.ired[0];
                __syncthreads();
            }
        } else {
            f = 0.0;
        }
        n_eval += (unsigned long long)m;
        // Projectron.update (projectron.py:39-60) on the (f, K_f) just formed
        const int y = (int)A.y[r];
        int branch = 0, m_new = m;
        double delta = 0.0;
        if (ALG == KB_ALG_PROJECTRON_PLUS) {
            // ProjectronPlus.update (projectron.py:71-107): a mistake is a sample that changed the dictionary (branches 1-3)
            const double t_last = sm.x[d - 1];
            m_new = apply_update_plus(D, K, dt, env, m, d, sm.x, t_last, grid_index(t_last, D.n_prbs), y, f, sm, &branch, &delta);
            if (branch >= 1 && branch <= 3) n_mist += 1;
            if (branch == 2 && m_new > m) n_grow += 1;
        } else if (f * (double)y <= 0.0) {
            const double t_last = sm.x[d - 1];
            m_new = apply_update(D, K, dt, env, m, d, sm.x, t_last, grid_index(t_last, D.n_prbs), y, sm, &branch, &delta);
            n_mist += 1;
            if (branch == 2 && m_new > m) n_grow += 1;
        }
        if (threadIdx.x == 0) {
            A.y_pred[r] = yp;
            A.f[r] = f;
            A.branch[r] = branch;
            A.delta[r] = delta;
            A.m_after[r] = m_new;
        }
        m = m_new;
    }
    if (threadIdx.x == 0) {
        K.m[dt] = m;
        K.f_last[task] = f;
        K.m_last[task] = -1;   // the cache of the last kb_predict is gone: kb_update answers RS_ESTATE until a new kb_predict
        K.kf_owner[dt] = -1;
        const unsigned long long ns = (unsigned long long)(r1 - r0);
        K.stats[(size_t)task * 4 + 0] += ns;
        K.stats[(size_t)task * 4 + 1] += n_mist;
        K.stats[(size_t)task * 4 + 2] += n_grow;
        atomicAdd(&A.work[0], ns);
        atomicAdd(&A.work[1], n_mist);
        atomicAdd(&A.work[2], n_grow);
        atomicAdd(&A.work[3], n_eval);
    }
}

__global__ __launch_bounds__(256) void fit_kernel(FitArgs A) {
    __shared__ Lds sm;
    fit_learner<KB_ALG_PROJECTRON>(A, sm);
}

__global__ __launch_bounds__(256) void fit_plus_kernel(FitArgs A) {
    __shared__ Lds sm;
    fit_learner<KB_ALG_PROJECTRON_PLUS>(A, sm);
}

// a workgroup of score_kernel: cnt <= KB_SCORE_Q consecutive queries (rows q0 .. of the staged block) against one dictionary
struct ScoreBlock {
    long long q0;
    int32_t dict, cnt;
};

struct ScoreArgs {
    KbDev D;   // of the handle whose pool holds the dictionaries (a by-reference handle: its store)
    KbState K;
    const ScoreBlock* blk;     // [gridDim.x]
    const double* x;           // [rows][KB_DMAX]
    double* f;                 // [rows]
    int32_t* y_pred;           // [rows]
    unsigned long long* work;  // [0] kernel evaluations of the call
};

// score_kernel's body: cnt <= KB_SCORE_Q queries (rows of 16 doubles from x on) against dictionary `dict`, f (and y_pred, unless
// NULL) written from f[0] / y_pred[0] on.  Returns the dictionary's size.  The LDS blocks are the calling kernel's.  Also the window
// scan of kb_fit's chip-wide rounds (kb_fit_wide.hip).
__device__ __forceinline__ int score_queries(const KbDev& D, const KbState& K, int dict, int cnt, const double* x, double* f_out,
                                             int32_t* y_pred, double (&xs)[KB_SCORE_Q][KB_DMAX], double (&red)[KB_SCORE_Q][4],
                                             double (&k1)[KB_SCORE_Q]) {
    const int s = dict % D.S, d = D.dims[s] + 1;
    const uint64_t* sh = shells_of(D, K, dict);
    const int m = K.m[dict];
    if (threadIdx.x < KB_SCORE_Q * KB_DMAX) {
        const int u = threadIdx.x / KB_DMAX, c = threadIdx.x - u * KB_DMAX;
        xs[u][c] = u < cnt ? x[u * KB_DMAX + c] : 0.0;
    }
    __syncthreads();
    double acc[KB_SCORE_Q];
#pragma unroll
    for (int u = 0; u < KB_SCORE_Q; ++u) acc[u] = 0.0;
    for (int j = threadIdx.x; j < m; j += 256) {
        const double* P = vec_page(K, sh, j >> 6);
        const int l = j & 63;
        const double co = P[KB_ROW_CO * KB_CH + l];
        double dist[KB_SCORE_Q];
#pragma unroll
        for (int u = 0; u < KB_SCORE_Q; ++u) dist[u] = 0.0;
        for (int q = 0; q < d; ++q) {
            const double v = P[q * KB_CH + l];
#pragma unroll
            for (int u = 0; u < KB_SCORE_Q; ++u) {
                const double t = v - xs[u][q];
                dist[u] += t * t;
            }
        }
#pragma unroll
        for (int u = 0; u < KB_SCORE_Q; ++u) {
            if (u < cnt) {  // (block-uniform)
                double k = rs_exp(-D.gamma * dist[u]);
                if (m == 1) {
                    k = (double)(float)k;
                    k1[u] = k;  // (thread 0 alone is here)
                }
                acc[u] += k * co;
            }
        }
    }
    // block_sum, per query: the butterfly per wave, the four wave totals in order
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int u = 0; u < KB_SCORE_Q; ++u) {
        double v = acc[u];
        for (int dd = 32; dd >= 1; dd >>= 1) v += __shfl_xor(v, dd);
        if (lane == 0) red[u][wv] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < cnt) {
        const int u = threadIdx.x;
        double f = 0.0;
        for (int w = 0; w < 4; ++w) f += red[u][w];
        if (m == 1) f = (double)(float)((float)k1[u] * (float)*vec_at(K, sh, KB_ROW_CO, 0));
        if (m == 0) f = 0.0;
        f_out[u] = f;
        if (y_pred) y_pred[u] = m > 0 ? (f > 0.0 ? 1 : (f < 0.0 ? -1 : 0)) : 0;
    }
    return m;
}

__global__ __launch_bounds__(256) void score_kernel(ScoreArgs A) {
    __shared__ double xs[KB_SCORE_Q][KB_DMAX];
    __shared__ double red[KB_SCORE_Q][4];
    __shared__ double k1[KB_SCORE_Q];  // the kernel value of the only landmark (m == 1), as the K_f row would hold it
    const ScoreBlock B = A.blk[blockIdx.x];
    const int m = score_queries(A.D, A.K, B.dict, B.cnt, A.x + B.q0 * KB_DMAX, A.f + B.q0, A.y_pred + B.q0, xs, red, k1);
    if (threadIdx.x == 0) atomicAdd(&A.work[0], (unsigned long long)m * (unsigned long long)B.cnt);
}

// The state of kb_fit's chip-wide rounds (kb_fit_wide.hip), in the call's staged block; rebuilt by every chunk's
// classification.  By listed learner: mark.  By slot of the chunk's list of wide learners: everything else.
struct FitWide {
    int32_t* mark;       // [n] 1: taught by the rounds this chunk (fit_learner returns at once)
    int32_t* hdr;        // [4]: wide learners of the chunk, how many of them have consumed their samples, -, -
    int32_t* list;       // [n] slot -> listed learner
    long long* cur;      // [n] the next row to decide; with pend: the mistaken row, whose kernel column is in the K_f row
    long long* end;      // [n] one past the learner's last row of the chunk
    int32_t* pend;       // [n] 1: a mistake (Projectron++: or a sample inside the margin) waits for its mat-vec and finish
    int32_t* grew;       // [n] 1: the round's update inserted: Kinv still needs its rank-1 update
    int32_t* gm;         // [n] dictionary size before that insertion
    double* gdelta;      // [n] its delta
    long long* mvbase;   // [n + 1] prefix sums of the mat-vec work (tiles) of the learners with a pending mistake
    long long* r1base;   // [n + 1] prefix sums of the rank-1 work (16-row units) of the learners that inserted
    double* wf;          // [n][window] the scores of the window scan
    unsigned long long* info;  // [4] kb_fit_wide_info
    int32_t min_m, window;
};

struct WideArgs {
    FitArgs F;
    FitWide W;
    int32_t n, nw;  // listed learners; wide learners of the chunk (0 until the host has read it: the classification)
};

__global__ __launch_bounds__(1024) void fit_wide_classify_kernel(WideArgs A);  // kb_fit_wide.hip

}  // namespace kb

// what kb_fit / kb_score keep on the handle: the counters of the last calls and their kernel timing
struct kb_fit_state {
    unsigned long long* d_work = nullptr;  // [12]: [8..11] the last kb_fit's kb_fit_wide_info; [0..3] the last kb_fit's samples, mistakes, insertions, kernel evaluations; [4] the last kb_score's
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    int32_t* h_wide = nullptr;             // pinned [4]: where the rounds' "wide learners, done" words are copied for the host (kb_fit_wide.hip)
    EventSpans fit_spans, score_spans;     // a pair per launch of the last call, when kernel timing was on at the call
    double fit_ms = 0.0, score_ms = 0.0;   // their sums, once drained (kb_fit_time_ms)
};

static void kb_fit_release(kb_handle* k) {
    kb_fit_state* p = k->fit;
    if (!p) return;
    if (p->d_work) (void)hipFree(p->d_work);
    if (p->ev_in) (void)hipEventDestroy(p->ev_in);
    if (p->ev_out) (void)hipEventDestroy(p->ev_out);
    if (p->h_wide) (void)hipHostFree(p->h_wide);
    p->fit_spans.release();
    p->score_spans.release();
    delete p;
    k->fit = nullptr;
}

static int kb_fit_prepare(kb_handle* k) {
    if (k->fit) return RS_OK;
    kb_fit_state* p = new kb_fit_state();
    k->fit = p;  // (kb_destroy frees whatever was allocated)
    HIPCHK(k, hipMalloc((void**)&p->d_work, sizeof(unsigned long long) * 12));
    HIPCHK(k, hipMemsetAsync(p->d_work, 0, sizeof(unsigned long long) * 12, k->stream));
    return RS_OK;
}

// One device block for a call's staged arrays, released when the call returns.  The call states its arrays ONCE, as a function of
// take() calls (256-byte boundaries, in their order): alloc runs it without a block, to count the bytes, and again on the block.
struct FitStage {
    char* base = nullptr;
    size_t used = 0;
    ~FitStage() {
        if (base) (void)hipFree(base);
    }
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    template <class Tp>
    Tp* take(size_t n) {
        Tp* p = base ? (Tp*)(base + used) : nullptr;
        used += pad(sizeof(Tp) * (n ? n : 1));
        return p;
    }
    template <class Layout>
    hipError_t alloc(Layout layout) {
        layout(*this);
        const hipError_t e = hipMalloc((void**)&base, used);
        if (e != hipSuccess) return e;
        used = 0;
        layout(*this);
        return hipSuccess;
    }
};

// kb_fit's chip-wide rounds (kb_fit_wide.hip): their state's arrays in the staged block, and the rounds of one chunk
static void kb_fit_wide_take(kb_handle* k, FitStage& st, int32_t n, kb::FitWide* W);
static int kb_fit_wide_rounds(kb_handle* k, kb::WideArgs& wa, int32_t chunk);

// the handles that cannot be taught, for kb_fit and kb_fit_steps (`who`)
static int kb_fit_can_learn(kb_handle* k, const char* who) {
    if (k->ref) {
        k->err = std::string(who) + ": a by-reference handle (kb_deploy_ref) shares read-only dictionaries: it cannot learn";
        return RS_ESTATE;
    }
    if (k->frozen) {
        k->err = std::string(who) + ": an inference-only handle (kb_deploy, kb_import_agents) cannot learn: it holds no Kinv";
        return RS_ESTATE;
    }
    if (k->D.shared) {
        k->err = std::string(who) + ": shared-dictionary handles are not supported: several learners map to one dictionary";
        return RS_ESTATE;
    }
    return RS_OK;
}

// and for the settings of the chip-wide rounds (kb_set_fit_wide, kb_set_fit_wide_plus)
static int kb_fit_wide_can_set(kb_handle* k, const char* who) { return kb_refuse_non_learning(k, who, "kb_fit"); }

// the list of a fitting call: every entry of `array` names one of `limit` learners / agents (`noun`), none twice (`seq`: its samples / rows)
static int kb_fit_list(kb_handle* k, const char* who, const char* array, const char* noun, const char* seq, const int32_t* list,
                       int32_t n, int32_t limit) {
    std::vector<char> seen((size_t)limit, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (list[i] < 0 || list[i] >= limit) {
            k->err = std::string(who) + ": " + array + "[" + std::to_string(i) + "] = " + std::to_string(list[i]) + " names no " + noun +
                     " (0 .. " + std::to_string(limit - 1) + ")";
            return RS_EINVAL;
        }
        if (seen[(size_t)list[i]]) {
            k->err = std::string(who) + ": " + noun + " " + std::to_string(list[i]) + " is listed twice: " +
                     (strchr("aeiou", noun[0]) ? "an " : "a ") + noun + "'s " + seq + " form ONE sequence";
            return RS_EINVAL;
        }
        seen[(size_t)list[i]] = 1;
    }
    return RS_OK;
}

// a fitting call opens behind whatever is queued on either stream, its counters and timing restarted; it closes with the side stream behind it
static int kb_fit_open(kb_handle* k) {
    int rc;
    HIPCHK(k, hipSetDevice(k->device));
    if ((rc = kb_fit_prepare(k)) != RS_OK) return rc;
    kb_fit_state* p = k->fit;
    k->gemm_fresh = false;
    if (k->side && (rc = stream_after(k, &p->ev_in, k->side, k->stream)) != RS_OK) return rc;
    HIPCHK(k, hipMemsetAsync(p->d_work, 0, sizeof(unsigned long long) * 4, k->stream));
    p->fit_spans.on = k->spans.on;
    p->fit_spans.reset();
    p->fit_ms = 0.0;
    return RS_OK;
}

static int kb_fit_close(kb_handle* k) {
    int rc;
    if (k->side && (rc = stream_after(k, &k->fit->ev_out, k->stream, k->side)) != RS_OK) return rc;
    return kb_check(k);  // (waits for the stream)
}

// the checks kb_fit and kb_score share: the sample ranges.  *rows = first[n] - first[0]
static int kb_fit_ranges(kb_handle* k, const char* who, const int64_t* first, int32_t n, int64_t* rows) {
    if (first[0] < 0) {
        k->err = std::string(who) + ": first[0] is negative";
        return RS_EINVAL;
    }
    for (int32_t i = 0; i < n; ++i)
        if (first[i + 1] < first[i]) {
            k->err = std::string(who) + ": first[] must not decrease (first[" + std::to_string(i + 1) + "] < first[" + std::to_string(i) + "])";
            return RS_EINVAL;
        }
    *rows = first[n] - first[0];
    return RS_OK;
}

extern "C" int kb_fit(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, const int8_t* y,
                      int32_t chunk, int32_t* y_pred, double* f, int32_t* branch, double* delta, int32_t* m_after) {
    if (!k) return RS_EINVAL;
    if (!k->is_reset) {
        k->err = "kb_fit: call kb_reset first";
        return RS_ESTATE;
    }
    int rc = kb_fit_can_learn(k, "kb_fit");
    if (rc != RS_OK) return rc;
    if (n < 0 || chunk < 0 || (n > 0 && (!task || !first))) {
        k->err = "kb_fit: n or chunk is negative, or task / first is NULL";
        return RS_EINVAL;
    }
    if (n == 0) return RS_OK;
    if ((rc = kb_fit_list(k, "kb_fit", "task", "learner", "samples", task, n, k->T)) != RS_OK) return rc;
    int64_t rows = 0;
    if ((rc = kb_fit_ranges(k, "kb_fit", first, n, &rows)) != RS_OK) return rc;
    if (rows == 0) return RS_OK;
    if (!x || !y) {
        k->err = "kb_fit: x or y is NULL";
        return RS_EINVAL;
    }
    const int64_t base = first[0];
    int64_t longest = 0;
    for (int32_t i = 0; i < n; ++i) longest = std::max<int64_t>(longest, first[i + 1] - first[i]);
    for (int64_t r = 0; r < rows; ++r)
        if (y[base + r] != 1 && y[base + r] != -1) {
            k->err = "kb_fit: y[" + std::to_string(base + r) + "] = " + std::to_string((int)y[base + r]) + " is neither +1 nor -1";
            return RS_EINVAL;
        }
    if (chunk == 0) chunk = KB_FIT_CHUNK;
    if ((rc = kb_fit_open(k)) != RS_OK) return rc;
    kb_fit_state* p = k->fit;
    HIPCHK(k, hipMemsetAsync(p->d_work + 8, 0, sizeof(unsigned long long) * 4, k->stream));  // (kb_fit_wide_info: of this call)
    std::vector<long long> rel((size_t)n + 1);
    for (int32_t i = 0; i <= n; ++i) rel[(size_t)i] = (long long)(first[i] - base);
    const size_t R = (size_t)rows;
    // kb_set_fit_wide: learners with large dictionaries are taught chunk by chunk in chip-wide rounds (kb_fit_wide.hip); Projectron++
    // keeps the one-workgroup loop whatever that setting, unless kb_set_fit_wide_plus is on as well
    const bool wide = k->fit_wide_min >= 2 && (k->alg != KB_ALG_PROJECTRON_PLUS || k->fit_wide_plus);
    kb::FitArgs a;
    memset(&a, 0, sizeof a);
    a.D = k->D;
    a.K = k->K;
    a.chunk = chunk;
    a.work = p->d_work;
    a.alg = k->alg;
    kb::WideArgs wa;
    memset(&wa, 0, sizeof wa);
    int32_t* d_task = nullptr;
    long long* d_first = nullptr;
    double* d_x = nullptr;
    int8_t* d_y = nullptr;
    FitStage st;
    HIPCHK(k, st.alloc([&](FitStage& s) {
        a.task = d_task = s.take<int32_t>((size_t)n);
        a.first = d_first = s.take<long long>((size_t)n + 1);
        a.x = d_x = s.take<double>(KB_DMAX * R);
        a.y = d_y = s.take<int8_t>(R);
        a.y_pred = s.take<int32_t>(R);
        a.branch = s.take<int32_t>(R);
        a.m_after = s.take<int32_t>(R);
        a.f = s.take<double>(R);
        a.delta = s.take<double>(R);
        if (wide) kb_fit_wide_take(k, s, n, &wa.W);
    }));
    if (wide) {
        wa.W.info = p->d_work + 8;
        wa.n = n;
        a.wide = wa.W.mark;
    }
    HIPCHK(k, hipMemcpyAsync(d_task, task, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_first, rel.data(), sizeof(long long) * ((size_t)n + 1), hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_x, x + (size_t)base * KB_DMAX, sizeof(double) * KB_DMAX * R, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_y, y + base, R, hipMemcpyHostToDevice, k->stream));
    for (int64_t from = 0; from < longest; from += chunk) {  // (no launch runs longer than `chunk` samples of one learner)
        a.from = (long long)from;
        hipEvent_t e;
        HIPCHK(k, p->fit_spans.begin(k->stream, 0, &e));
        if (wide) {  // which of the listed learners the rounds teach this chunk: decided on the device, from K.m
            wa.F = a;
            hipLaunchKernelGGL(kb::fit_wide_classify_kernel, dim3(1), dim3(1024), 0, k->stream, wa);
        }
        if (a.alg == KB_ALG_PROJECTRON_PLUS)
            hipLaunchKernelGGL(kb::fit_plus_kernel, dim3((unsigned)n), dim3(256), 0, k->stream, a);
        else
            hipLaunchKernelGGL(kb::fit_kernel, dim3((unsigned)n), dim3(256), 0, k->stream, a);
        if (e) HIPCHK(k, hipEventRecord(e, k->stream));
        if (wide && (rc = kb_fit_wide_rounds(k, wa, chunk)) != RS_OK) return rc;
    }
    HIPCHK(k, hipGetLastError());
    if (y_pred) HIPCHK(k, hipMemcpyAsync(y_pred + base, a.y_pred, sizeof(int32_t) * R, hipMemcpyDeviceToHost, k->stream));
    if (f) HIPCHK(k, hipMemcpyAsync(f + base, a.f, sizeof(double) * R, hipMemcpyDeviceToHost, k->stream));
    if (branch) HIPCHK(k, hipMemcpyAsync(branch + base, a.branch, sizeof(int32_t) * R, hipMemcpyDeviceToHost, k->stream));
    if (delta) HIPCHK(k, hipMemcpyAsync(delta + base, a.delta, sizeof(double) * R, hipMemcpyDeviceToHost, k->stream));
    if (m_after) HIPCHK(k, hipMemcpyAsync(m_after + base, a.m_after, sizeof(int32_t) * R, hipMemcpyDeviceToHost, k->stream));
    return kb_fit_close(k);
}

extern "C" int kb_score(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, double* f,
                        int32_t* y_pred) {
    if (!k) return RS_EINVAL;
    if (!k->is_reset) {
        k->err = "kb_score: call kb_reset first";
        return RS_ESTATE;
    }
    if (n < 0 || (n > 0 && (!task || !first))) {
        k->err = "kb_score: n is negative, or task / first is NULL";
        return RS_EINVAL;
    }
    if (n == 0) return RS_OK;
    for (int32_t i = 0; i < n; ++i)
        if (task[i] < 0 || task[i] >= k->T) {
            k->err = "kb_score: task[" + std::to_string(i) + "] = " + std::to_string(task[i]) + " names no learner (0 .. " + std::to_string(k->T - 1) + ")";
            return RS_EINVAL;
        }
    int64_t rows = 0;
    int rc = kb_fit_ranges(k, "kb_score", first, n, &rows);
    if (rc != RS_OK) return rc;
    if (rows == 0) return RS_OK;
    if (!x || !f) {
        k->err = "kb_score: x or f is NULL";
        return RS_EINVAL;
    }
    const int64_t base = first[0];
    kb_handle* own = k->ref ? kb_ref_store(k) : k;  // the handle whose pool holds the dictionaries
    // the prefix table of query blocks: a learner's queries in blocks of KB_SCORE_Q, the last one ragged
    std::vector<kb::ScoreBlock> blocks;
    for (int32_t i = 0; i < n; ++i) {
        const int dict = k->ref ? kb_ref_dict(k, (size_t)task[i]) : (k->D.shared ? task[i] % k->cfg.n_slices : task[i]);
        for (int64_t q = first[i]; q < first[i + 1]; q += KB_SCORE_Q) {
            kb::ScoreBlock b;
            b.q0 = (long long)(q - base);
            b.dict = dict;
            b.cnt = (int32_t)std::min<int64_t>(KB_SCORE_Q, first[i + 1] - q);
            blocks.push_back(b);
        }
    }
    HIPCHK(k, hipSetDevice(k->device));
    if ((rc = kb_fit_prepare(k)) != RS_OK) return rc;
    kb_fit_state* p = k->fit;
    const size_t R = (size_t)rows, NB = blocks.size();
    kb::ScoreArgs a;
    memset(&a, 0, sizeof a);
    a.D = own->D;
    a.K = own->K;
    a.work = p->d_work + 4;
    kb::ScoreBlock* d_blk = nullptr;
    double* d_x = nullptr;
    FitStage st;
    HIPCHK(k, st.alloc([&](FitStage& s) {
        a.blk = d_blk = s.take<kb::ScoreBlock>(NB);
        a.x = d_x = s.take<double>(KB_DMAX * R);
        a.f = s.take<double>(R);
        a.y_pred = s.take<int32_t>(R);
    }));
    if (k->side && (rc = stream_after(k, &p->ev_in, k->side, k->stream)) != RS_OK) return rc;
    HIPCHK(k, hipMemcpyAsync(d_blk, blocks.data(), sizeof(kb::ScoreBlock) * NB, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemcpyAsync(d_x, x + (size_t)base * KB_DMAX, sizeof(double) * KB_DMAX * R, hipMemcpyHostToDevice, k->stream));
    HIPCHK(k, hipMemsetAsync(p->d_work + 4, 0, sizeof(unsigned long long), k->stream));
    p->score_spans.on = k->spans.on;
    p->score_spans.reset();
    p->score_ms = 0.0;
    hipEvent_t e;
    HIPCHK(k, p->score_spans.begin(k->stream, 1, &e));
    hipLaunchKernelGGL(kb::score_kernel, dim3((unsigned)NB), dim3(256), 0, k->stream, a);
    if (e) HIPCHK(k, hipEventRecord(e, k->stream));
    HIPCHK(k, hipGetLastError());
    HIPCHK(k, hipMemcpyAsync(f + base, a.f, sizeof(double) * R, hipMemcpyDeviceToHost, k->stream));
    if (y_pred) HIPCHK(k, hipMemcpyAsync(y_pred + base, a.y_pred, sizeof(int32_t) * R, hipMemcpyDeviceToHost, k->stream));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    return RS_OK;
}

extern "C" int kb_fit_time_ms(kb_handle* k, double ms[2], uint64_t work[4]) {
    if (!k || !ms || !work) return RS_EINVAL;
    ms[0] = ms[1] = 0.0;
    for (int q = 0; q < 4; ++q) work[q] = 0;
    kb_fit_state* p = k->fit;
    if (!p) return RS_OK;
    HIPCHK(k, hipSetDevice(k->device));
    HIPCHK(k, hipStreamSynchronize(k->stream));
    HIPCHK(k, p->fit_spans.drain([&](int, double t) { p->fit_ms += t; }));
    HIPCHK(k, p->score_spans.drain([&](int, double t) { p->score_ms += t; }));
    ms[0] = p->fit_ms;
    ms[1] = p->score_ms;
    uint64_t w[8];
    const int rc = kb_read_words(k, p->d_work, 8, w);
    if (rc != RS_OK) return rc;
    work[0] = w[0];
    work[1] = w[1];
    work[2] = w[2];
    work[3] = w[3] + w[4];
    return RS_OK;
}
