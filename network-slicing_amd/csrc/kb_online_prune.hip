// kb_online_prune.hip -- the online budget: kb_prune's removal rule as a stage of the closed loop.
// #included by rs_api.hip after kb_prune.hip: the rule's device functions (prune_list, prune_choose, prune_move, prune_chains), its
// argument block, its work line (prune_plan_kernel) and its downdate (prune_downdate_kernel: both already read the list's length
// from device memory and run at a geometry fixed by the handle) and its scratch arrays behind the handle are that file's.
//
// kb_set_online_prune(k, target, rounds): every update phase -- kb_update_control, kb_step_resident, kb_run_resident, plain or
// captured -- is followed by a BUDGET STAGE before anything else reads the dictionaries: every dictionary with m > target loses
// min(m - target, rounds) landmarks, each by the seven steps of kb_prune.hip's header in that operation order, and is then finished
// once as prune_finish_kernel finishes it.  What is left above the target is the next stage's (carry).
//
// Nothing in the stage waits for the host.  kb_prune reads the list's length (its grids) and the number of rounds back; here
// the list, the plan and the per-round status stay on the device, and the launches are the same whatever the dictionaries hold:
//   budget_list_kernel                   the dictionaries over the target, in increasing order (one workgroup), the stage's counters
//   budget_round_kernel (choose)         steps 1-3 of the first removal
//   `rounds` times:
//     prune_plan_kernel                  the downdate's work line over the dictionaries still active
//     prune_downdate_kernel              step 4
//     budget_round_kernel (move, then    steps 5-7, and in the same workgroup steps 1-3 of the dictionary's next removal -- or,
//                          choose/finish) behind the last round, the finishing of every listed dictionary
// 2 + 3 * rounds launches.  budget_round_kernel is a fixed grid of persistent workgroups that stride over the device-side list; a
// workgroup owns a dictionary for the whole call, so move, choose and finish of one dictionary are ordered by __syncthreads and
// different dictionaries share nothing.  A stage with nothing over the target finds the length 0 everywhere and returns at once.
//
// The bits.  Choose and move are kb_prune.hip's prune_choose and prune_move, called in a loop over the list; no sum is formed,
// so a dictionary comes out as kb_prune(target) leaves it whenever `rounds` covers its excess, whatever the launch, the grid
// or the other dictionaries.  (tests/test_gpu_online_prune.py holds the stage to that, and to tests/prune_mirror.py.)
//
// A dictionary whose Kinv diagonal is not finite and positive (or whose coefficient is not finite) is left as kb_prune leaves it --
// untouched when met in the stage's first removal, stopped after the completed ones otherwise -- and its replica gets the sticky
// bit KB_FLAG_PRUNE_REFUSED in its flag word (kb_get_flags): the loop cannot return RS_ESTATE from the device.

#define KB_ONLINE_ROUNDS_MAX 64
#define KB_BUDGET_CHOOSE 1
#define KB_BUDGET_MOVE 2
#define KB_BUDGET_FINISH 4

namespace kb {

struct BudgetArgs {
    PruneArgs p;               // p.info: [0] listed, [1] the largest excess of this stage, [5] / [6] prune_plan_kernel's counters
    unsigned long long* work;  // since kb_reset: [0] stages, [1] removals, [2] dictionary-stages left above the target, [3] the largest
                               // excess met, [4] dictionaries flagged (each once)
    int32_t* marked;           // [n_dict] 1: counted in work[4]
};

// prune_list, and the stage's counters
__global__ __launch_bounds__(1024) void budget_list_kernel(BudgetArgs b) {
    __shared__ int part[1024];
    __shared__ int most;
    prune_list(b.p, part, most);
    if (threadIdx.x == 0) {
        b.work[0] += 1ull;
        if ((unsigned long long)most > b.work[3]) b.work[3] = (unsigned long long)most;
    }
}

// prune_finish_kernel's work for list place li with the stage's counters: a dictionary still active and above the target is
// carried; one that met a bad entry is marked, once since kb_reset
__device__ __forceinline__ void budget_finish(const BudgetArgs& b, int li, int& off) {
    const PruneArgs& a = b.p;
    const KbState& K = a.K;
    const int tid = threadIdx.x;
    const int n = a.removed[li], st = a.stat[li];
    const int dict = a.list[li];
    if (tid == 0) {
        if (st == 0 && K.m[dict] > a.target) atomicAdd(&b.work[2], 1ull);
        if ((st == 2 || st == 3) && atomicExch(&b.marked[dict], 1) == 0) atomicAdd(&b.work[4], 1ull);
    }
    if (n == 0) return;
    prune_chains(a, dict, off);
    __syncthreads();
    if (tid == 0) {
        K.offgrid[dict] = off;
        K.ver[dict] += 1;
        K.fver[dict] = -1;   // (one agent per replica: dictionary = task)
        K.f_last[dict] = 0.0;
        K.m_last[dict] = -1;
        K.kf_owner[dict] = -1;
        a.pruned[dict] += (long long)n;
        atomicAdd(&b.work[1], (unsigned long long)n);
    }
}

// persistent workgroups over the list: place li belongs to workgroup li % gridDim.x in every launch of the stage, so what one
// launch's move wrote its choose (and the next launch's) reads from the same workgroup, behind a barrier
__global__ __launch_bounds__(256) void budget_round_kernel(BudgetArgs b, int what) {
    __shared__ unsigned long long wkey[4];
    __shared__ int widx[4], wbad[4], off;
    const int count = (int)b.p.info[0];
    for (int li = blockIdx.x; li < count; li += gridDim.x) {
        if (what & KB_BUDGET_MOVE) {
            prune_move<KinvTri>(b.p, li);
            __syncthreads();
        }
        if (what & KB_BUDGET_CHOOSE) prune_choose<KinvTri, true>(b.p, li, wkey, widx, wbad);
        if (what & KB_BUDGET_FINISH) budget_finish(b, li, off);
        __syncthreads();  // (the shared words are the next place's)
    }
}

}  // namespace kb

// What the switch keeps behind a handle, outside its saved regions (created when it is first set).  The list, victim, q, status,
// removed and base arrays and the pruned counters are k->prune's, shared with kb_prune: every kernel that touches them is enqueued
// on k->stream, each call and each stage begins with its own list kernel, and kb_prune_release runs only from kb_destroy, so a
// captured loop keeps valid pointers.  d_info stays apart: the stage counts its own units of the downdate (kb_online_prune_info).
struct kb_online_prune_state {
    int32_t target = 0, rounds = 2;
    int32_t* d_marked = nullptr;
    unsigned long long *d_info = nullptr, *d_work = nullptr;
    int grid = 1024;  // budget_round_kernel's persistent workgroups
};

static void kb_online_prune_release(kb_handle* k) {
    kb_online_prune_state* p = k->oprune;
    if (!p) return;
    void* ds[] = {p->d_marked, p->d_info, p->d_work};
    for (void* d : ds)
        if (d) (void)hipFree(d);
    delete p;
    k->oprune = nullptr;
}

// kb_reset, kb_load_state, kb_fork (into this handle): the counters start over with kb_prune's, on the handle's stream
static void kb_online_prune_restart(kb_handle* k) {
    kb_online_prune_state* p = k->oprune;
    if (!p || !p->d_work) return;
    (void)hipMemsetAsync(p->d_work, 0, sizeof(unsigned long long) * 8, k->stream);
    (void)hipMemsetAsync(p->d_info, 0, sizeof(unsigned long long) * 8, k->stream);
    (void)hipMemsetAsync(p->d_marked, 0, sizeof(int32_t) * (size_t)k->n_dict, k->stream);
}

static int kb_online_prune_prepare(kb_handle* k) {
    int rc = kb_prune_prepare(k, kb::prune_downdate_kernel);  // (the scratch arrays, the pruned counters, the downdate's grid)
    if (rc != RS_OK || k->oprune) return rc;
    kb_online_prune_state* p = new kb_online_prune_state();
    k->oprune = p;  // (kb_destroy frees whatever was allocated)
    const size_t nd = (size_t)k->n_dict;
    HIPCHK(k, hipMalloc((void**)&p->d_marked, sizeof(int32_t) * nd));
    HIPCHK(k, hipMalloc((void**)&p->d_info, sizeof(unsigned long long) * 8));
    HIPCHK(k, hipMalloc((void**)&p->d_work, sizeof(unsigned long long) * 8));
    HIPCHK(k, hipMemsetAsync(p->d_marked, 0, sizeof(int32_t) * nd, k->stream));
    HIPCHK(k, hipMemsetAsync(p->d_info, 0, sizeof(unsigned long long) * 8, k->stream));
    HIPCHK(k, hipMemsetAsync(p->d_work, 0, sizeof(unsigned long long) * 8, k->stream));
    p->grid = k->n_dict < 1024 ? k->n_dict : 1024;
    return RS_OK;
}

// the budget stage, on the agent's stream behind the update phase (launch_update_control has joined its side stream); nothing
// when the switch is off
static int launch_online_prune(kb_handle* k) {
    kb_online_prune_state* p = k->oprune;
    if (!p || p->target == 0 || k->D.shared) return RS_OK;  // (a shared handle's state is kb_set_shared_online_prune's)
    kb::BudgetArgs b;
    memset(&b, 0, sizeof b);
    b.p = kb_prune_args(k, p->target, p->d_info);
    const kb::PruneArgs& a = b.p;
    b.work = p->d_work;
    b.marked = p->d_marked;
    const dim3 grid((unsigned)p->grid), down((unsigned)k->prune->grid);
    hipLaunchKernelGGL(kb::budget_list_kernel, dim3(1), dim3(1024), 0, k->stream, b);
    hipLaunchKernelGGL(kb::budget_round_kernel, grid, dim3(256), 0, k->stream, b, KB_BUDGET_CHOOSE);
    for (int r = 0; r < p->rounds; ++r) {
        hipLaunchKernelGGL(kb::prune_plan_kernel, dim3(1), dim3(1024), 0, k->stream, a);
        hipLaunchKernelGGL(kb::prune_downdate_kernel, down, dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::budget_round_kernel, grid, dim3(256), 0, k->stream, b,
                           KB_BUDGET_MOVE | (r + 1 < p->rounds ? KB_BUDGET_CHOOSE : KB_BUDGET_FINISH));
    }
    HIPCHK(k, hipGetLastError());
    return RS_OK;
}

extern "C" int kb_set_online_prune(kb_handle* k, int32_t target, int32_t rounds) {
    if (!k) return RS_EINVAL;
    if (target != 0 && (target < KB_PRUNE_MIN || target > k->cfg.capacity - 64)) {
        k->err = "kb_set_online_prune: target " + std::to_string(target) + " is neither 0 (off) nor in " + std::to_string(KB_PRUNE_MIN) +
                 " .. capacity - 64 = " + std::to_string(k->cfg.capacity - 64) + " (one shell of headroom for a step's insertions)";
        return RS_EINVAL;
    }
    if (rounds < 1 || rounds > KB_ONLINE_ROUNDS_MAX) {
        k->err = "kb_set_online_prune: rounds " + std::to_string(rounds) + " is outside 1 .. " + std::to_string(KB_ONLINE_ROUNDS_MAX);
        return RS_EINVAL;
    }
    if (k->D.shared) {
        k->err = "kb_set_online_prune: shared-dictionary handles are not supported: prune them between steps with kb_shared_prune "
                 "(their own switch is kb_set_shared_online_prune)";
        return RS_ESTATE;
    }
    if (k->ref) {
        k->err = "kb_set_online_prune: a by-reference handle (kb_deploy_ref) shares read-only dictionaries and never learns: set the "
                 "budget on the learning handle and deploy again";
        return RS_ESTATE;
    }
    if (k->frozen) {
        k->err = "kb_set_online_prune: an inference-only handle (kb_deploy) holds no Kinv and never learns: set the budget on the "
                 "learning handle and deploy again";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_set_online_prune: call kb_reset first";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    if (target != 0 || k->oprune) {  // (here, not at the first launch: that may be inside a stream capture)
        const int rc = kb_online_prune_prepare(k);
        if (rc != RS_OK) return rc;
    }
    kb_online_prune_state* p = k->oprune;
    if (p && (p->target != target || p->rounds != rounds)) {  // (a captured loop carries the stage it was captured with)
        const int rc = kb_retire_graph(k);
        if (rc != RS_OK) return rc;
    }
    if (p) {
        p->target = target;
        p->rounds = rounds;
    }
    return RS_OK;
}

extern "C" int kb_get_online_prune(kb_handle* k, int32_t* target, int32_t* rounds) {
    if (!k || !target || !rounds) return RS_EINVAL;
    const bool set = k->oprune && !k->D.shared;  // (a shared handle's state is kb_set_shared_online_prune's: kb_shared_online_prune.hip)
    *target = set ? k->oprune->target : 0;
    *rounds = set ? k->oprune->rounds : 2;
    return RS_OK;
}

// since kb_reset: work[0] stages enqueued, [1] landmarks removed, [2] dictionary-stages left above the target (carry), [3] the
// largest excess a stage met, [4] dictionaries flagged, [5] the downdate's units that held rows (8 KB read + 8 KB written each);
// [6], [7] reserved
static int kb_online_prune_words(kb_handle* k, uint64_t work[8]) {
    const int rc = kb_read_words(k, k->oprune ? k->oprune->d_work : nullptr, 8, work);
    if (rc != RS_OK || !k->oprune) return rc;
    uint64_t info[8];
    const int rc2 = kb_read_words(k, k->oprune->d_info, 8, info);
    if (rc2 != RS_OK) return rc2;
    work[5] = info[5];
    work[6] = work[7] = 0;
    return RS_OK;
}

extern "C" int kb_online_prune_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    if (k->D.shared) {  // (never set here: the shared stages' counters are kb_shared_online_prune_info's)
        for (int q = 0; q < 8; ++q) work[q] = 0;
        return RS_OK;
    }
    return kb_online_prune_words(k, work);
}
