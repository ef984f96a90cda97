// kb_shared_online_prune.hip -- the online budget of a shared-dictionary handle: kb_shared_prune's removal as the last stage of
// every shared learning step.  #included by rs_api.hip after kb_shared_prune.hip and kb_online_prune.hip: the
// rule's device functions and the storage policy KinvFull are kb_prune.hip's, the plan and downdate kernels
// (prune_shared_plan_kernel, prune_shared_downdate_kernel) kb_shared_prune.hip's, the list kernel, the argument block, the
// counters and the state behind a handle (kb_online_prune_state, k->oprune: a handle is of one storage for life, so the
// per-replica switch and this one never meet on it) kb_online_prune.hip's.
//
// kb_set_shared_online_prune(k, target, rounds): every shared learning step -- kb_shared_step, kb_shared_step_resident -- ends
// with a BUDGET STAGE, enqueued on the agent's stream behind the step's last round and in front of whatever reads the
// dictionaries next (in the resident step: the select that follows).  Every shared dictionary with m > target loses
// min(m - target, rounds) landmarks by the rule's seven steps and is then finished once as prune_shared_finish_kernel finishes
// it.  The host-driven rounds (kb_shared_scan / kb_shared_apply / kb_shared_commit) end a step only in the caller's eyes:
// kb_shared_online_prune_stage enqueues the stage there.
//
// The launches are kb_online_prune.hip's, the same whatever the dictionaries hold, and none waits for the host:
//   budget_list_kernel                         the dictionaries over the target, the stage's counters
//   shared_budget_round_kernel (choose)        steps 1-3 of the first removal
//   `rounds` times:
//     prune_shared_plan_kernel                 the downdate's work line (nb * nb * 4 units per active dictionary)
//     prune_shared_downdate_kernel             step 4 on both block triangles
//     shared_budget_round_kernel (move, then   steps 5-7, then steps 1-3 of the next removal -- or, behind the last round, the
//                                 choose/finish) finishing
// 2 + 3 * rounds launches.  A workgroup of shared_budget_round_kernel owns a list place for the whole stage (place li belongs to
// workgroup li % gridDim.x, and the grid is the number of dictionaries), so move, choose and finish of one dictionary are
// ordered by __syncthreads, and every barrier is met by the whole workgroup: prune_choose's and prune_move's branches are
// uniform over it, and so are the finishing's.
//
// The bits.  Choose and move are prune_choose<KinvFull, false> and prune_move<KinvFull>, the instances kb_shared_prune launches;
// no sum is formed: a dictionary comes out as kb_shared_prune(target) leaves it whenever `rounds` covers its excess.
//
// A dictionary the rule refuses (status 2: met in the stage's first removal, untouched; 3: stopped after the completed ones) is
// left as kb_shared_prune leaves it.  It serves every local replica, so every local replica's flag word gets the sticky
// KB_FLAG_PRUNE_REFUSED -- from stat[] in the finishing, so that prune_choose keeps its text.
//
// What kb_shared_prune_tail clears behind a shrink (d_cursor, d_cstar, d_counts, d_mcounts, d_taken) the stage leaves alone:
// every one of them is rewritten before it is read.  Round 0 of the scan takes its first candidate from the action, never from
// the cursor, and its thread 0 stores cstar and cursor of EVERY task (shared_scan_body: the early return is round > 0's);
// shared_merge_kernel stores mcounts[s] and taken[s] of every slice before apply and commit read them; d_counts is written by
// kb_shared_scan's collect kernel, by kb_shared_apply and by kb_shared_commit from the host's arrays, and the device-resident
// step does not read it.  So a stage that finds nothing over the target leaves every saved byte of the handle as it was.

namespace kb {

// prune_shared_finish_kernel's work for list place li, with the stage's counters (budget_finish's bookkeeping) and the flag words
__device__ __forceinline__ void shared_budget_finish(const BudgetArgs& b, int li, int& off) {
    const PruneArgs& a = b.p;
    const KbState& K = a.K;
    const int tid = threadIdx.x;
    const int n = a.removed[li], st = a.stat[li];
    const int dict = a.list[li];
    if (tid == 0) {
        if (st == 0 && K.m[dict] > a.target) atomicAdd(&b.work[2], 1ull);
        if ((st == 2 || st == 3) && atomicExch(&b.marked[dict], 1) == 0) atomicAdd(&b.work[4], 1ull);
    }
    if (st == 2 || st == 3)
        for (int e = tid; e < a.D.n_envs; e += 256) atomicOr(&K.err[e], KB_FLAG_PRUNE_REFUSED);  // (the dictionary serves them all)
    if (n == 0) return;  // (uniform: every thread read the same word)
    prune_chains(a, dict, off);
    for (int e = tid; e < a.D.n_envs; e += 256) {  // the tasks of the slice
        const size_t task = (size_t)e * a.D.S + dict;
        K.fver[task] = -1;
        K.f_last[task] = 0.0;
        K.m_last[task] = -1;
    }
    __syncthreads();
    if (tid == 0) {
        K.offgrid[dict] = off;
        K.ver[dict] += 1;
        K.kf_owner[dict] = -1;
        a.pruned[dict] += (long long)n;
        atomicAdd(&b.work[1], (unsigned long long)n);
    }
}

// budget_round_kernel on full storage: persistent workgroups over the device-side list
__global__ __launch_bounds__(256) void shared_budget_round_kernel(BudgetArgs b, int what) {
    __shared__ unsigned long long wkey[4];
    __shared__ int widx[4], wbad[4], off;
    const int count = (int)b.p.info[0];
    for (int li = blockIdx.x; li < count; li += gridDim.x) {
        if (what & KB_BUDGET_MOVE) {
            prune_move<KinvFull>(b.p, li);
            __syncthreads();
        }
        if (what & KB_BUDGET_CHOOSE) prune_choose<KinvFull, false>(b.p, li, wkey, widx, wbad);
        if (what & KB_BUDGET_FINISH) shared_budget_finish(b, li, off);
        __syncthreads();  // (the shared words are the next place's)
    }
}

}  // namespace kb

// the scratch arrays and the downdate's grid of a shared handle (kb_prune_prepare keeps the first kernel it is given: on a shared
// handle that is prune_shared_downdate_kernel, from here or from kb_shared_prune), then the stage's own state
static int kb_shared_online_prune_prepare(kb_handle* k) {
    const int rc = kb_prune_prepare(k, kb::prune_shared_downdate_kernel);
    return rc != RS_OK ? rc : kb_online_prune_prepare(k);
}

// the budget stage of a shared handle, on the agent's stream; nothing while the switch is off
static int launch_shared_online_prune(kb_handle* k) {
    kb_online_prune_state* p = k->oprune;
    if (!k->D.shared || !p || p->target == 0) return RS_OK;
    kb::BudgetArgs b;
    memset(&b, 0, sizeof b);
    b.p = kb_prune_args(k, p->target, p->d_info);
    const kb::PruneArgs& a = b.p;
    b.work = p->d_work;
    b.marked = p->d_marked;
    const dim3 grid((unsigned)p->grid), down((unsigned)k->prune->grid);
    hipLaunchKernelGGL(kb::budget_list_kernel, dim3(1), dim3(1024), 0, k->stream, b);
    hipLaunchKernelGGL(kb::shared_budget_round_kernel, grid, dim3(256), 0, k->stream, b, KB_BUDGET_CHOOSE);
    for (int r = 0; r < p->rounds; ++r) {
        hipLaunchKernelGGL(kb::prune_shared_plan_kernel, dim3(1), dim3(1024), 0, k->stream, a);
        hipLaunchKernelGGL(kb::prune_shared_downdate_kernel, down, dim3(256), 0, k->stream, a);
        hipLaunchKernelGGL(kb::shared_budget_round_kernel, grid, dim3(256), 0, k->stream, b,
                           KB_BUDGET_MOVE | (r + 1 < p->rounds ? KB_BUDGET_CHOOSE : KB_BUDGET_FINISH));
    }
    HIPCHK(k, hipGetLastError());
    k->gemm_fresh = false;  // (scores formed before the stage describe dictionaries that may be gone)
    return RS_OK;
}

extern "C" int kb_set_shared_online_prune(kb_handle* k, int32_t target, int32_t rounds) {
    if (!k) return RS_EINVAL;
    if (target != 0 && (target < KB_PRUNE_MIN || target > k->cfg.capacity - 1)) {
        k->err = "kb_set_shared_online_prune: target " + std::to_string(target) + " is neither 0 (off) nor in " +
                 std::to_string(KB_PRUNE_MIN) + " .. capacity - 1 = " + std::to_string(k->cfg.capacity - 1) +
                 " (a shared dictionary at its capacity projects: no headroom is needed)";
        return RS_EINVAL;
    }
    if (rounds < 1 || rounds > KB_ONLINE_ROUNDS_MAX) {
        k->err = "kb_set_shared_online_prune: rounds " + std::to_string(rounds) + " is outside 1 .. " + std::to_string(KB_ONLINE_ROUNDS_MAX);
        return RS_EINVAL;
    }
    if (!k->D.shared) {
        k->err = "kb_set_shared_online_prune: the handle is not a shared-dictionary handle (one agent per replica: kb_set_online_prune)";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_set_shared_online_prune: call kb_reset first";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_set_shared_online_prune: the handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    if (target != 0 || k->oprune) {  // (the scratch is allocated here, not at the first launch)
        const int rc = kb_shared_online_prune_prepare(k);
        if (rc != RS_OK) return rc;
    }
    if (k->oprune) {
        k->oprune->target = target;
        k->oprune->rounds = rounds;
    }
    return RS_OK;
}

extern "C" int kb_get_shared_online_prune(kb_handle* k, int32_t* target, int32_t* rounds) {
    if (!k || !target || !rounds) return RS_EINVAL;
    const bool set = k->D.shared && k->oprune;
    *target = set ? k->oprune->target : 0;
    *rounds = set ? k->oprune->rounds : 2;
    return RS_OK;
}

// kb_online_prune_info's words, for the stages of a shared handle
extern "C" int kb_shared_online_prune_info(kb_handle* k, uint64_t work[8]) {
    if (!k || !work) return RS_EINVAL;
    if (!k->D.shared) {
        k->err = "kb_shared_online_prune_info: the handle is not a shared-dictionary handle (one agent per replica: kb_online_prune_info)";
        return RS_ESTATE;
    }
    return kb_online_prune_words(k, work);
}

extern "C" int kb_shared_online_prune_stage(kb_handle* k) {
    if (!k) return RS_EINVAL;
    if (!k->D.shared) {
        k->err = "kb_shared_online_prune_stage: the handle is not a shared-dictionary handle (one agent per replica: kb_set_online_prune "
                 "runs its stage behind every update phase)";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_shared_online_prune_stage: call kb_reset first";
        return RS_ESTATE;
    }
    if (!k->oprune || k->oprune->target == 0) {
        k->err = "kb_shared_online_prune_stage: the switch is off: set a target with kb_set_shared_online_prune first";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_shared_online_prune_stage: the handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    HIPCHK(k, hipSetDevice(k->device));
    return launch_shared_online_prune(k);
}
