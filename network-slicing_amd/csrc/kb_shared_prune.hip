// kb_shared_prune.hip -- budgeted shared dictionaries: kb_shared_prune is kb_prune's removal (kb_prune.hip) on
// the storage a shared-dictionary handle has.  #included by rs_api.hip after kb_prune.hip: the rule's device
// functions, the list kernel, the state behind a handle and the host sequence are that file's.
//
// A shared dictionary keeps BOTH block triangles of Kinv, each the exact transpose of the other; what the rule does differently
// there is the storage policy KinvFull (kb_prune.hip), and the kernels below are its instances.  The operation order is the
// rule's, nothing is summed: one dictionary comes out, bit for bit, as kb_prune leaves its unshared copy (kb_unshare) --
// landmarks, slots, coefficients and the lower block triangle -- and the upper triangle as the lower one's transpose.  The work
// line holds nb * nb * 4 units of sixteen rows per dictionary instead of the triangle's nb (nb + 1) / 2 * 4.
// What is this file's own: prune_shared_finish_kernel -- one dictionary serves the n_envs tasks of its slice, and the cached
// predict of every one of them is invalidated, where prune_finish_kernel has dictionary = task -- and, on the host, the refusals
// and what the shared mode derives from a dictionary.
// Nothing depends on the rank of a handle or on its communicator: ranks that call kb_shared_prune with the same target at the
// same step of a run keep bit-identical dictionaries without a collective.

namespace kb {

__global__ __launch_bounds__(256) void prune_shared_choose_kernel(PruneArgs a) {
    __shared__ unsigned long long wkey[4];
    __shared__ int widx[4], wbad[4];
    prune_choose<KinvFull, false>(a, blockIdx.x, wkey, widx, wbad);
}

__global__ __launch_bounds__(1024) void prune_shared_plan_kernel(PruneArgs a) {
    __shared__ long long sc[1][1024];
    __shared__ unsigned long long filled;
    prune_plan<KinvFull>(a, sc, filled);
}

__global__ __launch_bounds__(256) void prune_shared_downdate_kernel(PruneArgs a) { prune_downdate<KinvFull>(a); }

__global__ __launch_bounds__(256) void prune_shared_move_kernel(PruneArgs a) { prune_move<KinvFull>(a, blockIdx.x); }

// Once per listed dictionary, after the rounds: prune_finish_kernel's chains, off-grid count (it decides gemm_applies: a
// dictionary whose last off-grid landmark left is scored on the wide path again), version and counters.  A shared dictionary is
// read by the n_envs tasks (replica, slice) of its slice: the cached predict of every one of them goes, and the K_f row
// belongs to nobody.
__global__ __launch_bounds__(256) void prune_shared_finish_kernel(PruneArgs a) {
    __shared__ int off;
    const KbState& K = a.K;
    const int li = blockIdx.x, tid = threadIdx.x;
    const int n = a.removed[li], st = a.stat[li];
    if (tid == 0 && st == 2) atomicAdd(&a.info[2], 1ull);
    if (tid == 0 && st == 3) atomicAdd(&a.info[4], 1ull);
    if (n == 0) return;
    const int dict = a.list[li];
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
        atomicAdd(&a.info[3], (unsigned long long)n);
    }
}

}  // namespace kb

// What the shared mode derives from a dictionary is rebuilt by the next step, as after kb_share: Q (workq) by every launch of
// the scoring product, F / E by it once gemm_fresh is off; the proposal cursors of an earlier round name candidates scored
// against dictionaries that are gone.  Shells, flag words and the communicator stay as they are.
static int kb_shared_prune_tail(kb_handle* k) {
    const size_t T = (size_t)k->T, S = (size_t)k->cfg.n_slices;
    HIPCHK(k, hipMemsetAsync(k->d_cursor, 0xFF, sizeof(int32_t) * T, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_cstar, 0xFF, sizeof(int32_t) * T, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_counts, 0, sizeof(int32_t) * S, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_mcounts, 0, sizeof(int32_t) * S, k->stream));
    HIPCHK(k, hipMemsetAsync(k->d_taken, 0, sizeof(int32_t) * S, k->stream));
    return RS_OK;
}

extern "C" int kb_shared_prune(kb_handle* k, int32_t target, uint64_t* removed_total) {
    if (!k) return RS_EINVAL;
    if (removed_total) *removed_total = 0;
    const int rc = kb_prune_target_ok(k, "kb_shared_prune", target);
    if (rc != RS_OK) return rc;
    if (!k->D.shared) {
        k->err = "kb_shared_prune: the handle is not a shared-dictionary handle (one agent per replica: kb_prune)";
        return RS_ESTATE;
    }
    if (!k->is_reset) {
        k->err = "kb_shared_prune: call kb_reset first";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_shared_prune: the handle is between kb_shared_scan and kb_shared_commit of a round: finish the round first";
        return RS_ESTATE;
    }
    const kb_prune_kernel kn[5] = {kb::prune_shared_choose_kernel, kb::prune_shared_plan_kernel, kb::prune_shared_downdate_kernel,
                                   kb::prune_shared_move_kernel, kb::prune_shared_finish_kernel};
    return kb_prune_run(k, "kb_shared_prune", target, removed_total, kn, kb_shared_prune_tail);
}
