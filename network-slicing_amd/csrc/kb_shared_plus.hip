// kb_shared_plus.hip -- the switch behind which a shared-dictionary handle's proposal rounds learn by ProjectronPlus.update
// (projectron.py:66-107) instead of Projectron.update: kb_set_shared_plus / kb_get_shared_plus (ranslice.h).
// #included by rs_api.hip after kb_fit_steps_batch.hip.  The device code is in kb_kbrl.hip, beside the instances it is a variant
// of: shared_scan_plus_kernel proposes the first candidate with y f < 1, shared_apply_plus_kernel walks a merged list by the
// margin rule (apply_full_batch<true> for a dictionary at its capacity, apply_update_plus one by one for one that can still grow).
// launch_shared_scan and launch_shared_apply (kb_api.hip) pick the instance from the handle's switch; with the switch off every
// launch is the one it was.

/* Host state of the handle, like kb_set_control_plus: off by default, in no kb_save_state blob, neither carried nor changed by
   kb_share, kb_unshare and kb_shared_prune.  kb_get_algorithm keeps answering KB_ALG_PROJECTRON on a shared handle. */
extern "C" int kb_set_shared_plus(kb_handle* k, int32_t on) {
    if (!k) return RS_EINVAL;
    if (on != 0 && on != 1) {
        k->err = "kb_set_shared_plus: on = " + std::to_string(on) + " (0: the rounds learn by Projectron's rule, the default; 1: by the margin rule of Projectron++)";
        return RS_EINVAL;
    }
    if (!k->D.shared) {
        k->err = "kb_set_shared_plus: not a shared-dictionary handle (the closed loop of a per-replica handle learns by the margin rule behind "
                 "kb_set_control_plus)";
        return RS_ESTATE;
    }
    if (k->round_open) {
        k->err = "kb_set_shared_plus: a round is open between kb_shared_scan and kb_shared_commit; the rule changes between steps only";
        return RS_ESTATE;
    }
    k->shared_plus = on;
    return RS_OK;
}

extern "C" int kb_get_shared_plus(kb_handle* k, int32_t* on) {
    if (!k || !on) return RS_EINVAL;
    *on = k->shared_plus;
    return RS_OK;
}
