#!/usr/bin/env python3
"""Register/scratch budget of the step-kernel instances, from the remarks of the last build
(network-slicing_amd/csrc/build/resources.log): VGPRs, scratch, occupancy, spilled SGPRs and VGPRs and LDS of every instance.  The two 16-lane production instances are built for 5 waves per
SIMD (96 VGPRs) and spill; instances that spilled more than ~256 B per lane have twice been seen to compute wrong
values on this toolchain, so the build fails if a change pushes them past 240 B."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'build', 'resources.log')
LIMIT = 240
KB_SCRATCH = {'update_small_kernel': 64, 'update_heavy_kernel': 16, 'update_control_kernelILb0E': 16, 'heavy_finish_kernel': 0,
              'heavy_matvec_kernel': 0, 'heavy_rank1_kernel': 0, 'select_bin_kernel': 16, 'select_bin_big_kernel': 16, 'select_gemm_kernel': 0}
# kb_prune's kernels (kb_prune.hip): reported, and held to no scratch at all -- the downdate is a pure streaming kernel
PRUNE = ['prune_list_kernel', 'prune_choose_kernel', 'prune_plan_kernel', 'prune_downdate_kernel', 'prune_move_kernel', 'prune_finish_kernel']
# kb_shared_prune's kernels (kb_shared_prune.hip): the same rule on full storage, reported beside them and held to no scratch as well
PRUNE_SHARED = ['prune_shared_choose_kernel', 'prune_shared_plan_kernel', 'prune_shared_downdate_kernel', 'prune_shared_move_kernel',
                'prune_shared_finish_kernel']
# the online budget's kernels (kb_online_prune.hip): the stage's list and its persistent choose / move / finish
# kernel, reported beside kb_prune's (whose plan and downdate the stage launches as they are) and held to no scratch as well
ONLINE_PRUNE = ['budget_list_kernel', 'budget_round_kernel']
# the same stage behind a shared learning step (kb_shared_online_prune.hip): its persistent choose / move / finish
# kernel on full storage (the list kernel above and kb_shared_prune's plan and downdate are launched as they are): no scratch
SHARED_ONLINE_PRUNE = ['shared_budget_round_kernel']
# kb_deploy_ref's kernels (kb_ref.hip): reported, and held to no scratch at all, as they are built and documented
REF_SCRATCH = {'select_ref_kernel': 0, 'ref_gather_kernel': 0}
# the agent-file kernels (kb_agents.hip): reported, and held to no scratch at all -- pack and build are pure streaming kernels
AGENTS = ['agents_count_kernel', 'agents_tables_kernel', 'agents_pack_kernel', 'agents_build_kernel', 'agents_finish_kernel']
# kb_fork_rebuild's kernels (kb_rebuild.hip): reported; the two streaming kernels of the rounds are held to no scratch at all, the
# per-dictionary ones to what update_small_kernel is allowed (they inline the same triangle mat-vec)
REBUILD_SCRATCH = {'rebuild_sizes_kernel': 0, 'rebuild_pages_kernel': 0, 'rebuild_small_kernel': 64, 'rebuild_matvec_kernel': 0,
                   'rebuild_finish_kernel': 0, 'rebuild_rank1_kernel': 0}
# the bridge's kernels (kb_bridge.hip): reported, and held to no scratch at all -- gathers on kb_fork's work line
BRIDGE = ['unshare_count_kernel', 'unshare_tables_kernel', 'unshare_shells_kernel', 'share_tables_kernel', 'share_shells_kernel']
# kb_fork's own kernels (kb_fork.hip), whose gather helpers and work line the bridge's and kb_fork_rebuild's call: the same
FORK = ['fork_count_kernel', 'fork_scan_kernel', 'fork_tables_kernel', 'fork_shells_kernel']
# kb_fit / kb_score (kb_fit.hip): reported; the scoring kernel is held to no scratch at all (KB_SCORE_Q was chosen by that), the
# fitting kernel -- predict_column and apply_update inlined into one persistent loop -- to what the build shows: none either; so
# is its Projectron++ instance (fit_plus_kernel: the same loop around apply_update_plus)
FIT_SCRATCH = {'fit_kernel': 0, 'fit_plus_kernel': 0, 'score_kernel': 0}
# kb_fit's chip-wide rounds (kb_fit_wide.hip): reported, and held to no scratch at all -- the scan is score_kernel's
# body, the two streaming kernels call the walker heavy_matvec_kernel and heavy_rank1_kernel call (walk_stretch, kb_kbrl.hip) on a
# work line of their own
FIT_SCRATCH.update({k: 0 for k in ('fit_wide_classify_kernel', 'fit_wide_scan_kernel', 'fit_wide_decide_kernel', 'fit_wide_plan_kernel',
                                   'fit_wide_matvec_kernel', 'fit_wide_finish_kernel', 'fit_wide_rank1_kernel')})
# kb_fit_steps (kb_fit_steps.hip): fit_learner's loop around the cached-prefix column, in both update rules: no scratch
FIT_SCRATCH.update({'fit_steps_kernel': 0, 'fit_steps_plus_kernel': 0})
# the closed loop's update phase in Projectron++ mode (kb_control_plus.hip): fit_steps_plus_kernel's row behind
# update_control's bookkeeping: no scratch
FIT_SCRATCH.update({'control_plus_kernel': 0})
# the same row with one pass over Kinv for a group of candidates (kb_control_plus_batch.hip), one instance per
# width, all built for two waves per SIMD: held to the VGPRs, LDS and scratch the build shows -- (registers, LDS bytes, scratch
# bytes per lane).  Widths 2 and 4 have no scratch.  Width 8 spills 196 B per lane at two waves per SIMD; left at one wave per SIMD
# (306 registers, no scratch) it was slower at every point measured (DESIGN.md §8m has both sets of figures)
CTL_BATCH = {'control_plus_batch_kernelILi2E': (209, 19968, 0), 'control_plus_batch_kernelILi4E': (249, 28240, 0),
             'control_plus_batch_kernelILi8E': (256, 44784, 196)}
# kb_fit_steps's rows through the same walk (kb_fit_steps_batch.hip), the same three widths at two waves per SIMD:
# what the build shows, which is the control loop's instances' but for 8 B per lane more at width 8.  (As a row loop inside a
# learner loop the kernel showed 124 B at width 4 and 372 B at width 8; it is one loop, a row per trip, for that reason.)
FIT_STEPS_BATCH = {'fit_steps_batch_kernelILi2E': (209, 19968, 0), 'fit_steps_batch_kernelILi4E': (249, 28240, 0),
                   'fit_steps_batch_kernelILi8E': (256, 44784, 204)}
# the same update phase with the large learners' passes spread over the chip (kb_control_plus_wide.hip): scratch
# bytes per lane.  The two kernels that stream Kinv (the pass, per width, and the rank-1 update), the list and the plan hold none;
# the walk holds none either; the rows kernel (the batch kernel's row, with the heavy learners' early exit) and the finisher (its
# walk from a cursor) are held to what the build shows at two waves per SIMD, below the 240 B line
CTL_WIDE = {'cpw_list_kernel': 0, 'cpw_plan_kernel': 0, 'cpw_rank1_kernel': 0,
            'cpw_pass_kernelILi2E': 0, 'cpw_pass_kernelILi4E': 0, 'cpw_pass_kernelILi8E': 0,
            'cpw_walk_kernelILi2E': 0, 'cpw_walk_kernelILi4E': 0, 'cpw_walk_kernelILi8E': 0,
            'cpw_rows_kernelILi2E': 0, 'cpw_rows_kernelILi4E': 0, 'cpw_rows_kernelILi8E': 220,
            'cpw_finish_kernelILi2E': 0, 'cpw_finish_kernelILi4E': 0, 'cpw_finish_kernelILi8E': 116}
# the shared-dictionary rounds under the margin rule (kb_set_shared_plus): each instance beside the Projectron one
# it is a variant of.  The scan holds no scratch and keeps the occupancy its __launch_bounds__(64, KB_SCAN_OCC) asks for; the
# apply may spill no more than the Projectron instance does
SHARED_PLUS = {'shared_scan_plus_kernel': 'shared_scan_kernel', 'shared_apply_plus_kernel': 'shared_apply_kernel'}
# the segments of a growing shared dictionary under the margin rule (kb_shared_plus_batch.hip): the wide kernels and
# begin kernel hold no scratch; the walk and the finishing kernel (both run apply_update_plus) no more than shared_apply_plus_kernel
SHARED_PLUS_BATCH = ('spb_begin_kernel', 'spb_cols_kernel', 'spb_matvec_kernel', 'spb_gram_kernel', 'spb_walk_kernel', 'spb_finish_kernel')
KB_SCAN_OCC = 3
PRODUCTION = ["embb_step_kernelILi16ELb0ELb0ELb1E", "embb_step_kernelILi16ELb0ELb1ELb1E"]   # <16, false, plain | BLOCK, FDIV>
PLAIN = PRODUCTION[0]          # the instance bench.py's headline runs
STEP_KERNEL = 'embb_step_kernelIL'
LDS_LIMIT = 32768              # per block: five blocks of the 16-lane instances share a CU's 160 KiB
# SGPRs the plain instance may spill.  Every spilled SGPR is parked in a lane of a VGPR the 96-register allocation then lacks, and
# fetched back with a v_readlane -- a VALU issue slot in a kernel bound by VALU issue -- wherever it is used (tools/spill_sites.py
# lists the sites).  The parent of this ceiling spilled 137; the value is what the build that introduced it reports
# (profiles/HISTORY.md, "Step kernel: launch constants and spilled SGPRs").
SGPR_SPILL_CEILING = 105
# the device listing of the same build (csrc/Makefile: build/rs_api.s): the plain instance's two hottest loops hold no spill reload
LISTING = os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'build', 'rs_api.s')


def parse(path=LOG):
    out, cur = {}, None
    for line in open(path, errors='replace'):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]+\])?: (\d+)', line)
        if m and cur:
            out[cur][m.group(1).strip()] = int(m.group(2))
    return out


def step_instances(res):
    """{template arguments as mangled, e.g. 'ILi16ELb0ELb0ELb1E' (<lanes, TRACE, BLOCK, FDIV>): remarks} of every step-kernel instance"""
    out = {}
    for k, r in res.items():
        m = re.search(r'embb_step_kernel(ILi\d+ELb[01]ELb[01]ELb[01]E)', k)
        if m:
            out[m.group(1)] = r
    return out


def check(path=LOG):
    res = parse(path)
    bad = []
    # every instance of the step kernel, the spilled registers of both files beside the allocation: the tracing, 8- and 32-lane
    # instances come from the same template, and what a change does to the production pair it does to them
    for targs, r in sorted(step_instances(res).items()):
        print('embb_step_kernel%s: VGPRs %s, scratch %s B/lane, occupancy %s, SGPRs spilled %s, VGPRs spilled %s, LDS %s B' % (
            targs, r.get('VGPRs'), r.get('ScratchSize'), r.get('Occupancy'), r.get('SGPRs Spill'), r.get('VGPRs Spill'), r.get('LDS Size')))
    for key in PRODUCTION:
        hit = [k for k in res if key in k]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        if r.get('ScratchSize', 0) > LIMIT:
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], LIMIT))
        if r.get('Occupancy', 0) < 5:
            bad.append('%s: occupancy %s < 5 waves/SIMD' % (key, r.get('Occupancy')))
        if r.get('LDS Size', 0) > LDS_LIMIT:
            bad.append('%s: %d B of LDS per block (> %d: five blocks no longer fit a CU)' % (key, r['LDS Size'], LDS_LIMIT))
        if key == PLAIN and r.get('SGPRs Spill', 0) > SGPR_SPILL_CEILING:
            bad.append('%s spills %d SGPRs (> %d)' % (key, r['SGPRs Spill'], SGPR_SPILL_CEILING))
    # where the plain instance's remaining reloads sit: none in the fast reception round loop, none in the PF leader's run
    if path == LOG:
        if not os.path.exists(LISTING):
            bad.append('%s: no device listing (make -C network-slicing_amd/csrc)' % LISTING)
        else:
            sys.path.insert(0, os.path.join(ROOT, 'tools'))
            import spill_sites
            problems = spill_sites.check_step_loops(LISTING, PLAIN)
            print('%s: fast reception round loop and PF leader-run loop: %s' % (PLAIN, '; '.join(problems) if problems else 'no spill reload'))
            bad += problems
    # The agent's per-learner kernels sit at their register limit too: a refactoring of a helper they inline (round 5: lambdas in the
    # triangle mat-vec) put 608 B per lane of scratch into update_small_kernel / update_heavy_kernel and doubled their time unnoticed.
    for key, limit in KB_SCRATCH.items():
        hit = [k for k in res if key in k]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
        elif res[hit[0]].get('ScratchSize', 0) > limit:
            bad.append('%s spills %d B/lane (> %d)' % (key, res[hit[0]]['ScratchSize'], limit))
    for key in PRUNE + PRUNE_SHARED:
        hit = [k for k in res if key in k]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('ScratchSize'), r.get('Occupancy'),
                                                                           r.get('LDS Size')))
        if r.get('ScratchSize', 0) > 0:
            bad.append('%s spills %d B/lane (> 0)' % (key, r['ScratchSize']))
    for key in ONLINE_PRUNE + SHARED_ONLINE_PRUNE + AGENTS + BRIDGE + FORK:
        hit = [k for k in res if re.search(r'\d' + key, k)]  # (the whole mangled name: share_* is not unshare_*)
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('ScratchSize'), r.get('Occupancy'),
                                                                           r.get('LDS Size')))
        if r.get('ScratchSize', 0) > 0:
            bad.append('%s spills %d B/lane (> 0)' % (key, r['ScratchSize']))
    for key, limit in REF_SCRATCH.items():
        hit = [k for k in res if key in k]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s, scratch %s B/lane, occupancy %s' % (key, r.get('VGPRs'), r.get('ScratchSize'), r.get('Occupancy')))
        if r.get('ScratchSize', 0) > limit:
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], limit))
    for key, limit in list(REBUILD_SCRATCH.items()) + list(FIT_SCRATCH.items()):
        hit = [k for k in res if re.search(r'\d' + key, k)] if key in FIT_SCRATCH else [k for k in res if key in k]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('ScratchSize'), r.get('Occupancy'),
                                                                           r.get('LDS Size')))
        if r.get('ScratchSize', 0) > limit:
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], limit))
    for key, (regs, lds, scratch) in list(CTL_BATCH.items()) + list(FIT_STEPS_BATCH.items()):
        hit = [k for k in res if re.search(r'\d' + key, k)]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        used = r.get('VGPRs', 0) + r.get('AGPRs', 0)
        print('%s: VGPRs %s + AGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('AGPRs'), r.get('ScratchSize'),
                                                                                      r.get('Occupancy'), r.get('LDS Size')))
        if used > regs:
            bad.append('%s uses %d vector registers (> %d)' % (key, used, regs))
        if r.get('LDS Size', 0) > lds:
            bad.append('%s uses %d B of LDS (> %d)' % (key, r['LDS Size'], lds))
        if r.get('ScratchSize', 0) > scratch:
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], scratch))
    for key, scratch in CTL_WIDE.items():
        hit = [k for k in res if re.search(r'\d' + key, k)]
        if not hit:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s + AGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('AGPRs'), r.get('ScratchSize'),
                                                                                      r.get('Occupancy'), r.get('LDS Size')))
        if r.get('ScratchSize', 0) > min(scratch, LIMIT):
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], scratch))
    for key, base in SHARED_PLUS.items():
        hit, hit0 = [k for k in res if re.search(r'\d' + key, k)], [k for k in res if re.search(r'\d' + base, k)]
        if not hit or not hit0:
            bad.append('%s: not found in %s' % (key if not hit else base, path))
            continue
        for name, r in ((base, res[hit0[0]]), (key, res[hit[0]])):
            print('%s: VGPRs %s, SGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (name, r.get('VGPRs'), r.get('TotalSGPRs'),
                                                                                        r.get('ScratchSize'), r.get('Occupancy'), r.get('LDS Size')))
        r, r0 = res[hit[0]], res[hit0[0]]
        if 'scan' in key:
            if r.get('ScratchSize', 0) > 0 or r0.get('ScratchSize', 0) > 0:
                bad.append('%s / %s: the scan spills (%s / %s B/lane)' % (key, base, r.get('ScratchSize'), r0.get('ScratchSize')))
            if min(r.get('Occupancy', 0), r0.get('Occupancy', 0)) < KB_SCAN_OCC:
                bad.append('%s / %s: occupancy %s / %s < %d waves/SIMD' % (key, base, r.get('Occupancy'), r0.get('Occupancy'), KB_SCAN_OCC))
        elif r.get('ScratchSize', 0) > r0.get('ScratchSize', 0):
            bad.append('%s spills %d B/lane (> %d, the Projectron instance)' % (key, r['ScratchSize'], r0['ScratchSize']))
    base = [k for k in res if re.search(r'\d' + 'shared_apply_plus_kernel', k)]
    for key in SHARED_PLUS_BATCH:
        hit = [k for k in res if re.search(r'\d' + key, k)]
        if not hit or not base:
            bad.append('%s: not found in %s' % (key, path))
            continue
        r = res[hit[0]]
        print('%s: VGPRs %s, SGPRs %s, scratch %s B/lane, occupancy %s, LDS %s B' % (key, r.get('VGPRs'), r.get('TotalSGPRs'),
                                                                                    r.get('ScratchSize'), r.get('Occupancy'), r.get('LDS Size')))
        limit = res[base[0]].get('ScratchSize', 0) if key in ('spb_walk_kernel', 'spb_finish_kernel') else 0
        if r.get('ScratchSize', 0) > limit:
            bad.append('%s spills %d B/lane (> %d)' % (key, r['ScratchSize'], limit))
    return bad


if __name__ == '__main__':
    problems = check()
    for p in problems:
        print('RESOURCE CHECK FAILED:', p)
    sys.exit(1 if problems else 0)
