#!/usr/bin/env python3
"""Measures the closed control loop in Projectron++ mode (kb_set_control_plus) and writes
profiles/control_plus_record.json.  No threshold is attached to any figure; every figure is ONE run.

--replicas (4096) agents of scenario 0 learn in the resident loop (kb_run_resident, plain launches).  Around each step of --at
(50, 500, 2000) kernel timing is switched on for --window (10) steps: ms per closed-loop step by phase (kb_phase_times_ms: the
update phase is control_plus_kernel's one launch in Projectron++ mode), dictionary sizes, samples per step, how many of them
changed a dictionary and how many ran the mat-vec (kb_get_repair_work's work[6]).  Then the same for Projectron on the same
build, unchanged code, for scale.  The slowest learner's share of a Projectron++ step: the update phase is one launch of one
workgroup per learner, so with kernel timing on the agents are stepped once more on a handle of ONE replica that holds a copy of
the replica with the largest dictionary -- its update phase is that replica's workgroups alone.

  python tools/control_plus_record.py [--replicas 4096] [--at 50 500 2000] [--window 10] [--out profiles/control_plus_record.json]

--batch W (2, 4 or 8) measures kb_set_control_plus_batch instead and writes profiles/control_plus_batch_record.json:
the same agents, the same three points; at each point the fleet is forked into a second pair of handles --rounds (3) times per
width, widths 0 and W alternating, and the window is timed on the fork -- same dictionaries, same states, same steps for both
widths (their results are equal bit for bit, so either may carry the run between the points: W does).  Per point: the update
phase's ms per step as median and range over the rounds, kb_control_plus_batch_info's work[0..7] per step, and the largest
learner's share at both widths.  --also 2 4 adds one round each at further widths, for the curve.

--batch W --wide M measures kb_set_control_plus_wide instead and writes profiles/control_plus_wide_record.json: the
fleet runs at width W; at each point it is forked and the window is timed on the fork with the switch off and on (min_landmarks
M, --wide-rounds rounds), alternating, --rounds times each -- the update phase's ms per step as median (min - max) -- and so is
the replica with the largest dictionary alone on a one-replica handle.  --wide-also 512 1024 adds further M at the last point
(--wide-also-rounds rounds each, 1 by default); --cell 30 repeats the last point on a fleet of that many replicas (the reference's cell: 30 runs x 5 learners).
Where no learner reaches M the on-figure is the price of the empty rounds.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'network-slicing_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)


def _kernel_resources():
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    res = cr.parse()
    hit = [k for k in res if 'control_plus_kernel' in k]
    if not hit:
        return None
    r = res[hit[0]]
    return dict(vgprs=r.get('VGPRs'), sgprs_spilled=r.get('SGPRs Spill'), scratch_bytes_per_lane=r.get('ScratchSize'),
                occupancy=r.get('Occupancy'), lds_bytes=r.get('LDS Size'))


def _leg(mode, n, at, window, capacity, pool_bytes, seed):
    import ctypes as C
    import numpy as np
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice, default_fading
    cfg = make_config(0, n_envs=n)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=default_fading(), seed=seed)
    ag = VecKBRL(n, dims, n_prbs, capacity=capacity, pool_bytes=pool_bytes, algorithm=mode, control_plus=mode == 'projectron_plus')
    ia = np.full((n, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32)
    env.reset()
    ag.reset(ia, np.full((n, len(dims)), 3, dtype=np.int32))
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    out, step = [], 0
    for a in at:
        first = max(step, a - window // 2)
        t0 = time.perf_counter()
        if first > step:
            ag.run_resident(env, first - step, graph=False)
        ag.synchronize()
        between = time.perf_counter() - t0
        step = first
        s0, w0 = ag.stats(), ag._repair_raw()
        ag.set_kernel_timing(True)
        ag.phase_times_ms()
        t0 = time.perf_counter()
        ag.run_resident(env, window, graph=False)
        ag.synchronize()
        wall = time.perf_counter() - t0
        ph = ag.phase_times_ms()
        ag.set_kernel_timing(False)
        step += window
        s1, w1 = ag.stats(), ag._repair_raw()
        sizes = ag.dictionary_sizes()
        rec = dict(steps=[first, step], update_ms_per_step=ph['update_ms'], select_ms_per_step=ph['select_ms'],
                   wall_ms_per_step=wall * 1e3 / window, wall_s_since_the_last_window=between,
                   landmarks_mean=float(sizes.mean()), landmarks_max=int(sizes.max()),
                   changed_a_dictionary_per_step=(s1[1] - s0[1]) / window, insertions_per_step=(s1[2] - s0[2]) / window)
        if mode == 'projectron_plus':
            # (predictions_per_step: the update phase's samples plus select_action's predictions, as the counter holds them)
            rec['matvec_samples_per_step'] = (int(w1[6]) - int(w0[6])) / window
            rec['predictions_per_step'] = (s1[0] - s0[0]) / window
            worst = int(np.argmax(sizes.max(axis=1)))
            one = VecKBRL(1, dims, n_prbs, capacity=capacity, pool_bytes=1 << 30, algorithm=mode, control_plus=True)
            one.fork_from(ag, [worst])
            oenv = VecRanSlice(n_envs=1, cfg=make_config(0, n_envs=1), fading=default_fading(), seed=seed)
            oenv.reset()
            oenv.fork_from(env, [worst])
            one.set_kernel_timing(True)
            one.phase_times_ms()
            one.run_resident(oenv, window, graph=False)
            one.synchronize()
            rec['largest_replica_alone'] = dict(replica=worst, landmarks=sizes[worst].tolist(),
                                                update_ms_per_step=one.phase_times_ms()['update_ms'])
            rec['largest_replica_share_of_the_update_phase'] = (rec['largest_replica_alone']['update_ms_per_step'] / ph['update_ms']
                                                                if ph['update_ms'] else None)
            one.close()
            oenv.close()
        else:
            rec['predictions_per_step'] = (s1[0] - s0[0]) / window
        out.append(rec)
        print(mode, json.dumps(rec), flush=True)
    flags = ag.flagged_replicas()
    env.close()
    ag.close()
    return dict(windows=out, flagged=sum(len(v) for v in flags.values()))


def _batch_leg(width, also, rounds, n, at, window, capacity, pool_bytes, seed, max_landmarks):
    import ctypes as C
    import statistics
    import numpy as np
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice, default_fading
    cfg = make_config(0, n_envs=n)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    mode = 'projectron_plus'

    def pair(k, pool):
        return (VecRanSlice(n_envs=k, cfg=make_config(0, n_envs=k), fading=default_fading(), seed=seed),
                VecKBRL(k, dims, n_prbs, capacity=capacity, pool_bytes=pool, algorithm=mode, control_plus=True))
    env, ag = pair(n, pool_bytes)
    fenv, fag = pair(n, pool_bytes)        # the fork the windows are timed on
    oenv, one = pair(1, 1 << 30)           # the replica with the largest dictionary, alone
    ag.set_control_plus_batch(width, max_landmarks)
    ia = np.full((n, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32)
    env.reset()
    fenv.reset()
    oenv.reset()
    ag.reset(ia, np.full((n, len(dims)), 3, dtype=np.int32))
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    everyone = np.arange(n, dtype=np.int32)

    def timed(a, e, w):
        a.set_control_plus_batch(w, max_landmarks)      # (also restarts the counters)
        a.set_kernel_timing(True)
        a.phase_times_ms()
        r0 = a._repair_raw()
        a.run_resident(e, window, graph=False)
        a.synchronize()
        ms = a.phase_times_ms()['update_ms']
        a.set_kernel_timing(False)
        return ms, [v / window for v in a.control_plus_batch_work()], (int(a._repair_raw()[6]) - int(r0[6])) / window

    out, step = [], 0
    for a_ in at:
        first = max(step, a_ - window // 2)
        t0 = time.perf_counter()
        while step < first:      # (in stretches, with a sign of life between them)
            k = min(250, first - step)
            ag.run_resident(env, k, graph=False)
            ag.synchronize()
            step += k
            print('step %d, %.1f s' % (step, time.perf_counter() - t0), file=sys.stderr, flush=True)
        between = time.perf_counter() - t0
        sizes = ag.dictionary_sizes()
        worst = int(np.argmax(sizes.max(axis=1)))
        plan = [(w, r) for r in range(rounds) for w in (0, width)] + [(w, 0) for w in also]
        ms, work, matvec, alone = {}, {}, {}, {}
        for w, _ in plan:
            fag.fork_from(ag, everyone)
            fenv.fork_from(env, everyone)
            t, wk, mv = timed(fag, fenv, w)
            ms.setdefault(w, []).append(t)
            work[w], matvec[w] = wk, mv
        for w in (0, width):
            one.fork_from(ag, [worst])
            oenv.fork_from(env, [worst])
            alone[w] = timed(one, oenv, w)[0]
        rec = dict(steps=[first, first + window], wall_s_since_the_last_window=between, landmarks_mean=float(sizes.mean()),
                   landmarks_max=int(sizes.max()), largest_replica=dict(replica=worst, landmarks=sizes[worst].tolist()),
                   matvec_samples_per_step=matvec[0],
                   widths={str(w): dict(update_ms_per_step=dict(median=statistics.median(v), min=min(v), max=max(v), runs=v),
                                        work_per_step=work[w],
                                        **(dict(largest_replica_alone_update_ms_per_step=alone[w],
                                                largest_replica_share_of_the_update_phase=alone[w] / statistics.median(v))
                                           if w in alone else {}))
                           for w, v in ms.items()})
        out.append(rec)
        print(json.dumps(rec), flush=True)
        ag.set_control_plus_batch(width, max_landmarks)
        ag.run_resident(env, window, graph=False)
        step += window
    flags = ag.flagged_replicas()
    for h in (env, ag, fenv, fag, oenv, one):
        h.close()
    return dict(windows=out, flagged=sum(len(v) for v in flags.values()))


def _wide_leg(width, wide, wide_also, also_rounds, wide_rounds, rounds, n, at, window, capacity, pool_bytes, seed, max_landmarks):
    """the fleet at width `width`; per point the fork's window with the wide switch off (0) and on (`wide`), alternating"""
    import ctypes as C
    import statistics
    import numpy as np
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice, default_fading
    cfg = make_config(0, n_envs=n)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs

    def pair(k, pool):
        return (VecRanSlice(n_envs=k, cfg=make_config(0, n_envs=k), fading=default_fading(), seed=seed),
                VecKBRL(k, dims, n_prbs, capacity=capacity, pool_bytes=pool, algorithm='projectron_plus', control_plus=True,
                        control_plus_batch=width, control_plus_batch_max=max_landmarks))
    env, ag = pair(n, pool_bytes)
    fenv, fag = pair(n, pool_bytes)        # the fork the windows are timed on
    oenv, one = pair(1, 1 << 30)           # the replica with the largest dictionary, alone
    ia = np.full((n, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32)
    for e in (env, fenv, oenv):
        e.reset()
    ag.reset(ia, np.full((n, len(dims)), 3, dtype=np.int32))
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    everyone = np.arange(n, dtype=np.int32)

    def timed(a, e, m):
        a.set_control_plus_batch(width, max_landmarks)      # (restarts the counters)
        a.set_control_plus_wide(m, max_landmarks, wide_rounds)
        a.set_kernel_timing(True)
        a.phase_times_ms()
        a.run_resident(e, window, graph=False)
        a.synchronize()
        ms = a.phase_times_ms()['update_ms']
        a.set_kernel_timing(False)
        return ms, [v / window for v in a.control_plus_wide_work()], [v / window for v in a.control_plus_batch_work()]

    def summary(v):
        return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)

    out, step = [], 0
    for i, a_ in enumerate(at):
        first = max(step, a_ - window // 2)
        t0 = time.perf_counter()
        while step < first:      # (in stretches, with a sign of life between them)
            k = min(250, first - step)
            ag.run_resident(env, k, graph=False)
            ag.synchronize()
            step += k
            print('%d replicas: step %d, %.1f s' % (n, step, time.perf_counter() - t0), file=sys.stderr, flush=True)
        sizes = ag.dictionary_sizes()
        worst = int(np.argmax(sizes.max(axis=1)))
        plan = [(m, r) for r in range(rounds) for m in (0, wide)] + ([(m, r) for r in range(also_rounds) for m in wide_also] if i == len(at) - 1 else [])
        ms, wwork, bwork, alone = {}, {}, {}, {}
        for m, _ in plan:
            fag.fork_from(ag, everyone)
            fenv.fork_from(env, everyone)
            t, ww, bw = timed(fag, fenv, m)
            ms.setdefault(m, []).append(t)
            wwork[m], bwork[m] = ww, bw
        for m, _ in plan:
            one.fork_from(ag, [worst])
            oenv.fork_from(env, [worst])
            alone.setdefault(m, []).append(timed(one, oenv, m)[0])
        rec = dict(steps=[first, first + window], landmarks_mean=float(sizes.mean()), landmarks_max=int(sizes.max()),
                   learners_at_or_above={str(m): int((sizes >= m).sum()) for m in [wide] + list(wide_also)},
                   largest_replica=dict(replica=worst, landmarks=sizes[worst].tolist()),
                   min_landmarks={str(m): dict(update_ms_per_step=summary(v), wide_work_per_step=wwork[m], batch_work_per_step=bwork[m],
                                               largest_replica_alone_update_ms_per_step=summary(alone[m]))
                                  for m, v in ms.items()})
        out.append(rec)
        print(json.dumps(rec), flush=True)
        ag.run_resident(env, window, graph=False)
        step += window
    flags = ag.flagged_replicas()
    for h in (env, ag, fenv, fag, oenv, one):
        h.close()
    return dict(windows=out, flagged=sum(len(v) for v in flags.values()))


def _wide_resources():
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    return {k: dict(vgprs=r.get('VGPRs'), agprs=r.get('AGPRs'), scratch_bytes_per_lane=r.get('ScratchSize'), occupancy=r.get('Occupancy'),
                    lds_bytes=r.get('LDS Size'))
            for k, r in cr.parse().items() if 'cpw_' in k or 'control_plus_batch_kernel' in k}


def _batch_resources():
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    res = cr.parse()
    out = {}
    for k, r in res.items():
        if 'control_plus_batch_kernel' in k or 'control_plus_kernel' in k:
            out[k] = dict(vgprs=r.get('VGPRs'), agprs=r.get('AGPRs'), sgprs_spilled=r.get('SGPRs Spill'),
                          scratch_bytes_per_lane=r.get('ScratchSize'), occupancy=r.get('Occupancy'), lds_bytes=r.get('LDS Size'))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, choices=[2, 4, 8], default=None,
                    help='measure kb_set_control_plus_batch at this width against width 0 (writes profiles/control_plus_batch_record.json)')
    ap.add_argument('--also', type=int, nargs='*', default=[], help='with --batch: further widths, one round each')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--wide', type=int, default=0, metavar='M',
                    help='with --batch: measure kb_set_control_plus_wide at min_landmarks M against the switch off (writes '
                         'profiles/control_plus_wide_record.json)')
    ap.add_argument('--wide-also', type=int, nargs='*', default=[], help='with --wide: further M at the last point')
    ap.add_argument('--wide-also-rounds', type=int, default=1, help='with --wide-also: rounds of each further M')
    ap.add_argument('--wide-rounds', type=int, default=32, help='with --wide: the rounds enqueued per update phase')
    ap.add_argument('--cell', type=int, default=0, help='with --wide: repeat the last point on a fleet of this many replicas')
    ap.add_argument('--max-landmarks', type=int, default=2048)
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--at', type=int, nargs='*', default=[50, 500, 2000])
    ap.add_argument('--window', type=int, default=10)
    ap.add_argument('--capacity', type=int, default=2048)
    ap.add_argument('--pool-gb', type=float, default=48.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'control_plus_record.json'))
    args = ap.parse_args()
    if args.wide and not args.batch:
        ap.error('--wide needs --batch')
    if args.wide:
        out = args.out if args.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'control_plus_wide_record.json')
        rec = dict(what='closed control loop in Projectron++ mode at batch width %d, scenario 0, %d replicas on one device: '
                        'kb_set_control_plus_wide at min_landmarks %d (%d rounds) against the switch off on forks of the same fleet, %d '
                        'rounds each alternating; plain launches, kernel timing on for %d steps per window; no threshold attached'
                        % (args.batch, args.replicas, args.wide, args.wide_rounds, args.rounds, args.window),
                   replicas=args.replicas, window=args.window, width=args.batch, rounds=args.rounds, max_landmarks=args.max_landmarks,
                   min_landmarks=args.wide, wide_rounds=args.wide_rounds, wide_also=args.wide_also, wide_also_rounds=args.wide_also_rounds,
                   kernels=_wide_resources())
        pool = int(args.pool_gb * (1 << 30))
        at = sorted(args.at)
        rec['fleet'] = _wide_leg(args.batch, args.wide, args.wide_also, args.wide_also_rounds, args.wide_rounds, args.rounds, args.replicas, at, args.window,
                                 args.capacity, pool, args.seed, args.max_landmarks)
        if args.cell:
            rec['cell'] = dict(replicas=args.cell, **_wide_leg(args.batch, args.wide, args.wide_also, args.wide_also_rounds, args.wide_rounds, args.rounds, args.cell,
                                                               at[-1:], args.window, args.capacity, min(pool, 8 << 30), args.seed,
                                                               args.max_landmarks))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        return
    if args.batch:
        out = args.out if args.out != ap.get_default('out') else os.path.join(ROOT, 'profiles', 'control_plus_batch_record.json')
        rec = dict(what='closed control loop in Projectron++ mode, scenario 0, %d replicas on one device: kb_set_control_plus_batch at '
                        'width %d against width 0 on forks of the same fleet, %d rounds per width alternating; plain launches, kernel '
                        'timing on for %d steps per window; no threshold attached' % (args.replicas, args.batch, args.rounds, args.window),
                   replicas=args.replicas, window=args.window, width=args.batch, rounds=args.rounds, max_landmarks=args.max_landmarks,
                   kernels=_batch_resources())
        rec.update(_batch_leg(args.batch, args.also, args.rounds, args.replicas, sorted(args.at), args.window, args.capacity,
                              int(args.pool_gb * (1 << 30)), args.seed, args.max_landmarks))
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump(rec, fh, indent=1, sort_keys=True)
            fh.write('\n')
        return
    rec = dict(what='closed control loop, scenario 0, %d replicas on one device: Projectron++ behind kb_set_control_plus, and '
                    'Projectron on the same build for scale; one run per figure, no threshold attached' % args.replicas,
               replicas=args.replicas, window=args.window, kernel=_kernel_resources())
    for mode in ('projectron_plus', 'projectron'):
        rec[mode] = _leg(mode, args.replicas, sorted(args.at), args.window, args.capacity, int(args.pool_gb * (1 << 30)), args.seed)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
