#!/usr/bin/env python3
"""Measures budgeted shared dictionaries (kb_shared_prune, SharedVecKBRL.shrink) and writes
profiles/shared_prune_record.json.  No threshold is attached to any figure, and nothing is asserted about a ratio.

The shape is the bench's config 4 (scenario index 2, --replicas (4096) replicas, capacity 1024, budget 256, one exchange round
per step, its own world), closed loop through step_resident for --steps steps, run twice, each run a child process of its own
under `timeout`:
  plain    as it is: the largest dictionary reaches its capacity and from then on every mistake is projected;
  shrink   the same, and from the first multiple of --every (200) steps at which a dictionary is at its capacity on, one
           shrink(--target (768)) every --every steps.
Recorded for both, per window of 100 steps: insertions (kb_get_stats[2]), the dictionary sizes at the window's end, SLA
violations per step and replica (mean over the window), wall ms per step.  Every step ends with a fetch of its violations, in
both runs alike, so the ms per step include it.  Per shrink: landmarks removed, rounds (the most any dictionary needed), sizes
before and after, and either the device ms of its three kernels (kb_prune_time_ms, with the launches counted; kernel timing is
switched on for that call alone) or -- every other shrink, timing off -- the wall ms of the call.

--shared-plus: the fleet learns by the margin rule of Projectron++ in both runs (kb_set_shared_plus); the record
then says so, and --out should name another file than the committed one.

--online-prune T [--online-prune-rounds R[,R...]] [--repeat K] [--against DIR] [--time-budget S]: the budget inside the step
(kb_set_shared_online_prune) beside the two runs above.  Modes, each a child of its own under `timeout`, K times
over in this order (alternating, so that drift of the machine falls on all alike): parent_plain -- with --against DIR, a built
checkout of the parent commit: ITS tool's `--child plain`, the same cell on the parent's library --; plain; shrink (--target,
--every); online_rR for every R given -- the stage on at target T with R rounds, never combined with the periodic shrink --; and
the idle pair idle_off / idle_on: the same fleet at --idle-capacity (4096) for --idle-steps (100) steps, switch off and stage on at
the target idle-capacity - 1, compared over the windows at whose end no dictionary had reached that target, so that the
difference is the stage's 2 + 3 R launches that find nothing to do.  (At the cell's own capacity no target is idle: a full
dictionary exceeds capacity - 1, the largest one there is.  The pair is short because a dictionary that grows takes its
proposals one by one -- some 100 ms per step in this cell, where the dictionary holds 3,695 landmarks at step 100 and 4,096 at
step 200 -- and a stage that works on a dictionary of thousands of landmarks costs some 200 ms per step: the children's
--timeout (400 s) covers 1,400 steps at 30 ms and 100 at 200 ms with room to spare, not a long pair past its saturation.)
--time-budget S: no further round of all modes is begun once the rounds so far and another one like the last would pass S
seconds; the record says how many rounds it holds.  Per mode and run: ms per step over all windows and over the windows from step
200 on, the windows themselves (insertions, sizes, violations per step and replica), the largest dictionary, the stage's counters
per window (shared_online_prune_info; carry = dictionary-stages left above the target), the shrinks with their wall or device
time; per mode the median and the range over the runs.  The record is written after every run and goes to
profiles/shared_online_prune_record.json unless --out says otherwise.

  python tools/shared_prune_record.py [--replicas 4096] [--steps 1400] [--target 768] [--every 200] [--shared-plus]
  python tools/shared_prune_record.py --online-prune 768 --online-prune-rounds 1,2,4,8 --repeat 3 --against ../parent
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO, BUDGET, MAX_ROUNDS, CAPACITY, FADING_COLS, WINDOW = 2, 256, 1, 1024, 4096, 100
ONLINE_OUT = os.path.join(ROOT, 'profiles', 'shared_online_prune_record.json')


def child(a):
    import numpy as np
    from ranslice.config import make_config, EMBB_A, EMBB_SEC, MMTC_A, MMTC_SEC
    from ranslice.fading import synth_fading
    from ranslice.kbrl_dev import SharedVecKBRL
    from ranslice.sharding import replica_seeds
    from ranslice.vec_env import VecRanSlice
    n = a.replicas
    cfg = make_config(SCENARIO, n_envs=n)
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=[synth_fading(t, FADING_COLS) for t in range(3)])
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    rng = np.random.default_rng(1000)
    ia = np.concatenate([rng.integers(EMBB_A[0], EMBB_A[1], size=(n, cfg.n_embb)),
                         rng.integers(MMTC_A[0], MMTC_A[1], size=(n, cfg.n_mmtc))], axis=1).astype(np.int32)
    sf = np.concatenate([rng.integers(EMBB_SEC[0], EMBB_SEC[1], size=(n, cfg.n_embb)),
                         rng.integers(MMTC_SEC[0], MMTC_SEC[1], size=(n, cfg.n_mmtc))], axis=1).astype(np.int32)
    env.reset(seeds=replica_seeds(0, 0, n))
    online = (a.online_prune, int(a.online_prune_rounds)) if a.mode == 'online' else None
    agent = SharedVecKBRL(n, dims, cfg.n_prbs, budget=BUDGET, max_rounds=MAX_ROUNDS, capacity=a.capacity, shared_plus=a.shared_plus,
                          shared_plus_batch=a.shared_plus_batch or None, shared_online_prune=online[0] if online else None,
                          shared_online_prune_rounds=online[1] if online else 2)
    agent.reset(ia, sf, seeds=replica_seeds(7, 0, n))
    assert agent.shared_online_prune == online
    env._check(env.L.rs_step(env.h, np.ascontiguousarray(ia).ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    windows, shrinks = [], []
    grown, saturated_at, pool0 = agent.stats()[2], None, None
    for w0 in range(0, a.steps, WINDOW):
        viol = 0.0
        env.synchronize()
        agent.synchronize()
        t0 = time.perf_counter()
        for _ in range(WINDOW):
            agent.step_resident(env)
            env.step_resident()
            viol += float(env.fetch()['violations'].sum())
        agent.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / WINDOW
        now, sizes = agent.stats()[2], agent.dictionary_sizes().astype(int)
        windows.append(dict(steps=[w0, w0 + WINDOW], insertions=int(now - grown), dictionary_sizes=sizes.tolist(),
                            violations_per_step_and_replica=viol / WINDOW / n, ms_per_step=ms))
        if online:
            windows[-1]['online_prune_info'] = agent.shared_online_prune_info()
        grown = now
        step = w0 + WINDOW
        if saturated_at is None and sizes.max() >= a.capacity:
            saturated_at = step
        if a.mode == 'shrink' and saturated_at is not None and step % a.every == 0 and step < a.steps:
            timed = len(shrinks) % 2 == 0
            pool0 = pool0 or agent.pool()['used_bytes']
            agent.set_kernel_timing(timed)
            agent.synchronize()
            t0 = time.perf_counter()
            removed = agent.shrink(a.target)
            wall = 1e3 * (time.perf_counter() - t0)
            pt = agent.prune_times_ms()
            agent.set_kernel_timing(False)
            after = agent.dictionary_sizes().astype(int)
            rec = dict(step=step, removed=removed, rounds=int((sizes - after).max()), sizes_before=sizes.tolist(), sizes_after=after.tolist(),
                       pool_used_bytes_unchanged=bool(agent.pool()['used_bytes'] == pool0))
            if timed:
                rec.update(device_ms=dict(choose=pt['choose_ms'], downdate=pt['downdate_ms'], move=pt['move_ms']),
                           launches=dict(choose=pt['n_choose'], downdate=pt['n_downdate'], move=pt['n_move']),
                           device_ms_sum=pt['choose_ms'] + pt['downdate_ms'] + pt['move_ms'])
            else:
                rec.update(wall_ms=wall)
            shrinks.append(rec)
    out = dict(mode=a.mode, replicas=n, steps=a.steps, saturated_by_step=saturated_at, windows=windows, pruned=agent.pruned().tolist())
    out.update(capacity=a.capacity, largest_dictionary=max(max(w['dictionary_sizes']) for w in windows))
    if online:
        out.update(online_prune=list(online), online_prune_info=agent.shared_online_prune_info(), launches_per_stage=2 + 3 * online[1])
    if a.mode == 'shrink':
        pt = agent.prune_times_ms()
        out.update(shrinks=shrinks, target=a.target, every=a.every, downdate_bytes_read_plus_written=pt['downdate_bytes'],
                   downdate_launches_with_work=pt['downdate_launches'])
    agent.close()
    env.close()
    print(json.dumps(out))


def run(mode, a, extra=(), script=None, steps=None):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, script or os.path.abspath(__file__), '--child', mode, '--replicas', str(a.replicas),
           '--steps', str(steps or a.steps), '--target', str(a.target), '--every', str(a.every)] + (['--shared-plus'] if a.shared_plus else []) + (
        ['--shared-plus-batch', str(a.shared_plus_batch)] if a.shared_plus_batch else []) + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def _spread(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2]), min=v[0], max=v[-1], runs=len(v))


def _summaries(rec, a):
    """per mode the median and range over its runs, and the idle pair window by window"""
    for label, m in rec['modes'].items():
        if not m['runs']:
            continue
        first = m['runs'][0]
        m['ms_per_step_all'] = _spread([r['ms_per_step_all'] for r in m['runs']])
        m['ms_per_step_from_step_200'] = _spread([r['ms_per_step_from_step_200'] for r in m['runs']])
        m['largest_dictionary'] = max(r['largest_dictionary'] for r in m['runs'])
        m['insertions_per_window'] = [x['insertions'] for x in first['windows']]
        m['violations_per_step_and_replica'] = _spread([sum(x['violations_per_step_and_replica'] for x in r['windows']) / len(r['windows'])
                                                        for r in m['runs']])
        if 'online_prune_info' in first:
            m['online_prune_info'] = first['online_prune_info']
            m['carry_per_window'] = [x['online_prune_info']['carry'] for x in first['windows']]
        walls = [s['wall_ms'] for r in m['runs'] for s in r.get('shrinks', []) if 'wall_ms' in s]
        if walls:
            m['shrink_wall_ms'] = _spread(walls)
    off, on = rec['modes']['idle_off']['runs'], rec['modes']['idle_on']['runs']
    if off and on:
        n = min(len(r['windows']) for r in off + on)
        quiet = [i for i in range(n) if all(max(r['windows'][i]['dictionary_sizes']) < a.idle_capacity - 1 for r in off + on)]
        per = lambda rs: _spread([sum(r['windows'][i]['ms_per_step'] for i in quiet) / len(quiet) for r in rs])
        rec['idle'] = dict(windows_compared=quiet, launches_per_stage=on[0]['launches_per_stage'],
                           removed_in_them=[r['windows'][quiet[-1]]['online_prune_info']['removed'] if quiet else None for r in on])
        if quiet:
            rec['idle'].update(ms_per_step_off=per(off), ms_per_step_on=per(on))
            rec['idle']['us_per_launch'] = 1e3 * (rec['idle']['ms_per_step_on']['median'] - rec['idle']['ms_per_step_off']['median']) / on[0]['launches_per_stage']


def online_record(a):
    """the modes of --online-prune, up to a.repeat times over in one fixed order; one child on the GPU at a time"""
    rounds = [int(r) for r in str(a.online_prune_rounds).split(',')]
    idle = ['--capacity', str(a.idle_capacity)]
    order = []
    if a.against:
        order.append(('parent_plain', 'plain', [], dict(script=os.path.join(os.path.abspath(a.against), 'tools', 'shared_prune_record.py'))))
    order += [('plain', 'plain', [], {}), ('shrink', 'shrink', [], {})]
    order += [('online_r%d' % r, 'online', ['--online-prune', str(a.online_prune), '--online-prune-rounds', str(r)], {}) for r in rounds]
    order += [('idle_off', 'plain', idle, dict(steps=a.idle_steps)),
              ('idle_on', 'online', idle + ['--online-prune', str(a.idle_capacity - 1), '--online-prune-rounds', str(rounds[len(rounds) // 2])],
               dict(steps=a.idle_steps))]
    rec = dict(scenario=SCENARIO, replicas=a.replicas, steps=a.steps, budget=BUDGET, max_rounds=MAX_ROUNDS, capacity=CAPACITY,
               idle_capacity=a.idle_capacity, idle_steps=a.idle_steps, target=a.online_prune, rounds_of_all_modes=0,
               statistic='alternating runs per mode (rounds_of_all_modes of them), one MI355X; ms per step: wall, fetch of the violations '
               'included, median and range over the runs', modes={label: dict(runs=[]) for label, _, _, _ in order})
    t_start = time.perf_counter()
    for _ in range(a.repeat):
        t_round = time.perf_counter()
        for label, mode, extra, kw in order:
            out = run(mode, a, extra, **kw)
            w = out['windows']
            out['ms_per_step_all'] = sum(x['ms_per_step'] for x in w) / len(w)
            late = [x['ms_per_step'] for x in w if x['steps'][0] >= 200] or [x['ms_per_step'] for x in w]
            out['ms_per_step_from_step_200'] = sum(late) / len(late)
            out.setdefault('largest_dictionary', max(max(x['dictionary_sizes']) for x in w))
            rec['modes'][label]['runs'].append(out)
            _summaries(rec, a)
            with open(a.out or ONLINE_OUT, 'w') as f:
                json.dump(rec, f, indent=1)
                f.write('\n')
            print(json.dumps(dict(mode=label, ms_per_step_all=out['ms_per_step_all'], ms_from_200=out['ms_per_step_from_step_200'],
                                  largest=out['largest_dictionary'], info=out.get('online_prune_info'))), flush=True)
        rec['rounds_of_all_modes'] += 1
        now = time.perf_counter()
        if a.time_budget and (now - t_start) + (now - t_round) > a.time_budget:
            break
    _summaries(rec, a)
    with open(a.out or ONLINE_OUT, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(rounds_of_all_modes=rec['rounds_of_all_modes'], idle=rec.get('idle'))), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', dest='mode')
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1400)
    ap.add_argument('--target', type=int, default=768)
    ap.add_argument('--every', type=int, default=200)
    ap.add_argument('--shared-plus', action='store_true', help='the rounds learn by the margin rule (kb_set_shared_plus)')
    ap.add_argument('--shared-plus-batch', type=int, default=0, metavar='M',
                    help='with --shared-plus: growing dictionaries of M landmarks or more take their lists in segments (kb_set_shared_plus_batch)')
    ap.add_argument('--online-prune', type=int, default=0, metavar='T',
                    help='the budget stage inside the step at target T (kb_set_shared_online_prune); never together with the periodic shrink')
    ap.add_argument('--online-prune-rounds', default='2', metavar='R', help='its rounds; a comma-separated list runs one mode each')
    ap.add_argument('--repeat', type=int, default=3, help='with --online-prune: alternating runs per mode')
    ap.add_argument('--capacity', type=int, default=CAPACITY, help='(a child of --online-prune: the idle pair runs at --idle-capacity)')
    ap.add_argument('--idle-capacity', type=int, default=4096)
    ap.add_argument('--idle-steps', type=int, default=100)
    ap.add_argument('--against', default='', metavar='DIR', help='with --online-prune: a built checkout of the parent commit, measured as parent_plain')
    ap.add_argument('--time-budget', type=float, default=0.0, metavar='S', help='with --online-prune: begin no further round of all modes beyond S seconds')
    ap.add_argument('--timeout', type=int, default=400)
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    if a.online_prune and a.mode == 'shrink':
        raise SystemExit('--online-prune holds the budget inside the step: it is never combined with the periodic shrink')
    if (a.mode == 'online') != bool(a.online_prune and a.mode):
        raise SystemExit('--child online wants --online-prune T, and --online-prune in a child wants --child online')
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    if a.mode:
        return child(a)
    if a.online_prune:
        if a.steps % WINDOW or a.every % WINDOW or a.idle_steps % WINDOW:
            raise SystemExit('--steps, --every and --idle-steps must be multiples of %d' % WINDOW)
        return online_record(a)
    a.out = a.out or os.path.join(ROOT, 'profiles', 'shared_prune_record.json')
    if a.steps % WINDOW or a.every % WINDOW:
        raise SystemExit('--steps and --every must be multiples of %d' % WINDOW)
    rec = dict(scenario=SCENARIO, budget=BUDGET, max_rounds=MAX_ROUNDS, capacity=CAPACITY, statistic='one run per mode, one MI355X')
    if a.shared_plus:
        rec['shared_plus'] = True
    if a.shared_plus_batch:
        rec['shared_plus_batch'] = a.shared_plus_batch
    for mode in ('plain', 'shrink'):   # (one after the other: never two processes on the GPU at once)
        rec[mode] = run(mode, a)
        print(json.dumps({k: v for k, v in rec[mode].items() if k != 'windows'}), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
