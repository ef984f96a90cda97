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

  python tools/shared_prune_record.py [--replicas 4096] [--steps 1400] [--target 768] [--every 200] [--shared-plus]
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
    agent = SharedVecKBRL(n, dims, cfg.n_prbs, budget=BUDGET, max_rounds=MAX_ROUNDS, capacity=CAPACITY, shared_plus=a.shared_plus,
                          shared_plus_batch=a.shared_plus_batch or None)
    agent.reset(ia, sf, seeds=replica_seeds(7, 0, n))
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
        grown = now
        step = w0 + WINDOW
        if saturated_at is None and sizes.max() >= CAPACITY:
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
    if a.mode == 'shrink':
        pt = agent.prune_times_ms()
        out.update(shrinks=shrinks, target=a.target, every=a.every, downdate_bytes_read_plus_written=pt['downdate_bytes'],
                   downdate_launches_with_work=pt['downdate_launches'])
    agent.close()
    env.close()
    print(json.dumps(out))


def run(mode, a):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', mode, '--replicas', str(a.replicas),
           '--steps', str(a.steps), '--target', str(a.target), '--every', str(a.every)] + (['--shared-plus'] if a.shared_plus else []) + (
        ['--shared-plus-batch', str(a.shared_plus_batch)] if a.shared_plus_batch else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', dest='mode')
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=1400)
    ap.add_argument('--target', type=int, default=768)
    ap.add_argument('--every', type=int, default=200)
    ap.add_argument('--shared-plus', action='store_true', help='the rounds learn by the margin rule (kb_set_shared_plus)')
    ap.add_argument('--shared-plus-batch', type=int, default=0, metavar='M',
                    help='with --shared-plus: growing dictionaries of M landmarks or more take their lists in segments (kb_set_shared_plus_batch)')
    ap.add_argument('--timeout', type=int, default=400)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_prune_record.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    if a.mode:
        return child(a)
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
