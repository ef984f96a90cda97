#!/usr/bin/env python3
"""BASELINE config 3 at the REFERENCE's run length (experiments_kbrl.py:22: 50,400 steps): N replicas of scenario_0 with one
KBRL agent each, closed loop on the device, the dictionary pool sized from the device's free memory -- how many replicas of
one GPU get through a run of that length without a dictionary that had to project for want of storage?

  python tools/run_length.py [--envs 2048] [--steps 50400] [--budget-s 900] [--profile tdl] [--prune-to T --prune-every P]
      [--online-prune T [--online-prune-rounds R]] > profiles/<tag>_run_length.txt
Prints one progress line per --report steps and a JSON summary: steps done, wall time, env-steps/s over the whole run and over
the last window, dictionary sizes, pool use (its peak too), violations per step and mean PRBs, replicas flagged (kb_get_flags:
capacity / pool).  Stops early at --budget-s.  --prune-to T --prune-every P: budgeted dictionaries -- every P steps the
dictionaries above T landmarks are pruned back to T (kb_prune), between two resident stretches.  --online-prune T: the same
budget held inside the loop instead -- a budget stage behind every step's update phase takes up to R landmarks from every
dictionary above T (kb_set_online_prune); the stretches are not cut and the summary adds the stage's counters.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
import numpy as np  # noqa: E402
from ranslice import _lib  # noqa: E402
from ranslice.config import make_config, EMBB_A, EMBB_SEC  # noqa: E402
from ranslice.fading import synth_traces  # noqa: E402
from ranslice.kbrl_dev import VecKBRL  # noqa: E402
from ranslice.vec_env import VecRanSlice  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=2048)
    ap.add_argument('--steps', type=int, default=50400)
    ap.add_argument('--report', type=int, default=4200)
    ap.add_argument('--chunk', type=int, default=600)
    ap.add_argument('--capacity', type=int, default=16384)
    ap.add_argument('--headroom-gb', type=float, default=24.0)
    ap.add_argument('--budget-s', type=float, default=900.0)
    ap.add_argument('--profile', default='tdl')
    ap.add_argument('--history', action='store_true', help='record the per-step histories on the device (26 bytes per replica and step) '
                                                           'and report violations per step and mean PRBs')
    ap.add_argument('--prune-to', type=int, default=None)
    ap.add_argument('--prune-every', type=int, default=None)
    ap.add_argument('--online-prune', type=int, default=None, metavar='T')
    ap.add_argument('--online-prune-rounds', type=int, default=2, metavar='R')
    args = ap.parse_args()
    if (args.prune_to is None) != (args.prune_every is None):
        ap.error('--prune-to and --prune-every go together')
    if args.online_prune is not None and args.prune_to is not None:
        ap.error('--online-prune and --prune-to / --prune-every are two ways to hold one budget: give one')
    import ctypes as C
    N = args.envs
    cfg = make_config(0, n_envs=N)
    env = VecRanSlice(n_envs=N, cfg=cfg, fading=synth_traces(10000, args.profile))
    free, total = _lib.device_mem_info(0)
    pool_bytes = _lib.default_pool_bytes(0, headroom=int(args.headroom_gb * 2 ** 30))
    agent = VecKBRL(N, [10] * 5, cfg.n_prbs, accuracy_range=(0.99, 0.999), capacity=args.capacity, pool_bytes=pool_bytes,
                    online_prune=args.online_prune, online_prune_rounds=args.online_prune_rounds)
    rng = np.random.default_rng(0)
    ia = rng.integers(EMBB_A[0], EMBB_A[1], size=(N, 5)).astype(np.int32)   # scenario_creator.py:220-221
    sf = rng.integers(EMBB_SEC[0], EMBB_SEC[1], size=(N, 5)).astype(np.int32)
    env.reset()
    agent.reset(ia, sf)
    if args.history:
        agent.history_begin(args.steps)
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    print('# %d replicas x %d steps, scenario_0 + one KBRL agent per replica (%s traces); device memory %.1f GB free of %.1f, pool %.1f GB, capacity %d'
          % (N, args.steps, args.profile, free / 1e9, total / 1e9, pool_bytes / 1e9, args.capacity), flush=True)
    t0 = time.perf_counter()
    done, last_t, last_done = 0, t0, 0
    windows = []
    removed, peak_pool = 0, 0
    while done < args.steps:
        k = min(args.chunk, args.steps - done)
        if args.prune_every:
            k = min(k, args.prune_every - done % args.prune_every)
        agent.run_resident(env, k, graph=True)
        done += k
        if args.prune_every and done % args.prune_every == 0 and done < args.steps:
            removed += agent.prune(args.prune_to)
        if done % args.report == 0 or done == args.steps:
            env.synchronize()
            agent.synchronize()
            now = time.perf_counter()
            sizes = agent.dictionary_sizes()
            pool = agent.pool()
            w = dict(step=done, wall_s=now - t0, ms_per_step=1e3 * (now - last_t) / (done - last_done),
                     env_steps_per_s=N * (done - last_done) / (now - last_t), dict_mean=float(sizes.mean()), dict_max=int(sizes.max()),
                     pool_used_gb=pool['used_bytes'] / 1e9, saturated=pool['saturated'], pool_full=pool['pool_full'])
            peak_pool = max(peak_pool, pool['used_bytes'])
            if args.prune_every:
                w['pruned_so_far'] = removed
            if args.online_prune is not None:
                w['pruned_so_far'] = int(agent.pruned().sum())
            windows.append(w)
            print('step %6d  %7.1f s  %.3f ms/step  %.3g env-steps/s  dictionaries mean %.0f max %d  pool %.1f GB  flagged: capacity %d pool %d'
                  % (done, w['wall_s'], w['ms_per_step'], w['env_steps_per_s'], w['dict_mean'], w['dict_max'], w['pool_used_gb'],
                     w['saturated'], w['pool_full']), flush=True)
            last_t, last_done = now, done
            if now - t0 > args.budget_s:
                break
    env.synchronize()
    agent.synchronize()
    wall = time.perf_counter() - t0
    fl = agent.flagged_replicas()
    out = env.fetch()
    assert np.isfinite(out['reward']).all()
    viol = prbs = None
    if args.history:   # KBRL_Control.run's history columns of the whole run: violations per step and the mean PRBs handed out
        h = agent.history_fetch()
        rec = h['recorded']
        viol = float(h['violation'][:, :rec].mean())
        prbs = float(h['resources'][:, :rec].mean())
    online = agent.online_prune_info() if args.online_prune is not None else None
    if online:
        removed = online['removed']
        online['replicas_flagged_unpruned'] = int((agent.flags() & 32 != 0).sum())
    print(json.dumps({'replicas': N, 'steps_done': done, 'steps_asked': args.steps, 'wall_s': wall, 'env_steps_per_s_whole_run': N * done / wall,
                      'ms_per_step_whole_run': 1e3 * wall / done, 'last_window': windows[-1] if windows else None,
                      'pool_bytes': pool_bytes, 'peak_pool_bytes': max(peak_pool, agent.pool()['used_bytes']),
                      'violations_per_step': viol, 'mean_prbs': prbs,
                      'prune_to': args.prune_to, 'prune_every': args.prune_every, 'online_prune': args.online_prune, 'online_prune_rounds': args.online_prune_rounds if online else None,
                      'online_prune_info': online, 'landmarks_pruned': removed, 'replicas_flagged_capacity': len(fl['saturated']), 'replicas_flagged_pool': len(fl['pool_full']),
                      'replicas_unflagged': N - len(set(fl['saturated']) | set(fl['pool_full']))}))
    env.close()
    agent.close()


if __name__ == '__main__':
    main()
