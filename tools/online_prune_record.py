#!/usr/bin/env python3
"""What the online budget (kb_set_online_prune) costs and buys: profiles/online_prune_record.json.

  python tools/online_prune_record.py [--envs 4096] [--grow 3000] [--window 200] [--reps 3] [--against TREE]
      [--out profiles/online_prune_record.json]

--envs replicas of scenario 0 learn in the captured resident loop up to step --grow.  Every arm then runs on a FORK of that
fleet (kb_fork + rs_fork: the same --window steps from the same state), 10 steps of warm-up (the capture), then the window
between two host waits; ms per closed-loop step = wall time of the window / its steps, simulator step included.
  off        the switch off, captured and plain; and the update / select phases (kb_phase_times_ms, kernel timing on, plain)
  empty      the switch on with a target above every size (capacity - 64): the price of launches that find nothing, rounds 2 and 8
  binding    target 256, captured.  HOLDING the budget: every arm's fork is first brought to the target by one kb_prune (outside
             the window), then: no budget at all; the stage at rounds 2 and 8; kb_prune between stretches of 1 step and of 100
             steps (the only ways to comparable states without the switch) -- removals, sizes at the end, the stage's counters.
             CATCHING UP: the stage alone from the fleet as it is, dictionaries far above the target, rounds 2, 8 and 64
--against TREE: a built checkout of the commit to compare with (its package and library are used by a child process): the
`off` arm of both, alternating, --reps rounds each -- "unchanged" is inside the spread of TREE's own rounds.
A run without a GPU fails; nothing here falls back."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fleet(tree, n, capacity, pool_gb, seed):
    sys.path.insert(0, os.path.join(tree, 'network-slicing_amd'))
    import ctypes as C
    import numpy as np
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice, default_fading
    cfg = make_config(0, n_envs=n)
    dims, n_prbs = [10] * cfg.n_embb, cfg.n_prbs

    def pair():
        return (VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=default_fading(), seed=seed),
                VecKBRL(n, dims, n_prbs, capacity=capacity, pool_bytes=int(pool_gb * 2 ** 30)))
    env, ag = pair()
    fenv, fag = pair()
    ia = np.full((n, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32)
    sf = np.full((n, len(dims)), 3, dtype=np.int32)
    env.reset()
    fenv.reset()
    ag.reset(ia, sf)
    fag.reset(ia, sf)
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    return env, ag, fenv, fag, np.arange(n, dtype=np.int32)


def _grow(env, ag, steps):
    t0 = time.perf_counter()
    done = 0
    while done < steps:
        k = min(500, steps - done)
        ag.run_resident(env, k, graph=True)
        ag.synchronize()
        done += k
        print('step %d, %.1f s' % (done, time.perf_counter() - t0), file=sys.stderr, flush=True)
    return time.perf_counter() - t0


def _window(env, ag, fenv, fag, everyone, window, graph, setup=None, between=None, stretch=None):
    """fork, setup(fag), 10 steps, then `window` steps timed between two host waits (in stretches with between(fag) behind each,
    for the host-driven arms) -> ms per step"""
    fag.fork_from(ag, everyone)
    fenv.fork_from(env, everyone)
    if setup:
        setup(fag)
    fag.run_resident(fenv, 10, graph=graph)
    if between:
        between(fag)
    fag.synchronize()
    fenv.synchronize()
    t0 = time.perf_counter()
    done = 0
    while done < window:
        k = min(stretch or window, window - done)
        fag.run_resident(fenv, k, graph=graph)
        done += k
        if between:
            between(fag)
    fag.synchronize()
    fenv.synchronize()
    return 1e3 * (time.perf_counter() - t0) / window


def _phases(env, ag, fenv, fag, everyone, window, setup=None):
    fag.fork_from(ag, everyone)
    fenv.fork_from(env, everyone)
    if setup:
        setup(fag)
    fag.run_resident(fenv, 10, graph=False)
    fag.set_kernel_timing(True)
    fag.phase_times_ms()
    fag.run_resident(fenv, window, graph=False)
    fag.synchronize()
    ph = fag.phase_times_ms()
    fag.set_kernel_timing(False)
    return dict(update_ms=ph['update_ms'], select_ms=ph['select_ms'])


def _summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def leg_off(args, tree):
    """the switch off (the only arm a tree without the switch can run)"""
    env, ag, fenv, fag, everyone = _fleet(tree, args.envs, args.capacity, args.pool_gb, args.seed)
    grow_s = _grow(env, ag, args.grow)
    sizes = ag.dictionary_sizes()
    cap, plain, ph = [], [], []
    for _ in range(args.reps):
        cap.append(_window(env, ag, fenv, fag, everyone, args.window, True))
        plain.append(_window(env, ag, fenv, fag, everyone, args.window, False))
        ph.append(_phases(env, ag, fenv, fag, everyone, min(args.window, 50)))
    out = dict(tree=os.path.relpath(tree, ROOT), grow_s=grow_s, landmarks_mean=float(sizes.mean()), landmarks_max=int(sizes.max()),
               step_ms_captured=_summary(cap), step_ms_plain=_summary(plain),
               update_ms=_summary([p['update_ms'] for p in ph]), select_ms=_summary([p['select_ms'] for p in ph]))
    for h in (env, ag, fenv, fag):
        h.close()
    return out


def leg_arms(args):
    env, ag, fenv, fag, everyone = _fleet(ROOT, args.envs, args.capacity, args.pool_gb, args.seed)
    grow_s = _grow(env, ag, args.grow)
    sizes = ag.dictionary_sizes()
    W, above, bind = args.window, args.capacity - 64, args.bind
    out = dict(grow_s=grow_s, steps=[args.grow + 10, args.grow + 10 + W], landmarks_mean=float(sizes.mean()), landmarks_max=int(sizes.max()),
               dictionaries_above_the_binding_target=int((sizes > bind).sum()))
    assert sizes.max() <= above, 'a dictionary is above capacity - 64: the empty arm would not be empty'
    on = lambda t, r: (lambda a: a.set_online_prune(t, r))
    off = lambda a: a.set_online_prune(0)
    empty = {}
    for rep in range(args.reps):          # (the arms alternate inside a repetition)
        for name, setup in (('off', off), ('rounds_2', on(above, 2)), ('rounds_8', on(above, 8))):
            for graph in (True, False):
                empty.setdefault('%s_%s' % (name, 'captured' if graph else 'plain'), []).append(
                    _window(env, ag, fenv, fag, everyone, W, graph, setup=setup))
        assert fag.online_prune_info()['removed'] == 0
    out['empty'] = {k: _summary(v) for k, v in empty.items()}
    for r in (2, 8):
        for how in ('captured', 'plain'):
            out['empty']['added_ms_per_step_rounds_%d_%s' % (r, how)] = (statistics.median(empty['rounds_%d_%s' % (r, how)]) -
                                                                         statistics.median(empty['off_%s' % how]))
    binding = {}
    state = {}

    def end_state(a, key):
        z = a.dictionary_sizes()
        state[key] = dict(landmarks_mean=float(z.mean()), landmarks_max=int(z.max()), landmarks_pruned=int(a.pruned().sum()),
                          info=a.online_prune_info())
    prune = lambda a: a.prune(bind)

    def held(setup):       # (the fork at the target before anything is timed, and its counters at zero as a fork leaves them)
        def go(a):
            off(a)
            a.prune(bind)
            setup(a)
        return go
    for rep in range(args.reps):
        for key, kw in (('no_budget', dict(setup=held(off))),
                        ('online_rounds_2', dict(setup=held(on(bind, 2)))), ('online_rounds_8', dict(setup=held(on(bind, 8)))),
                        ('prune_every_1', dict(setup=held(off), between=prune, stretch=1)),
                        ('prune_every_100', dict(setup=held(off), between=prune, stretch=100))):
            binding.setdefault(key, []).append(_window(env, ag, fenv, fag, everyone, W, True, **kw))
            end_state(fag, key)
    out['binding'] = {k: dict(step_ms=_summary(v), **state[k]) for k, v in binding.items()}
    out['binding']['note'] = ('landmarks_pruned counts the kb_prune that brought the fork to the target as well; the stage\'s own '
                              'removals are info.removed (warm-up and window: %d steps)' % (W + 10))
    for key in ('online_rounds_2', 'online_rounds_8', 'prune_every_1', 'prune_every_100'):
        out['binding'][key]['added_ms_per_step_over_no_budget'] = statistics.median(binding[key]) - statistics.median(binding['no_budget'])
    out['binding']['phases_no_budget'] = _phases(env, ag, fenv, fag, everyone, min(W, 50), setup=held(off))
    out['binding']['phases_online_rounds_2'] = _phases(env, ag, fenv, fag, everyone, min(W, 50), setup=held(on(bind, 2)))
    catch = {}
    for r in (2, 8, 64):
        ms = _window(env, ag, fenv, fag, everyone, W, True, setup=on(bind, r))
        end_state(fag, 'catch')
        catch['rounds_%d' % r] = dict(step_ms=ms, **state['catch'])
    catch['unbudgeted_step_ms'] = statistics.median(empty['off_captured'])
    out['catching_up'] = catch
    for h in (env, ag, fenv, fag):
        h.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--grow', type=int, default=3000)
    ap.add_argument('--window', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--capacity', type=int, default=4096, help='above every size at --grow: the empty arm\'s target is capacity - 64')
    ap.add_argument('--bind', type=int, default=256, help='the binding arm\'s target')
    ap.add_argument('--pool-gb', type=float, default=40.0, help='per handle (two are alive: the fleet and its fork)')
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--against', default=None, help='a built checkout of the commit to compare the switched-off loop with')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'online_prune_record.json'))
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)      # child processes: 'off:TREE' or 'arms'
    args = ap.parse_args()
    if args.leg:
        res = leg_off(args, args.leg[4:]) if args.leg.startswith('off:') else leg_arms(args)
        print('RECORD ' + json.dumps(res), flush=True)
        return
    base = [sys.executable, os.path.abspath(__file__)] + [a for a in sys.argv[1:]]

    def child(leg):
        t0 = time.perf_counter()
        p = subprocess.run(base + ['--leg', leg], stdout=subprocess.PIPE, text=True, check=True, timeout=600)   # (a failed or hung leg ends the run)
        line = [l for l in p.stdout.splitlines() if l.startswith('RECORD ')][-1]
        print('%s: %.0f s' % (leg, time.perf_counter() - t0), file=sys.stderr, flush=True)
        return json.loads(line[7:])
    record = dict(command='python tools/online_prune_record.py ' + ' '.join(sys.argv[1:]), envs=args.envs, capacity=args.capacity,
                  grow=args.grow, window=args.window, reps=args.reps)

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(record, f, indent=1)
            f.write('\n')
    if args.against:
        rounds = []
        for _ in range(args.reps):        # one process per round and tree, alternating
            rounds.append(dict(parent=child('off:' + os.path.abspath(args.against)), this=child('off:' + ROOT)))
        record['off_against_parent'] = dict(rounds=rounds)
        for key in ('step_ms_captured', 'step_ms_plain', 'update_ms', 'select_ms'):
            p = [r['parent'][key]['median'] for r in rounds]
            t = [r['this'][key]['median'] for r in rounds]
            record['off_against_parent'][key] = dict(parent=p, this=t, parent_spread=[min(p), max(p)],
                                                     inside_the_parents_spread=bool(min(p) <= statistics.median(t) <= max(p)))
        save()
    record['arms'] = child('arms')
    save()
    print(json.dumps(record))


if __name__ == '__main__':
    main()
