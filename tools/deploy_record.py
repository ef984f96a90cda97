#!/usr/bin/env python3
"""Measures the agent fork and the deployed (inference-only) replicas and writes profiles/deploy_record.json:

  * closed-loop env-steps/s of 4096 replicas of scenario 0 steered by 30 agents trained for 3,000 steps and fanned out -- in
    learning mode and in inference mode, on the same full fork (kb_fork) in the same process; the inference step launches a
    strict subset of the learning step's kernels, so it must not be the slower one;
  * the same in inference mode at 65,536 deployed replicas (kb_deploy), with the bytes of their pool;
  * what kb_fork and kb_deploy cost for the 4096-agent fan-out: time, bytes read + written (the shells, from the scan's total
    as kb_get_pool reports it), GB/s -- beside rs_fork's figure in profiles/clairvoyant_record.json for orientation.

  python tools/deploy_record.py [--train-steps 3000] [--steps 200] [--big 65536] [--experiment 40000 64 9500] [--fanout-only]
                                [--out profiles/deploy_record.json]

--fanout-only: train, fan out once with each call and exit (the run to put under `rocprofv3 --kernel-trace --stats`).

--by-reference [--ref-sizes 4096 65536]: the fan-out by reference (kb_deploy_ref) against the copy (kb_deploy), the same trained
agents in the same process, and nothing else; writes profiles/deploy_ref_record.json.  Per size and per kind: the bytes of the
pool, the device memory the handle took (free memory before and after the call), closed-loop inference ms per step (hipGraph)
and the select phase's ms (kb_phase_times_ms, plain launches) -- over --ref-repeats rounds in which the two kinds alternate in
going first, every round's figure with min / median / max.  With one size and one round it is the run to put under rocprofv3.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))


def fresh_env(scenario, n, action, device=0):
    """n replicas on seeds of their own, one step under `action` behind them (KBRL_Control.run's first step)"""
    from ranslice import config as _c
    from ranslice.vec_env import VecRanSlice, default_fading
    import experiments_trained as et
    env = VecRanSlice(n_envs=n, cfg=_c.make_config(scenario, n_envs=n), fading=default_fading(), device=device)
    env.reset(seeds=et.eval_seeds(n))
    env.enqueue_step(action)
    return env


def rate(agent, env, steps, warm=20):
    agent.run_resident(env, warm, graph=True)
    agent.synchronize()
    env.synchronize()
    t0 = time.perf_counter()
    agent.run_resident(env, steps, graph=True)
    agent.synchronize()
    env.synchronize()
    dt = time.perf_counter() - t0
    return dict(env_steps_per_s=env.n_envs * steps / dt, ms_per_step=1e3 * dt / steps, steps=steps)


def timed(call, sync):
    t0 = time.perf_counter()
    out = call()
    sync(out)
    return out, time.perf_counter() - t0


def by_reference_leg(agent, scenario, sizes_n, steps, repeats=3):
    """copy against by-reference at every size of `sizes_n`: `repeats` rounds, each round both kinds on a fresh deployment and a
    fresh fleet, the kind that goes first alternating from round to round.  Per kind the record keeps every round's closed-loop
    ms per step and select-phase ms with their min, median and max; the ratios are formed from the medians.
    -> {size: {copy: ..., by_reference: ..., by_reference_over_copy: ...}}"""
    from ranslice import _lib
    from ranslice.kbrl_dev import deploy_pool_bytes, deploy_ref_pool_bytes
    n = agent.n_envs
    sizes = agent.dictionary_sizes()

    def spread(v):
        return dict(runs=[float(x) for x in v], min=float(min(v)), median=float(np.median(v)), max=float(max(v)))
    out = {}
    for N in sizes_n:
        index = (np.arange(N) % n).astype(np.int32)
        runs = {'copy': [], 'by_reference': []}
        failed = {}
        for rep in range(repeats):
            for kind in (('copy', 'by_reference') if rep % 2 == 0 else ('by_reference', 'copy')):
                try:
                    agent.synchronize()
                    free0, _ = _lib.device_mem_info(0)
                    dep, t_dep = timed(lambda: agent.deploy(index, by_reference=kind == 'by_reference'), lambda d: d.synchronize())
                    free1, _ = _lib.device_mem_info(0)
                    pool = dep.pool()
                    want = deploy_ref_pool_bytes(sizes, index) if kind == 'by_reference' else deploy_pool_bytes(sizes[index])
                    assert pool['used_bytes'] == pool['total_bytes'] == want, (kind, pool, want)
                    env = fresh_env(scenario, N, dep.control(with_accuracies=False)['action'])
                    r = rate(dep, env, steps)
                    dep.set_kernel_timing(True)       # (timed launches go one by one: the graph is not used)
                    dep.run_resident(env, 10, graph=False)
                    dep.synchronize()
                    dep.phase_times_ms()
                    dep.run_resident(env, 40, graph=False)
                    dep.synchronize()
                    ph = dep.phase_times_ms()
                    dep.set_kernel_timing(False)
                    runs[kind].append(dict(pool_bytes=pool['used_bytes'], device_memory_taken_bytes=int(free0 - free1),
                                           deploy_wall_ms=1e3 * t_dep, ms_per_step=r['ms_per_step'], select_phase_ms=ph['select_ms'],
                                           select_phases_timed=int(ph['n_select'])))
                    env.close()
                    dep.close()
                except Exception as e:      # recorded, not hidden
                    failed[kind] = repr(e)
        leg = {}
        for kind, rs in runs.items():
            if kind in failed or not rs:
                leg[kind] = dict(failed=failed.get(kind, 'no run'))
                continue
            leg[kind] = dict(pool_bytes=rs[0]['pool_bytes'], steps=steps, select_phases_timed=rs[0]['select_phases_timed'],
                             device_memory_taken_bytes=spread([x['device_memory_taken_bytes'] for x in rs]),
                             deploy_wall_ms=spread([x['deploy_wall_ms'] for x in rs]),
                             ms_per_step=spread([x['ms_per_step'] for x in rs]),
                             select_phase_ms=spread([x['select_phase_ms'] for x in rs]))
        if all('failed' not in v for v in leg.values()):
            leg['by_reference_over_copy'] = dict(
                pool_bytes=leg['by_reference']['pool_bytes'] / leg['copy']['pool_bytes'],
                **{k: leg['by_reference'][k]['median'] / leg['copy'][k]['median']
                   for k in ('device_memory_taken_bytes', 'ms_per_step', 'select_phase_ms')})
        out[str(N)] = dict(leg, order='copy first in rounds 0, 2, ..; by reference first in rounds 1, 3, ..', rounds=repeats)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenario', type=int, default=0)
    ap.add_argument('--agents', type=int, default=30)
    ap.add_argument('--train-steps', type=int, default=3000)
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--big', type=int, default=65536)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--fanout-only', action='store_true')
    ap.add_argument('--experiment', type=int, nargs=3, metavar=('TRAIN_STEPS', 'EVAL_REPLICAS', 'EVAL_STEPS'), default=None,
                    help='also run experiments_trained.train_and_deploy for the scenario and record its numbers (e.g. 40000 64 9500)')
    ap.add_argument('--by-reference', action='store_true',
                    help='measure kb_deploy_ref against kb_deploy only, and write profiles/deploy_ref_record.json')
    ap.add_argument('--ref-sizes', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--ref-repeats', type=int, default=3, help='rounds of the --by-reference leg (the two kinds alternate in going first)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, 'profiles', 'deploy_ref_record.json' if args.by_reference else 'deploy_record.json')
    import scenario_creator as sc
    from experiments_kbrl import BatchedEvaluator
    from ranslice.kbrl_dev import VecKBRL, deploy_pool_bytes, fork_pool_bytes
    n, N = args.agents, args.replicas
    ev = BatchedEvaluator(args.scenario, [0.99, 0.999], steps=args.train_steps, out_dir=tempfile.mkdtemp(prefix='deploy_record_'))
    t0 = time.perf_counter()
    agent, _ = ev.train(range(n), pool_bytes=8 << 30, graph=True)
    agent.synchronize()
    rec = dict(scenario=args.scenario, agents=n, train_steps=args.train_steps, train_wall_s=time.perf_counter() - t0, replicas=N)
    sizes = agent.dictionary_sizes()
    rec['dictionary'] = dict(max=int(sizes.max()), mean=float(sizes.mean()))
    if args.by_reference:
        del rec['replicas']
        rec['sizes'] = by_reference_leg(agent, args.scenario, args.ref_sizes, args.steps, args.ref_repeats)
        ev.release()
        with open(args.out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')
        print(json.dumps(rec, sort_keys=True))
        return
    index = (np.arange(N) % n).astype(np.int32)
    need = fork_pool_bytes(sizes[index])
    full = VecKBRL(N, agent.dims, agent.n_prbs, alfa=sc.alfa, accuracy_range=(0.99, 0.999), capacity=agent.capacity,
                   pool_bytes=need + (16 << 30))     # room to keep learning in
    # ---- gather cost (the second call of each: the first pays for the lazily created buffers)
    full.fork_from(agent, index)
    full.synchronize()
    _, t_fork = timed(lambda: full.fork_from(agent, index), lambda _: full.synchronize())
    d0 = agent.deploy(index)
    d0.synchronize()
    d0.close()
    dep, t_dep = timed(lambda: agent.deploy(index), lambda d: d.synchronize())
    moved_fork = 2 * (full.pool()['used_bytes'] - 512)
    moved_dep = 2 * (dep.pool()['used_bytes'] - 512)
    assert full.pool()['used_bytes'] == need and dep.pool()['used_bytes'] == deploy_pool_bytes(sizes[index])
    rec['gather'] = dict(
        kb_fork=dict(wall_ms=1e3 * t_fork, shell_bytes_read_plus_written=moved_fork, gb_per_s=moved_fork / t_fork / 1e9),
        kb_deploy=dict(wall_ms=1e3 * t_dep, shell_bytes_read_plus_written=moved_dep, gb_per_s=moved_dep / t_dep / 1e9,
                       note='wall time of the whole call: creating the handle (its allocations and memsets) included'))
    try:
        cr = json.load(open(os.path.join(ROOT, 'profiles', 'clairvoyant_record.json')))
        rec['gather']['rs_fork_for_orientation'] = cr['fork_kernel']
    except Exception:
        pass
    if args.fanout_only:
        print(json.dumps(rec['gather']))
        return
    # ---- closed-loop rates at N replicas: learning, then the same fork again in inference mode
    a0 = full.control(with_accuracies=False)['action']
    env = fresh_env(args.scenario, N, a0)
    rec['learning'] = rate(full, env, args.steps)
    env.close()
    full.fork_from(agent, index)
    full.set_learning(False)
    env = fresh_env(args.scenario, N, a0)
    rec['inference_full_fork'] = rate(full, env, args.steps)
    env.close()
    full.close()
    env = fresh_env(args.scenario, N, a0)
    rec['inference_deployed'] = dict(rate(dep, env, args.steps), pool=dep.pool())
    env.close()
    dep.close()
    rec['inference_not_slower_than_learning'] = bool(rec['inference_full_fork']['ms_per_step'] <= rec['learning']['ms_per_step'])
    # ---- inference at `big` deployed replicas: a learning handle of this size does not fit the device
    B = args.big
    try:
        bindex = (np.arange(B) % n).astype(np.int32)
        big = agent.deploy(bindex)
        env = fresh_env(args.scenario, B, big.control(with_accuracies=False)['action'])
        rec['inference_big'] = dict(rate(big, env, max(20, args.steps // 4)), replicas=B, pool=big.pool(),
                                    learning_pool_would_be_bytes=fork_pool_bytes(sizes[bindex]))
        env.close()
        big.close()
    except Exception as e:      # recorded, not hidden: the issue asks why when it does not fit or run
        rec['inference_big'] = dict(replicas=B, failed=repr(e))
    ev.release()
    if args.experiment:     # experiments_trained.py's two pairs of numbers for the scenario, both accuracy ranges
        import experiments_trained as et
        from experiments_kbrl import accuracy_list
        keep = ('accuracy_range', 'runs', 'train_steps', 'eval_replicas', 'eval_steps', 'window', 'train_wall_s', 'eval_wall_s',
                'deployed', 'training_window', 'learning_control', 'max_dictionary', 'deployed_pool_bytes')
        rec['experiment'] = []
        for a_range in accuracy_list:
            sm = et.train_and_deploy(args.scenario, a_range, range(args.agents), train_steps=args.experiment[0],
                                     eval_replicas=args.experiment[1], eval_steps=args.experiment[2],
                                     out_dir=tempfile.mkdtemp(prefix='deploy_record_'), verbose=False, learning_control=True)
            rec['experiment'].append({k: sm[k] for k in keep})
    with open(args.out, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(rec, sort_keys=True))
    if not rec['inference_not_slower_than_learning']:
        sys.exit('the inference step was slower than the learning step of the same run')


if __name__ == '__main__':
    main()
