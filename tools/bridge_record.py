#!/usr/bin/env python3
"""Measures the bridge between shared and per-replica KBRL handles (kb_unshare, kb_share) and writes
profiles/bridge_record.json.  No threshold is attached to any figure, and nothing is asserted about a ratio.

Two legs, each a child process of its own under `timeout`:
  timing  a shared-dictionary handle at the shape of the bench's config 4 (scenario index 2, --replicas (4096) replicas, budget
          256, capacity 1024, one exchange round per step, its own world) learns closed loop until its largest dictionary is at
          capacity (the bench calls that regime "saturated").  It is then unshared onto 1, 256 and 4,096 agents: device ms of the
          gather through one pair of HIP events, the bytes its work plan counts (read, written) and the TB/s they make, and the
          wall ms of the call.  The baseline, in the same process: kb_fork of the resulting handle into a third handle of the
          same size -- it writes the same bytes.  kb_fork has no event pair of its own, so it is timed as host wall ms (the call
          and a wait for the stream): the like-for-like pair is unshare_wall_ms against kb_fork_same_bytes_wall_ms, and
          gather_device_ms is the part of the former that is the gather.  Then one kb_share of agent 0 back into a fresh shared
          handle.
  use     what the bridge exists for.  Leg 1: the shared handle learns --pretrain (400) steps on --replicas replicas, is unshared
          onto --agents fresh environments and goes on learning per replica for --tail (200) steps.  Leg 2: as many agents learn
          from scratch for --pretrain + --tail steps on environments of the same seeds.  Recorded for the last --tail steps of
          both: SLA violations per step and PRBs allocated per step (means over agents and steps), and the dictionary sizes.
          Whether pre-training helps is a result; nothing is asserted.  (The unshared agents meet environments they have never
          seen: their first learning step pairs the shared fleet's last observation with the new environment's labels.)

  python tools/bridge_record.py [--replicas 4096] [--agents 4096] [--pretrain 400] [--tail 200] [--only timing|use]

--only LEG measures that leg alone and keeps the other as the record at --base (default: --out) holds it.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO, BUDGET, CAPACITY, FADING_COLS = 2, 256, 1024, 4096
AGENT_CAPACITY = 2048     # of the per-replica handles of the `use` leg: room to go on growing behind a full shared dictionary


def world(n, first_seed=0):
    """a config-4 environment of n replicas, its dims, and the reference's ranges of initial actions / security factors"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    from ranslice.config import make_config, EMBB_A, EMBB_SEC, MMTC_A, MMTC_SEC
    from ranslice.fading import synth_fading
    from ranslice.sharding import replica_seeds
    from ranslice.vec_env import VecRanSlice
    cfg = make_config(SCENARIO, n_envs=n)
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=[synth_fading(t, FADING_COLS) for t in range(3)])
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    rng = np.random.default_rng(1000)
    ia = np.concatenate([rng.integers(EMBB_A[0], EMBB_A[1], size=(n, cfg.n_embb)),
                         rng.integers(MMTC_A[0], MMTC_A[1], size=(n, cfg.n_mmtc))], axis=1).astype(np.int32)
    sf = np.concatenate([rng.integers(EMBB_SEC[0], EMBB_SEC[1], size=(n, cfg.n_embb)),
                         rng.integers(MMTC_SEC[0], MMTC_SEC[1], size=(n, cfg.n_mmtc))], axis=1).astype(np.int32)
    env.reset(seeds=replica_seeds(first_seed, 0, n))
    return env, cfg, dims, ia, sf


def first_step(env, actions):
    import numpy as np
    a = np.ascontiguousarray(actions, dtype=np.int32)
    env._check(env.L.rs_step(env.h, a.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))


def shared_fleet(n, steps=None, limit=800, shared_plus=False, shared_plus_batch=0):
    """-> (env, shared agent, steps run): `steps` closed-loop steps, or (None) until the largest dictionary is at capacity;
    shared_plus: the fleet learns by the margin rule (kb_set_shared_plus)"""
    from ranslice.kbrl_dev import SharedVecKBRL
    from ranslice.sharding import replica_seeds
    env, cfg, dims, ia, sf = world(n)
    agent = SharedVecKBRL(n, dims, cfg.n_prbs, budget=BUDGET, max_rounds=1, capacity=CAPACITY, shared_plus=shared_plus,
                          shared_plus_batch=shared_plus_batch or None)
    agent.reset(ia, sf, seeds=replica_seeds(7, 0, n))
    first_step(env, ia)
    done = 0
    while done < (steps if steps is not None else limit):
        k = 10 if steps is None else min(50, steps - done)
        for _ in range(k):
            agent.step_resident(env)
            env.step_resident()
        done += k
        if steps is None and int(agent.dictionary_sizes().max()) >= CAPACITY:
            break
    env.synchronize()
    agent.synchronize()
    return env, agent, done


def agents_like(shared, n, sizes, capacity=None):
    import numpy as np
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    c = shared.cfg
    return VecKBRL(n, shared.dims, shared.n_prbs, alfa=c.alfa, accuracy_range=(c.acc_lo, c.acc_hi), gamma=c.gamma, eta=c.eta,
                   capacity=capacity or shared.capacity, pool_bytes=fork_pool_bytes(np.tile(np.asarray(sizes, dtype=np.int64), (n, 1))))


def child_timing(a):
    import numpy as np
    from ranslice.kbrl_dev import SharedVecKBRL, shared_pool_bytes
    env, shared, steps = shared_fleet(a.replicas, shared_plus=a.shared_plus, shared_plus_batch=a.shared_plus_batch)
    sizes = shared.dictionary_sizes().astype(int)
    out = dict(replicas=a.replicas, steps_trained=steps, dictionary_sizes=sizes.tolist(),
               regime='saturated' if sizes.max() >= CAPACITY else 'filling', unshare=[])
    env.close()
    # first launches load code objects: a two-agent pass through every call that is timed below
    w1, w2 = agents_like(shared, 2, sizes), agents_like(shared, 2, sizes)
    w1.unshare_from(shared, [0, 1])
    w2.fork_from(w1, [0, 1])
    w3 = SharedVecKBRL(2, shared.dims, shared.n_prbs, budget=BUDGET, max_rounds=1, capacity=CAPACITY, gamma=shared.cfg.gamma)
    w3.share_from(w1, 0)
    for w in (w1, w2, w3):
        w.close()
    rng = np.random.default_rng(0)
    for n in (1, 256, 4096):
        index = rng.integers(0, a.replicas, n).astype(np.int32)
        dst, third = agents_like(shared, n, sizes), agents_like(shared, n, sizes)
        dst.set_kernel_timing(True)
        dst.synchronize()
        shared.synchronize()
        t0 = time.perf_counter()
        dst.unshare_from(shared, index)
        dst.synchronize()
        wall = 1e3 * (time.perf_counter() - t0)
        bt = dst.bridge_time_ms()
        third.synchronize()
        t0 = time.perf_counter()
        third.fork_from(dst, np.arange(n, dtype=np.int32))
        third.synchronize()
        fork_wall = 1e3 * (time.perf_counter() - t0)
        by = bt['read_bytes'] + bt['written_bytes']
        out['unshare'].append(dict(agents=n, gather_device_ms=bt['ms'], read_bytes=bt['read_bytes'], written_bytes=bt['written_bytes'],
                                   TBps_read_plus_written=by / bt['ms'] / 1e9 if bt['ms'] else None, unshare_wall_ms=wall,
                                   kb_fork_same_bytes_wall_ms=fork_wall, pool_used_bytes=dst.pool()['used_bytes'],
                                   same_dictionary_bytes_in_fork=bool(dst.learner(n - 1, 0, with_kinv=True)['kinv'].tobytes() ==
                                                                      third.learner(n - 1, 0, with_kinv=True)['kinv'].tobytes())))
        third.close()
        if n == 4096:
            back = SharedVecKBRL(a.replicas, shared.dims, shared.n_prbs, budget=BUDGET, max_rounds=1, capacity=CAPACITY, gamma=shared.cfg.gamma,
                                 pool_bytes=shared_pool_bytes(np.minimum(sizes + 128, CAPACITY)))
            back.set_kernel_timing(True)
            back.synchronize()
            t0 = time.perf_counter()
            back.share_from(dst, 0)
            back.synchronize()
            wall = 1e3 * (time.perf_counter() - t0)
            bt = back.bridge_time_ms()
            same = all(back.learner(0, s, with_kinv=True)['kinv'].tobytes() == shared.learner(0, s, with_kinv=True)['kinv'].tobytes()
                       for s in range(len(sizes)))
            out['share'] = dict(replicas=a.replicas, gather_device_ms=bt['ms'], read_bytes=bt['read_bytes'], written_bytes=bt['written_bytes'],
                                TBps_read_plus_written=(bt['read_bytes'] + bt['written_bytes']) / bt['ms'] / 1e9 if bt['ms'] else None,
                                share_wall_ms=wall, kinv_bytes_equal_to_the_shared_source=bool(same))
            back.close()
        dst.close()
    shared.close()
    print(json.dumps(out))


def tail_figures(agent, tail):
    h = agent.history_fetch()
    n = h['recorded']
    v, r = h['violation'][:, n - tail:n].astype(float), h['resources'][:, n - tail:n].astype(float)
    return dict(steps=[n - tail, n], violations_per_step=float(v.mean()), prbs_per_step=float(r.mean()))


def child_use(a):
    import numpy as np
    from ranslice.sharding import replica_seeds
    # leg 1
    env, shared, _ = shared_fleet(a.replicas, steps=a.pretrain, shared_plus=a.shared_plus, shared_plus_batch=a.shared_plus_batch)
    shared_sizes = shared.dictionary_sizes().astype(int)
    env.close()
    index = np.arange(a.agents, dtype=np.int32) % a.replicas
    env1, cfg, dims, ia, sf = world(a.agents, first_seed=1)
    ag = agents_like(shared, a.agents, np.minimum(shared_sizes + 192, AGENT_CAPACITY), capacity=AGENT_CAPACITY)
    ag.unshare_from(shared, index)
    shared.close()
    first_step(env1, ag.control(with_accuracies=False)['action'])
    ag.history_begin(a.tail)
    t0 = time.perf_counter()
    ag.run_resident(env1, a.tail)
    env1.synchronize()
    ag.synchronize()
    leg1 = dict(pretrain_steps=a.pretrain, shared_dictionary_sizes=shared_sizes.tolist(), tail_wall_s=time.perf_counter() - t0,
                **tail_figures(ag, a.tail))
    sz = ag.dictionary_sizes()
    leg1.update(dictionary_sizes_mean=sz.mean(axis=0).tolist(), dictionary_sizes_max=sz.max(axis=0).tolist(), pool=ag.pool())
    ag.close()
    env1.close()
    # leg 2: the same environments, agents that start empty
    env2, cfg, dims, ia, sf = world(a.agents, first_seed=1)
    from ranslice.kbrl_dev import VecKBRL
    from ranslice import _lib
    sc = VecKBRL(a.agents, dims, cfg.n_prbs, accuracy_range=(0.99, 0.999), capacity=AGENT_CAPACITY,
                 pool_bytes=_lib.default_pool_bytes(0, headroom=48 << 30))
    sc.reset(ia, sf, seeds=replica_seeds(7, 0, a.agents))
    first_step(env2, ia)
    total = a.pretrain + a.tail
    sc.history_begin(total)
    t0 = time.perf_counter()
    sc.run_resident(env2, total)
    env2.synchronize()
    sc.synchronize()
    leg2 = dict(steps_from_scratch=total, wall_s=time.perf_counter() - t0, **tail_figures(sc, a.tail))
    sz = sc.dictionary_sizes()
    leg2.update(dictionary_sizes_mean=sz.mean(axis=0).tolist(), dictionary_sizes_max=sz.max(axis=0).tolist(), pool=sc.pool())
    sc.close()
    env2.close()
    print(json.dumps(dict(replicas=a.replicas, agents=a.agents, tail_steps=a.tail, pretrained_then_unshared=leg1, from_scratch=leg2)))


def run(leg, a):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', leg, '--replicas', str(a.replicas),
           '--agents', str(a.agents), '--pretrain', str(a.pretrain), '--tail', str(a.tail)] + (['--shared-plus'] if a.shared_plus else []) + (
        ['--shared-plus-batch', str(a.shared_plus_batch)] if a.shared_plus_batch else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--pretrain', type=int, default=400)
    ap.add_argument('--tail', type=int, default=200)
    ap.add_argument('--shared-plus', action='store_true',
                    help='the shared fleet that is grown learns by the margin rule (kb_set_shared_plus); name another --out than the committed record')
    ap.add_argument('--shared-plus-batch', type=int, default=0, metavar='M',
                    help='with --shared-plus: growing dictionaries of M landmarks or more take their lists in segments (kb_set_shared_plus_batch)')
    ap.add_argument('--timeout', type=int, default=540)
    ap.add_argument('--only', choices=['timing', 'use'])
    ap.add_argument('--base', default=None, help='with --only: the record whose other leg is kept (default: --out)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'bridge_record.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    if a.child:
        return {'timing': child_timing, 'use': child_use}[a.child](a)
    rec = dict(scenario=SCENARIO, budget=BUDGET, shared_capacity=CAPACITY, statistic='one run per leg')
    if a.shared_plus:
        rec['shared_plus'] = True
    if a.shared_plus_batch:
        rec['shared_plus_batch'] = a.shared_plus_batch
    if a.only and os.path.exists(a.base or a.out):
        with open(a.base or a.out) as f:
            rec.update(json.load(f))
    if a.only != 'use':
        rec['timing'] = run('timing', a)
        print(json.dumps(rec['timing']), flush=True)
    if a.only != 'timing':
        rec['use'] = run('use', a)
        print(json.dumps(rec['use']), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
