#!/usr/bin/env python3
"""Measures kb_fork_rebuild and writes profiles/rebuild_record.json.  No threshold is attached to any figure.

Two legs, each a child process of its own under `timeout`:
  fleet   --agents (4096) agents of scenario 0 trained --train-steps (3,000) steps, the workload of tools/agent_file_record.py.
          The timed chain is import -> rebuild: wall ms of VecKBRL.load_agents(blob) and of fork_from(imported, index,
          rebuild=True) into a learning handle created beforehand, the replay's device ms (HIP events), the bytes its plan counts
          (mat-vec tiles read, rank-1 units read and written) and the TB/s they make of the replay's time, the rounds, and the
          smallest min_delta.  For orientation, in the same process: kb_fork of the same agents from the live source into a
          handle of the same size -- the only other way to a learning copy, which needs the source alive.  Eight dictionaries,
          the largest among them, are compared with the source's Kinv as bytes.
  long    --long-agents (8) agents trained --long-steps steps, to reach dictionaries above 2,000 landmarks: the same chain.

  python tools/rebuild_record.py [--agents 4096] [--train-steps 3000] [--long-agents 8] [--long-steps 40000] [--only fleet|long]

--only LEG measures that leg alone and keeps the other as the record at --base (default: --out) holds it.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(n, steps, with_fork):
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    from experiments_kbrl import BatchedEvaluator
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    ev = BatchedEvaluator(0, [0.99, 0.999], steps=steps, out_dir=tempfile.mkdtemp(prefix='rebuild_record_'))
    t0 = time.perf_counter()
    agent, _ = ev.train(range(n), graph=True)
    agent.synchronize()
    t_train = time.perf_counter() - t0
    index = np.arange(n, dtype=np.int32)
    sizes = agent.dictionary_sizes()
    pool = fork_pool_bytes(sizes)

    def learning_handle(k=n, pool_bytes=pool):
        return VecKBRL(k, agent.dims, agent.n_prbs, alfa=agent.cfg.alfa, accuracy_range=(agent.cfg.acc_lo, agent.cfg.acc_hi),
                       gamma=agent.cfg.gamma, eta=agent.cfg.eta, capacity=agent.capacity, pool_bytes=pool_bytes)
    # first launches load code objects: a two-agent pass through every call that is timed below
    warm = VecKBRL.load_agents(agent.export_agents(index[:2]), learning=True)
    warm.fork_from(agent, index[:2])
    warm.close()
    out = dict(train_wall_s=t_train, dictionaries=int(sizes.size), landmarks=int(sizes.sum()), mean_dictionary=float(sizes.mean()),
               max_dictionary=int(sizes.max()), learning_pool_bytes=int(pool))
    if with_fork:
        dst = learning_handle()
        dst.synchronize()
        t0 = time.perf_counter()
        dst.fork_from(agent, index)
        dst.synchronize()
        out['kb_fork_from_live_source_wall_ms'] = 1e3 * (time.perf_counter() - t0)
        dst.close()
    blob = agent.export_agents(index)
    out['file_bytes'] = len(blob)
    big = np.argsort(sizes.ravel())[::-1][:1].tolist() + np.random.default_rng(0).choice(sizes.size, 7, replace=False).tolist()
    want = {d: agent.learner(d // agent.S, d % agent.S, with_kinv=True) for d in big}
    ev.release()
    t0 = time.perf_counter()
    imported = VecKBRL.load_agents(blob)
    imported.synchronize()
    out['import_wall_ms'] = 1e3 * (time.perf_counter() - t0)
    dst = learning_handle()
    dst.set_kernel_timing(True)
    dst.synchronize()
    t0 = time.perf_counter()
    dst.fork_from(imported, index, rebuild=True)
    dst.synchronize()
    out['rebuild_wall_ms'] = 1e3 * (time.perf_counter() - t0)
    st = dst.rebuild_stats()
    same = True
    for d, w in want.items():
        got = dst.learner(d // agent.S, d % agent.S, with_kinv=True)
        same = same and got['m'] == w['m'] and got['kinv'].tobytes() == w['kinv'].tobytes() and got['coeff'].tobytes() == w['coeff'].tobytes()
    by = st['matvec_bytes'] + st['rank1_bytes']
    out.update(replay_ms=st['replay_ms'], matvec_bytes=st['matvec_bytes'], rank1_bytes=st['rank1_bytes'], plan_bytes=by,
               replay_TBps=by / st['replay_ms'] / 1e9 if st['replay_ms'] else None, rounds=st['rounds'],
               dictionaries_rebuilt=st['dictionaries'], smallest_min_delta=float(st['min_delta'].min()),
               kinv_bytes_equal_to_source_in_sampled_dictionaries=bool(same), sampled_dictionary_sizes=[int(want[d]['m']) for d in big])
    dst.close()
    imported.close()
    print(json.dumps(out))


def run(leg, n, steps, timeout):
    cmd = ['timeout', '-k', '10', str(timeout), sys.executable, os.path.abspath(__file__), '--child', leg, '--agents', str(n),
           '--train-steps', str(steps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--train-steps', type=int, default=3000)
    ap.add_argument('--long-agents', type=int, default=8)
    ap.add_argument('--long-steps', type=int, default=40000)
    ap.add_argument('--timeout', type=int, default=600)
    ap.add_argument('--only', choices=['fleet', 'long'])
    ap.add_argument('--base', default=None, help='with --only: the record whose other leg is kept (default: --out)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rebuild_record.json'))
    a = ap.parse_args()
    if a.child:
        return child(a.agents, a.train_steps, a.child == 'fleet')
    rec = dict(scenario=0, statistic='one run per leg', small_threshold=192)
    if a.only:
        with open(a.base or a.out) as f:
            rec.update(json.load(f))
    if a.only != 'long':
        rec['fleet'] = dict(agents=a.agents, train_steps=a.train_steps, **run('fleet', a.agents, a.train_steps, a.timeout))
        print(json.dumps(rec['fleet']), flush=True)
    if a.only != 'fleet':
        rec['long'] = dict(agents=a.long_agents, train_steps=a.long_steps, **run('long', a.long_agents, a.long_steps, a.timeout))
        print(json.dumps(rec['long']), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
