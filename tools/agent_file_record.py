#!/usr/bin/env python3
"""Measures the agent files (kb_export_agents / kb_import_agents) and writes profiles/agent_file_record.json.

Workload: --agents (4096) agents of scenario 0 trained --train-steps (3,000) steps, the bench's config-3 point.  Each repeat
is a child process of its own under `timeout` (it trains, then measures); the record holds the median of the repeats.
  * wall time of kb_export_bytes + kb_export_agents of all agents, of kb_import_agents of the result, and of kb_deploy_ref
    from the import onto --replicas (65,536) replicas;
  * effective GB/s of agents_pack_kernel and agents_build_kernel: HIP events around the one launch over the bytes the
    kernel's own work plan counts (kb_agents_kernel_times);
  * the file's size beside kb_state_bytes of the source and beside deploy_pool_bytes;
  * the baseline: the only route the parent commit offers, a loop of kb_get_learner over the same (agent, slice) pairs, run
    from a built checkout of that commit (--tree DIR), not from the code under test.

  python tools/agent_file_record.py [--tree ../parent] [--agents 4096] [--train-steps 3000] [--replicas 65536]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def train(tree, n, steps):
    sys.path.insert(0, os.path.join(tree, 'network-slicing_amd'))
    from experiments_kbrl import BatchedEvaluator
    ev = BatchedEvaluator(0, [0.99, 0.999], steps=steps, out_dir=tempfile.mkdtemp(prefix='agent_file_record_'))
    t0 = time.perf_counter()
    agent, _ = ev.train(range(n), graph=True)
    agent.synchronize()
    return ev, agent, time.perf_counter() - t0


def child_file(tree, n, steps, replicas):
    import numpy as np
    ev, agent, t_train = train(tree, n, steps)
    from ranslice.kbrl_dev import VecKBRL, deploy_pool_bytes
    index = np.arange(n, dtype=np.int32)
    sizes = agent.dictionary_sizes()
    nb = C.c_uint64()
    agent._check(agent.L.kb_state_bytes(agent.h, C.byref(nb)))
    VecKBRL.load_agents(agent.export_agents(index[:2])).deploy([0, 1, 0], by_reference=True).close()   # first launches load code objects
    t0 = time.perf_counter()
    blob = agent.export_agents(index)
    t_export = time.perf_counter() - t0
    ms, by = (C.c_double * 2)(), (C.c_uint64 * 2)()
    agent.L.kb_agents_kernel_times(ms, by)
    pack_ms, pack_bytes = ms[0], by[0]
    ev.release()
    t0 = time.perf_counter()
    imported = VecKBRL.load_agents(blob)
    imported.synchronize()
    t_import = time.perf_counter() - t0
    imported.L.kb_agents_kernel_times(ms, by)
    build_ms, build_bytes = ms[1], by[1]
    t0 = time.perf_counter()
    fleet = imported.deploy((np.arange(replicas) % n).astype(np.int32), by_reference=True)
    fleet.synchronize()
    t_fan = time.perf_counter() - t0
    pool = fleet.pool()['used_bytes']
    fleet.close()
    imported.close()
    print(json.dumps(dict(train_wall_s=t_train, landmarks=int(sizes.sum()), mean_dictionary=float(sizes.mean()),
                          max_dictionary=int(sizes.max()), file_bytes=len(blob), state_bytes=int(nb.value),
                          deploy_pool_bytes=int(deploy_pool_bytes(sizes)), export_wall_ms=1e3 * t_export, import_wall_ms=1e3 * t_import,
                          deploy_ref_wall_ms=1e3 * t_fan, deploy_ref_pool_bytes=int(pool), pack_kernel_ms=pack_ms,
                          pack_kernel_bytes=int(pack_bytes), pack_kernel_GBps=pack_bytes / pack_ms / 1e6 if pack_ms else None,
                          build_kernel_ms=build_ms, build_kernel_bytes=int(build_bytes),
                          build_kernel_GBps=build_bytes / build_ms / 1e6 if build_ms else None)))


def child_get_learner(tree, n, steps):
    ev, agent, t_train = train(tree, n, steps)
    t0 = time.perf_counter()
    total = 0
    for e in range(n):
        for s in range(agent.S):
            total += agent.learner(e, s)['m']
    dt = time.perf_counter() - t0
    ev.release()
    print(json.dumps(dict(train_wall_s=t_train, landmarks=int(total), get_learner_loop_wall_ms=1e3 * dt, calls=n * agent.S)))


def run(leg, a, tree):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, os.path.abspath(__file__), '--child', leg, '--agents', str(a.agents),
           '--train-steps', str(a.train_steps), '--replicas', str(a.replicas), '--tree', tree]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def median_of(rows):
    out = {}
    for key in rows[0]:
        vals = [r[key] for r in rows]
        out[key] = statistics.median(vals) if all(isinstance(v, (int, float)) for v in vals) else vals[0]
        if isinstance(vals[0], float):
            out[key + '_runs'] = vals
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--train-steps', type=int, default=3000)
    ap.add_argument('--replicas', type=int, default=65536)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--tree', default=None, help='a built checkout of the parent commit: the kb_get_learner baseline runs from it')
    ap.add_argument('--timeout', type=int, default=300)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'agent_file_record.json'))
    a = ap.parse_args()
    if a.child == 'file':
        return child_file(a.tree or ROOT, a.agents, a.train_steps, a.replicas)
    if a.child == 'get_learner':
        return child_get_learner(a.tree or ROOT, a.agents, a.train_steps)
    rec = dict(scenario=0, agents=a.agents, train_steps=a.train_steps, replicas=a.replicas, repeats=a.repeats, statistic='median')
    rec['agent_file'] = median_of([run('file', a, ROOT) for _ in range(a.repeats)])
    print(json.dumps(rec['agent_file']), flush=True)
    if a.tree:
        rec['baseline_parent_tree'] = median_of([run('get_learner', a, os.path.abspath(a.tree)) for _ in range(a.repeats)])
        print(json.dumps(rec['baseline_parent_tree']), flush=True)
    else:
        rec['baseline_parent_tree'] = 'not measured: no --tree given'
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
