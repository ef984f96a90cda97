#!/usr/bin/env python3
"""Measures the shared-dictionary rounds under the margin rule (kb_set_shared_plus, SharedVecKBRL.set_shared_plus)
and writes profiles/shared_plus_record.json.  No threshold is attached to the mode's own cost.

The shape is the config-4 shape of §8p's record (scenario index 2, --replicas (4096) replicas, capacity 1024, budget 256, its own
world), closed loop through step_resident, every run a child process of its own under `timeout`, all from the same seeds: the
runs of the two modes start from the same state.  For max_rounds 1 and 4, switch off and switch on alternate, --rounds (3) times
each; per run the wall ms per step of the filling window (steps 30-230) and of the saturated window (steps 330-530) -- every step
ends with a fetch of its violations, in every run alike -- and the median over the rounds is recorded beside the single values.
One more run per mode and max_rounds, untimed, counts per step and window: the exchange rounds used, and from the counters the
samples of branches 1-3 (kb_get_stats[1]), of branch 2 (kb_get_stats[2]) and of branch 4 (kb_get_repair_work's work[6] less
kb_get_stats[1]; with the switch off work[6] stays 0), with the SLA violations per step and replica.  Branch 0 (a proposal that
an earlier one of its list already taught) and the split of branches 1 and 3 are not counted by the library.

The two modes are not forks of one handle: kb_fork does not take a shared-dictionary handle.  Every run resets the simulator
and the agent from the same seeds, which is the same start, bit for bit.

--parent-checkout DIR: a built checkout of the parent commit with this file copied into its tools/.  Its switch-off run (a child
of THAT copy, against THAT library; a switch-off child never touches the switch, so the tool runs there) takes its turn in every
round, before this build's two: parent, off, on, parent, off, on, ...  Its figures go into the record as `parent_shared_kbrl`,
beside the switch-off ranges of this build.  --parent-on: the parent's switch-on run takes a turn as well (the parent must have
kb_set_shared_plus), recorded as `parent_shared_kbrl_switch_on`.

Mode `batch`: the switch on and kb_set_shared_plus_batch(--shared-plus-batch M (2), --segments (4)) beside it; its
counting run also records kb_shared_plus_batch_info's work[0..4] per step.  --extra-min 64,256: one more timed `batch` run per cell
at each of these min_landmarks, recorded as `batch_min_<M>`; --extra-segments 8,16 the same for the segment rounds
(`batch_segments_<N>`).  --cells 1,4: the max_rounds measured.  The §8r record is
profiles/shared_plus_batch_record.json (--out), measured with --modes off,on,batch --parent-checkout DIR.

  python tools/shared_plus_record.py [--replicas 4096] [--rounds 3] [--modes off,on] [--parent-checkout DIR]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIO, BUDGET, CAPACITY, FADING_COLS = 2, 256, 1024, 4096
WINDOWS = {'filling': (30, 230), 'saturated': (330, 530)}
STEPS = 530


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
    agent = SharedVecKBRL(n, dims, cfg.n_prbs, budget=BUDGET, max_rounds=a.max_rounds, capacity=CAPACITY)
    if a.mode in ('on', 'batch'):       # (the switch-off runs never touch the switch: the tool measures the parent commit as well)
        agent.set_shared_plus(True)
    if a.mode == 'batch':
        agent.set_shared_plus_batch(a.shared_plus_batch, a.segments)
    agent.reset(ia, sf, seeds=replica_seeds(7, 0, n))
    env._check(env.L.rs_step(env.h, np.ascontiguousarray(ia).ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    out = dict(mode=a.mode, max_rounds=a.max_rounds, replicas=n, counting=bool(a.count))
    edges = sorted({e for w in WINDOWS.values() for e in w})
    marks, step = {}, 0
    viol = rounds = 0.0

    def counters():
        st, wk = agent.stats(), agent._repair_raw()
        c = dict(changed=st[1], inserted=st[2], work6=int(wk[6]))
        if a.mode == 'batch':
            c['spb'] = agent.shared_plus_batch_work()[:5]
        return c
    for edge in edges + [STEPS]:
        while step < edge:
            agent.step_resident(env, count_rounds=bool(a.count))
            env.step_resident()
            viol += float(env.fetch()['violations'].sum())
            rounds += agent.rounds_last if a.count else 0
            step += 1
        env.synchronize()
        agent.synchronize()
        marks[edge] = dict(t=time.perf_counter(), viol=viol, rounds=rounds, sizes=agent.dictionary_sizes().astype(int).tolist(), **counters())
    for name, (lo, hi) in WINDOWS.items():
        m0, m1, k = marks[lo], marks[hi], float(hi - lo)
        w = dict(steps=[lo, hi], ms_per_step=1e3 * (m1['t'] - m0['t']) / k, dictionary_sizes_at_end=m1['sizes'],
                 violations_per_step_and_replica=(m1['viol'] - m0['viol']) / k / n)
        if a.count:
            ch, ins, w6 = (m1[q] - m0[q] for q in ('changed', 'inserted', 'work6'))
            w.update(per_step=dict(rounds_used=(m1['rounds'] - m0['rounds']) / k, branches_1_to_3=ch / k, branch_2=ins / k,
                                   branches_1_and_3=(ch - ins) / k, branch_4=(max(w6 - ch, 0) / k) if a.mode in ('on', 'batch') else 0.0))
            if a.mode == 'batch':
                w['per_step']['shared_plus_batch_work_0_to_4'] = [(q1 - q0) / k for q0, q1 in zip(m0['spb'], m1['spb'])]
            del w['ms_per_step']      # (a counting run waits for every step's round count: not a timing)
        out[name] = w
    agent.close()
    env.close()
    print(json.dumps(out))


def run(mode, max_rounds, count, a, tool=None, min_landmarks=None, segments=None):
    cmd = ['timeout', '-k', '10', str(a.timeout), sys.executable, tool or os.path.abspath(__file__), '--child', mode, '--replicas', str(a.replicas),
           '--max-rounds', str(max_rounds), '--shared-plus-batch', str(min_landmarks or a.shared_plus_batch), '--segments', str(segments if segments is not None else a.segments)
           ] + (['--count'] if count else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', dest='mode')
    ap.add_argument('--max-rounds', type=int, default=1)
    ap.add_argument('--count', action='store_true')
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--modes', default='off,on', help='of off, on, batch')
    ap.add_argument('--shared-plus-batch', type=int, default=2, help='mode batch: min_landmarks of kb_set_shared_plus_batch')
    ap.add_argument('--segments', type=int, default=4, help='mode batch: the segment rounds enqueued per apply')
    ap.add_argument('--extra-min', default='', help='mode batch: one more timed run per cell at each of these min_landmarks')
    ap.add_argument('--extra-segments', default='', help='mode batch: one more timed run per cell at each of these segment rounds')
    ap.add_argument('--cells', default='1,4', help='the max_rounds measured')
    ap.add_argument('--no-counts', action='store_true', help='skip the untimed counting runs')
    ap.add_argument('--parent-checkout', help='a built checkout of the parent commit with this tool copied into its tools/')
    ap.add_argument('--parent-on', action='store_true', help="with --parent-checkout: the parent's switch-on run takes a turn in every round as well")
    ap.add_argument('--timeout', type=int, default=300)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'shared_plus_record.json'))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
    if a.mode:
        return child(a)
    modes = a.modes.split(',')
    rec = dict(scenario=SCENARIO, replicas=a.replicas, budget=BUDGET, capacity=CAPACITY, windows=WINDOWS, rounds=a.rounds,
               statistic='median of %d alternating runs per mode, one MI355X; every run a process of its own from the same seeds' % a.rounds)
    parent, parent_on = {}, {}
    for mr in [int(v) for v in a.cells.split(',')]:
        runs = {m: [] for m in modes}
        par, par_on = [], []
        for _ in range(a.rounds):      # (one after the other: never two processes on the GPU at once)
            if a.parent_checkout:
                par.append(run('off', mr, False, a, tool=os.path.join(os.path.abspath(a.parent_checkout), 'tools', os.path.basename(__file__))))
                if a.parent_on:
                    par_on.append(run('on', mr, False, a, tool=os.path.join(os.path.abspath(a.parent_checkout), 'tools', os.path.basename(__file__))))
            for m in modes:
                runs[m].append(run(m, mr, False, a))
        if par:
            parent['max_rounds_%d' % mr] = {w: dict(ms_per_step_runs=[r[w]['ms_per_step'] for r in par],
                                                     ms_per_step_range=[min(r[w]['ms_per_step'] for r in par), max(r[w]['ms_per_step'] for r in par)])
                                            for w in WINDOWS}
        if par_on:
            parent_on['max_rounds_%d' % mr] = {w: dict(ms_per_step_runs=[r[w]['ms_per_step'] for r in par_on],
                                                        ms_per_step_range=[min(r[w]['ms_per_step'] for r in par_on), max(r[w]['ms_per_step'] for r in par_on)])
                                               for w in WINDOWS}
        entry = {}
        for m in modes:
            e = {}
            for wname in WINDOWS:
                ms = [r[wname]['ms_per_step'] for r in runs[m]]
                e[wname] = dict(ms_per_step_median=statistics.median(ms), ms_per_step_runs=ms, ms_per_step_range=[min(ms), max(ms)],
                                violations_per_step_and_replica=runs[m][0][wname]['violations_per_step_and_replica'],
                                dictionary_sizes_at_end=runs[m][0][wname]['dictionary_sizes_at_end'])
            if not a.no_counts:
                c = run(m, mr, True, a)
                for wname in WINDOWS:
                    e[wname]['per_step'] = c[wname]['per_step']
            entry['switch_' + m] = e
            print(json.dumps({'max_rounds': mr, 'switch': m, **{w: e[w]['ms_per_step_median'] for w in WINDOWS}}), flush=True)
        if 'batch' in modes:
            entry['switch_batch']['min_landmarks'], entry['switch_batch']['segments'] = a.shared_plus_batch, a.segments
            for lo in [int(v) for v in a.extra_min.split(',') if v]:
                r = run('batch', mr, False, a, min_landmarks=lo)
                entry['batch_min_%d' % lo] = {w: dict(ms_per_step_one_run=r[w]['ms_per_step']) for w in WINDOWS}
                print(json.dumps({'max_rounds': mr, 'batch_min': lo, **{w: r[w]['ms_per_step'] for w in WINDOWS}}), flush=True)
            for sg in [int(v) for v in a.extra_segments.split(',') if v]:
                r = run('batch', mr, False, a, segments=sg)
                entry['batch_segments_%d' % sg] = {w: dict(ms_per_step_one_run=r[w]['ms_per_step']) for w in WINDOWS}
                print(json.dumps({'max_rounds': mr, 'batch_segments': sg, **{w: r[w]['ms_per_step'] for w in WINDOWS}}), flush=True)
        rec['max_rounds_%d' % mr] = entry
    if parent:
        rec['parent_shared_kbrl'] = parent
        rec['parent_statistic'] = ('the parent commit, switch-off children of this tool in a checkout of it, one in every round before this '
                                   "build's two, %d runs each" % a.rounds)
    if parent_on:
        rec['parent_shared_kbrl_switch_on'] = parent_on
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
