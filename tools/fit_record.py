#!/usr/bin/env python3
"""Measures kb_fit / kb_score and writes profiles/fit_record.json.  No threshold is attached to any figure.
Kernel timing is on throughout (kb_set_kernel_timing): device times are HIP events through kb_fit_time_ms, wall times are
time.perf_counter around the call.

Three legs, each a child process of its own under `timeout`:
  streams  the reference's recordings G14 (7,000 samples to 790 landmarks) and G17 (12,400 samples to 3,000+) through ONE kb_fit
           call each, against the same recordings through kb_predict / kb_update one sample at a time -- the path the parent
           commit has, unchanged by kb_fit, so the same build serves.  The longest single launch with the default chunk is found
           by teaching a second handle the recording 256 samples per call: each such call is exactly one launch.
  fleet    --agents (4096) x 5 learners, each fitted with the augmented samples of the same --steps (20) logged steps of G10:
           all but the last 256 samples of every learner in one call, the last 256 in a second one (ONE launch with the default
           chunk, against the largest dictionaries: the longest launch).  Samples per second over both.
  score    on the handle the fleet leg's fit leaves: kb_score of every learner on the 201 grid candidates of one state, against
           1,000 kb_predict calls extrapolated to the same number, and select_action's own device time on that state.

  python tools/fit_record.py [--agents 4096] [--steps 20] [--only streams|fleet]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CHUNK = 256        # KB_FIT_CHUNK (csrc/kb_fit.hip)
SCORE_Q = 8        # KB_SCORE_Q


def _paths():
    for p in (ROOT, os.path.join(ROOT, 'network-slicing_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _kernel_resources():
    """registers / scratch of the two kernels from the build's remarks (csrc/build/resources.log), if it is there"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    res = cr.parse()
    out = {}
    for key in cr.FIT_SCRATCH:
        hit = [k for k in res if key in k and 'kb' in k]
        if hit:
            r = res[hit[0]]
            out[key] = dict(vgprs=r.get('VGPRs'), scratch_bytes_per_lane=r.get('ScratchSize'), occupancy=r.get('Occupancy'),
                            lds_bytes=r.get('LDS Size'))
    return out


def child_streams():
    import numpy as np
    _paths()
    from ranslice.kbrl_dev import VecKBRL

    def handle():
        ag = VecKBRL(1, [10], 200, capacity=4096, pool_bytes=1 << 30)
        ag.reset([[10]], [[3]])
        ag.set_kernel_timing(True)
        return ag
    warm = handle()   # first launches load code objects
    warm.fit([(0, 0)], [np.full((3, 11), 0.5)], [[1, -1, 1]])
    warm.predict(0, 0, np.full(11, 0.5))
    warm.close()
    out = {}
    for name in ('g14_projectron_long', 'g17_projectron_3000'):
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        if 'x' in g.files:
            xs = g['x']
        else:
            xs = np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1)
        ys = g['y']
        n = len(xs)
        a = handle()
        t0 = time.perf_counter()
        a.fit([(0, 0)], [xs], [ys])
        wall_fit = time.perf_counter() - t0
        w = a.fit_time_ms()
        b = handle()
        longest = 0.0
        for i in range(0, n, CHUNK):
            b.fit([(0, 0)], [xs[i:i + CHUNK]], [ys[i:i + CHUNK]])
            longest = max(longest, b.fit_time_ms()['fit_ms'])
        c = handle()
        t0 = time.perf_counter()
        for i in range(n):
            c.predict(0, 0, xs[i])
            c.update(0, 0, xs[i], int(ys[i]))
        wall_one = time.perf_counter() - t0
        la, lc = a.learner(0, 0, with_kinv=True), c.learner(0, 0, with_kinv=True)
        same = la['m'] == lc['m'] and all(la[k].tobytes() == lc[k].tobytes() for k in ('landmarks', 'coeff', 'kinv'))
        out[name] = dict(samples=n, landmarks=int(la['m']), mistakes=w['mistakes'], fit_wall_ms=1e3 * wall_fit, fit_device_ms=w['fit_ms'],
                         launches=(n + CHUNK - 1) // CHUNK, longest_launch_ms=longest, one_by_one_wall_ms=1e3 * wall_one,
                         one_by_one_round_trips=2 * n, wall_ratio=wall_one / wall_fit,
                         dictionary_bytes_equal_to_one_by_one=bool(same))
        for h in (a, b, c):
            h.close()
    print(json.dumps(out))


def _raw_fit(ag, task, first, rows, lab):
    i64p, i8p, ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ag._check(ag.L.kb_fit(ag.h, task.ctypes.data_as(ip), int(task.size), first.ctypes.data_as(i64p), rows.ctypes.data_as(dp),
                          lab.ctypes.data_as(i8p), 0, None, None, None, None, None))


def child_fleet(n_agents, steps):
    import numpy as np
    _paths()
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL, augmented_samples
    g = np.load(os.path.join(GOLDEN, 'g10_kbrl_s0.npz'))
    cfg = make_config(0)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    S = len(dims)
    X, Y = augmented_samples(g['state'][:steps], g['action_in'][:steps], g['labels'][:steps], dims, n_prbs)
    ag = VecKBRL(n_agents, dims, n_prbs, accuracy_range=tuple(g['a_range']), capacity=1024, pool_bytes=max(n_agents * S * (256 << 10), 64 << 20))
    ag.reset(np.tile(g['init_action'], (n_agents, 1)), np.tile(g['init_sec'], (n_agents, 1)))
    ag.set_kernel_timing(True)
    ag.fit([(0, 0)], [X[0][:0]], [Y[0][:0]])
    task = np.arange(n_agents * S, dtype=np.int32)
    out = dict(agents=n_agents, learners=n_agents * S, logged_steps=steps, samples_per_learner=[int(len(y)) for y in Y])
    total_ms, total_wall, total = 0.0, 0.0, 0
    for part, cut in (('head', lambda a: a[:max(len(a) - CHUNK, 0)]), ('tail', lambda a: a[max(len(a) - CHUNK, 0):])):
        xs = [np.pad(cut(x), ((0, 0), (0, 16 - x.shape[1]))) for x in X]
        ys = [cut(y) for y in Y]
        per_agent_x, per_agent_y = np.concatenate(xs), np.concatenate(ys)
        rows = np.tile(per_agent_x, (n_agents, 1))
        lab = np.tile(per_agent_y, n_agents).astype(np.int8)
        counts = np.tile(np.array([len(y) for y in ys], dtype=np.int64), n_agents)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        t0 = time.perf_counter()
        _raw_fit(ag, task, first, np.ascontiguousarray(rows), lab)
        wall = time.perf_counter() - t0
        w = ag.fit_time_ms()
        out[part] = dict(samples=int(first[-1]), staged_bytes=int(rows.nbytes + lab.nbytes), wall_ms=1e3 * wall, device_ms=w['fit_ms'],
                         launches=int((counts.max() + CHUNK - 1) // CHUNK), mistakes=w['mistakes'], insertions=w['insertions'])
        total_ms += w['fit_ms']
        total_wall += wall
        total += int(first[-1])
        del rows, lab
    sizes = ag.dictionary_sizes()
    out.update(samples=total, device_ms=total_ms, wall_ms=1e3 * total_wall, samples_per_second_device=total / (total_ms / 1e3),
               samples_per_second_wall=total / total_wall, longest_launch_ms=out['tail']['device_ms'],
               mean_dictionary=float(sizes.mean()), max_dictionary=int(sizes.max()), flags=ag.flagged_replicas())
    # ---- score: every learner on the 201 grid candidates of the next logged state
    state = g['state'][steps]
    cand = np.arange(n_prbs + 1) / n_prbs
    per_agent, off = [], 0
    for d in dims:
        q = np.zeros((n_prbs + 1, 16))
        q[:, :d] = state[off:off + d].astype(np.float64)
        q[:, d] = cand
        per_agent.append(q)
        off += d
    rows = np.ascontiguousarray(np.tile(np.concatenate(per_agent), (n_agents, 1)))
    first = (np.arange(n_agents * S + 1, dtype=np.int64) * (n_prbs + 1))
    f = np.zeros(len(rows))
    i64p, ip, dp = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    before = ag.fit_time_ms()['kernel_evals']
    t0 = time.perf_counter()
    ag._check(ag.L.kb_score(ag.h, task.ctypes.data_as(ip), int(task.size), first.ctypes.data_as(i64p), rows.ctypes.data_as(dp),
                            f.ctypes.data_as(dp), None))
    wall = time.perf_counter() - t0
    w = ag.fit_time_ms()
    # (kernel_evals: the last fit's plus the last score's; the last fit is the tail call in both readings)
    evals = int((sizes.astype(np.int64) * (n_prbs + 1)).sum())
    t0 = time.perf_counter()
    npred = 1000
    same = True
    for i in range(npred):
        t = (i * 7919) % (n_agents * S)
        c = (i * 31) % (n_prbs + 1)
        same = same and ag.predict(t // S, t % S, rows[t * (n_prbs + 1) + c, :dims[t % S] + 1])[1] == f[t * (n_prbs + 1) + c]
    wall_pred = time.perf_counter() - t0
    ag.phase_times_ms()
    st = np.tile(state, (n_agents, 1))
    ag.select_action(st)
    ag.select_action(st)
    ph = ag.phase_times_ms()
    out['score'] = dict(queries=int(len(rows)), queries_per_learner=n_prbs + 1, wall_ms=1e3 * wall, device_ms=w['score_ms'],
                        landmark_evaluations=evals, counted_by_the_kernel=int(w['kernel_evals'] - before) == evals,
                        landmark_evaluations_per_second_device=evals / (w['score_ms'] / 1e3) if w['score_ms'] else None,
                        kb_predict_calls_timed=npred, kb_predict_wall_ms_per_call=1e3 * wall_pred / npred,
                        kb_predict_extrapolated_wall_s=wall_pred / npred * len(rows), f_equal_to_kb_predict_in_the_timed_calls=bool(same),
                        select_action_device_ms=ph['select_ms'], Q=SCORE_Q, kernels=_kernel_resources())
    ag.close()
    print(json.dumps(out))


def run(leg, timeout, extra=()):
    cmd = ['timeout', '-k', '10', str(timeout), sys.executable, os.path.abspath(__file__), '--child', leg] + list(extra)
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--timeout', type=int, default=400)
    ap.add_argument('--only', choices=['streams', 'fleet'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_record.json'))
    a = ap.parse_args()
    if a.child == 'streams':
        return child_streams()
    if a.child == 'fleet':
        return child_fleet(a.agents, a.steps)
    rec = dict(statistic='one run per leg', default_chunk=CHUNK, Q=SCORE_Q)
    if a.only and os.path.exists(a.out):
        with open(a.out) as f:
            rec.update(json.load(f))
    if a.only != 'fleet':
        rec['streams'] = run('streams', a.timeout)
        print(json.dumps(rec['streams']), flush=True)
    if a.only != 'streams':
        rec['fleet'] = run('fleet', a.timeout, ['--agents', str(a.agents), '--steps', str(a.steps)])
        print(json.dumps(rec['fleet']), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
