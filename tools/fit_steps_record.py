#!/usr/bin/env python3
"""Measures kb_fit_steps and writes profiles/fit_steps_record.json.  No threshold is attached to any figure.
Kernel timing is on throughout (kb_set_kernel_timing): device times are HIP events through kb_fit_time_ms, wall times are
time.perf_counter around what is named.  One run per figure; each leg is a child process of its own under `timeout`.

  a  --agents (4096) agents x the first --steps (20) steps of G10 s0, two ways on two handles created and reset alike:
     augmented_samples + fit (the parent commit's path, unchanged by this one: expansion of one agent's log, replication to the
     fleet, the call with its staging) and fit_steps on the log itself; whether the two handles hold equal dictionaries.
  b  the same fleet on all 120 steps of G10 s0 through fit_steps alone.
  c  64 agents x G15's 2,200 steps through fit_steps alone (dictionaries of up to 496 landmarks: both paths of the column).
  d  leg a in 'projectron_plus' mode.
  e  kb_set_fit_steps_batch, written to profiles/fit_steps_batch_record.json: fleets of --agents agents in
     'projectron_plus' mode are taught one log at widths 0, 2, 4 and 8 in the same build -- widths 0 and 8 alternate over --rounds
     (3) rounds (median and range), widths 2 and 4 run once -- and the dictionaries every width leaves are compared as bytes.
     Two logs: `early`, leg d's log on fresh fleets (small dictionaries); `step_N`, --window (10) steps logged by this tool from a
     Projectron++ closed loop (control_plus on, batch 8) of the same size around step --at (500), taught to forks of the fleet as
     it stood in front of the window.  Per width: device ms, wall ms, kb_fit_steps_batch_info's eight counters, landmarks mean / max.

  python tools/fit_steps_record.py [--agents 4096] [--steps 20] [--only a|b|c|d|e] [--at 500] [--window 10] [--rounds 3]
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


def _paths():
    for p in (ROOT, os.path.join(ROOT, 'network-slicing_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _kernel_resources():
    """registers / scratch / LDS of the two kernels from the build's remarks (csrc/build/resources.log), if it is there"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    res = cr.parse()
    out = {}
    for key in ('fit_steps_kernel', 'fit_steps_plus_kernel', 'fit_kernel', 'fit_plus_kernel'):
        hit = [k for k in res if ('%d%s' % (len(key), key)) in k]
        if hit:
            r = res[hit[0]]
            out[key] = dict(vgprs=r.get('VGPRs'), scratch_bytes_per_lane=r.get('ScratchSize'), occupancy=r.get('Occupancy'),
                            lds_bytes=r.get('LDS Size'))
    return out


def _log(name, steps=None):
    import numpy as np
    from ranslice.config import make_config
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    cfg = make_config(int(g['scenario']))
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    cut = slice(0, steps)
    return (g, dims, n_prbs, np.ascontiguousarray(g['state'][cut], dtype=np.float32),
            np.ascontiguousarray(g['action_in'][cut], dtype=np.int32), np.ascontiguousarray(g['labels'][cut], dtype=np.int32))


def _handle(n_agents, g, dims, n_prbs, pool_bytes, algorithm='projectron'):
    import numpy as np
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(n_agents, dims, n_prbs, accuracy_range=tuple(g['a_range']), capacity=1024, pool_bytes=pool_bytes, algorithm=algorithm)
    ag.reset(np.tile(g['init_action'], (n_agents, 1)), np.tile(g['init_sec'], (n_agents, 1)))
    ag.set_kernel_timing(True)
    return ag


def _raw_steps(ag, n_agents, state, action, labels):
    """kb_fit_steps with every agent given the same log (replicated on the host: part of what a caller stages); -> wall s, bytes"""
    import numpy as np
    T = len(state)
    t0 = time.perf_counter()
    st, ac, lb = (np.ascontiguousarray(np.tile(v, (n_agents, 1))) for v in (state, action, labels))
    agent = np.arange(n_agents, dtype=np.int32)
    first = np.arange(n_agents + 1, dtype=np.int64) * T
    rep = time.perf_counter() - t0
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    t0 = time.perf_counter()
    ag._check(ag.L.kb_fit_steps(ag.h, agent.ctypes.data_as(ip), n_agents, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                st.ctypes.data_as(fp), ac.ctypes.data_as(ip), lb.ctypes.data_as(ip), 0, None, None, None, None, None))
    return rep, time.perf_counter() - t0, int(st.nbytes + ac.nbytes + lb.nbytes + agent.nbytes + first.nbytes)


def _steps_leg(ag, n_agents, state, action, labels):
    rep, wall, staged = _raw_steps(ag, n_agents, state, action, labels)
    w = ag.fit_time_ms()
    sizes = ag.dictionary_sizes()
    return dict(logged_steps=len(state), samples=w['samples'], mistakes=w['mistakes'], insertions=w['insertions'],
                kernel_evals=w['kernel_evals'], device_ms=w['fit_ms'], call_wall_ms=1e3 * wall, replicate_log_wall_ms=1e3 * rep,
                staged_bytes=staged, samples_per_second_device=w['samples'] / (w['fit_ms'] / 1e3) if w['fit_ms'] else None,
                mean_dictionary=float(sizes.mean()), max_dictionary=int(sizes.max()), flags=ag.flagged_replicas())


def child_fleet(n_agents, steps, algorithm):
    import numpy as np
    _paths()
    from ranslice.kbrl_dev import augmented_samples
    g, dims, n_prbs, state, action, labels = _log('g10_kbrl_s0', steps)
    S = len(dims)
    pool = max(n_agents * S * (256 << 10), 64 << 20)
    a, b = (_handle(n_agents, g, dims, n_prbs, pool, algorithm) for _ in range(2))
    for h in (a, b):   # first launches load code objects
        h.fit([(0, 0)], [np.zeros((0, dims[0] + 1))], [np.zeros(0, dtype=np.int8)])
    warm = _handle(1, g, dims, n_prbs, 64 << 20, algorithm)
    warm.fit_steps([0], [state[:1]], [action[:1]], [labels[:1]])
    warm.fit([(0, 0)], [np.full((2, 11), 0.5)], [[1, -1]])
    warm.close()
    # ---- the parent's path: expand one agent's log, replicate it to the fleet, one kb_fit
    t0 = time.perf_counter()
    X, Y = augmented_samples(state, action, labels, dims, n_prbs)
    expand = time.perf_counter() - t0
    t0 = time.perf_counter()
    per_x = np.concatenate([np.pad(x, ((0, 0), (0, 16 - x.shape[1]))) for x in X])
    rows = np.ascontiguousarray(np.tile(per_x, (n_agents, 1)))
    lab = np.tile(np.concatenate(Y), n_agents).astype(np.int8)
    first = np.concatenate([[0], np.cumsum(np.tile(np.array([len(y) for y in Y], dtype=np.int64), n_agents))]).astype(np.int64)
    task = np.arange(n_agents * S, dtype=np.int32)
    rep = time.perf_counter() - t0
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    t0 = time.perf_counter()
    a._check(a.L.kb_fit(a.h, task.ctypes.data_as(ip), int(task.size), first.ctypes.data_as(C.POINTER(C.c_int64)), rows.ctypes.data_as(dp),
                        lab.ctypes.data_as(C.POINTER(C.c_int8)), 0, None, None, None, None, None))
    wall = time.perf_counter() - t0
    w = a.fit_time_ms()
    out = dict(agents=n_agents, learners=n_agents * S, algorithm=algorithm, samples_per_learner=[int(len(y)) for y in Y])
    out['augmented_samples_then_fit'] = dict(
        samples=w['samples'], mistakes=w['mistakes'], insertions=w['insertions'], kernel_evals=w['kernel_evals'], device_ms=w['fit_ms'],
        call_wall_ms=1e3 * wall, expand_one_log_wall_ms=1e3 * expand, replicate_samples_wall_ms=1e3 * rep,
        wall_ms_with_expansion_and_staging=1e3 * (wall + expand + rep), staged_bytes=int(rows.nbytes + lab.nbytes + first.nbytes + task.nbytes),
        samples_per_second_device=w['samples'] / (w['fit_ms'] / 1e3) if w['fit_ms'] else None)
    del rows, lab
    # ---- fit_steps on the log itself
    out['fit_steps'] = _steps_leg(b, n_agents, state, action, labels)
    fs = out['fit_steps']
    fs['wall_ms_with_replication_and_staging'] = fs['call_wall_ms'] + fs['replicate_log_wall_ms']
    # ---- the two handles: sizes and statistics of every learner, the bytes of every learner of 128 agents spread over the fleet
    same = bool(np.array_equal(a.dictionary_sizes(), b.dictionary_sizes())) and a.stats() == b.stats() and \
        a.flagged_replicas() == b.flagged_replicas()
    picked = sorted(set(np.linspace(0, n_agents - 1, min(n_agents, 128)).astype(int).tolist()))
    for e in picked:
        for s in range(S):
            la, lb_ = a.learner(e, s, with_kinv=True), b.learner(e, s, with_kinv=True)
            same = same and la['m'] == lb_['m'] and all(la[k].tobytes() == lb_[k].tobytes() for k in ('landmarks', 'coeff', 'kinv'))
    out['dictionaries_equal_bytes'] = bool(same)
    out['dictionaries_compared'] = 'sizes, statistics and flags of all learners; landmarks, coefficients and Kinv of %d agents' % len(picked)
    out['device_ms_ratio_fit_over_fit_steps'] = out['augmented_samples_then_fit']['device_ms'] / fs['device_ms'] if fs['device_ms'] else None
    out['kernels'] = _kernel_resources()
    a.close()
    b.close()
    print(json.dumps(out))


def child_steps_only(name, n_agents, pool_per_learner):
    import numpy as np
    _paths()
    g, dims, n_prbs, state, action, labels = _log(name)
    warm = _handle(1, g, dims, n_prbs, 64 << 20)
    warm.fit_steps([0], [state[:1]], [action[:1]], [labels[:1]])
    warm.close()
    ag = _handle(n_agents, g, dims, n_prbs, max(n_agents * len(dims) * pool_per_learner, 64 << 20))
    out = dict(agents=n_agents, learners=n_agents * len(dims), recording=name)
    out.update(_steps_leg(ag, n_agents, state, action, labels))
    lm = [len(np.atleast_2d(g['landmarks%d' % s])) for s in range(len(dims))]
    out['sizes_of_agent_0'] = ag.dictionary_sizes()[0].tolist()
    out['sizes_equal_the_recording'] = out['sizes_of_agent_0'] == lm
    out['augmented_rows_would_stage_bytes'] = int(out['samples']) * 129
    ag.close()
    print(json.dumps(out))


def _batch_resources():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    return {k: dict(vgprs=r.get('VGPRs'), agprs=r.get('AGPRs'), sgprs_spilled=r.get('SGPRs Spill'), scratch_bytes_per_lane=r.get('ScratchSize'),
                    occupancy=r.get('Occupancy'), lds_bytes=r.get('LDS Size'))
            for k, r in cr.parse().items() if 'fit_steps_batch_kernel' in k or 'fit_steps_plus_kernel' in k}


def _digest(ag, picked):
    """sizes, statistics and flags of all learners; landmarks, coefficients and Kinv of the picked agents"""
    import hashlib
    h = hashlib.sha256()
    h.update(ag.dictionary_sizes().tobytes())
    h.update(repr((ag.stats(), ag.flagged_replicas())).encode())
    for e in picked:
        for s in range(ag.S):
            lr = ag.learner(e, s, with_kinv=True)
            for k in ('landmarks', 'coeff', 'kinv'):
                h.update(lr[k].tobytes())
    return h.hexdigest()


def _widths_on_a_log(prepare, n_agents, log, rounds, max_landmarks):
    """prepare() -> a pupil fleet in the state the log is taught to; the log [T, ...] of one agent (replicated) or [n, T, ...]"""
    import statistics
    import numpy as np
    st, ac, lb = log
    if st.ndim == 2:
        st, ac, lb = (np.ascontiguousarray(np.tile(v, (n_agents, 1))) for v in (st, ac, lb))
    else:
        st, ac, lb = (np.ascontiguousarray(v.reshape((-1,) + v.shape[2:])) for v in (st, ac, lb))
    T = len(st) // n_agents
    agent, first = np.arange(n_agents, dtype=np.int32), np.arange(n_agents + 1, dtype=np.int64) * T
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    picked = sorted(set(np.linspace(0, n_agents - 1, min(n_agents, 128)).astype(int).tolist()))
    runs, digests, before = {}, set(), None
    for w in [w for _ in range(rounds) for w in (0, 8)] + [2, 4]:
        ag = prepare()
        if before is None:
            sizes = ag.dictionary_sizes()
            before = dict(landmarks_mean=float(sizes.mean()), landmarks_max=int(sizes.max()))
        ag.set_fit_steps_batch(w, max_landmarks)
        ag.set_kernel_timing(True)
        t0 = time.perf_counter()
        ag._check(ag.L.kb_fit_steps(ag.h, agent.ctypes.data_as(ip), n_agents, first.ctypes.data_as(C.POINTER(C.c_int64)),
                                    st.ctypes.data_as(fp), ac.ctypes.data_as(ip), lb.ctypes.data_as(ip), 0, None, None, None, None, None))
        wall = 1e3 * (time.perf_counter() - t0)
        ft = ag.fit_time_ms()
        sizes = ag.dictionary_sizes()
        r = runs.setdefault(str(w), dict(device_ms=[], call_wall_ms=[]))
        r['device_ms'].append(ft['fit_ms'])
        r['call_wall_ms'].append(wall)
        r.update(work=ag.fit_steps_batch_work(), samples=ft['samples'], mistakes=ft['mistakes'], insertions=ft['insertions'],
                 kernel_evals=ft['kernel_evals'], landmarks_mean_after=float(sizes.mean()), landmarks_max_after=int(sizes.max()))
        digests.add(_digest(ag, picked))
        print('width %d: %.1f ms on the device, %.1f ms wall, work %s' % (w, ft['fit_ms'], wall, r['work']), file=sys.stderr, flush=True)
    for r in runs.values():
        for k in ('device_ms', 'call_wall_ms'):
            v = r[k]
            r[k] = dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)
    if len(digests) != 1:
        raise SystemExit('the widths left different dictionaries')
    m0 = runs['0']['device_ms']['median']
    return dict(logged_steps=T, before=before, widths=runs, dictionaries_equal_bytes=True,
                dictionaries_compared='sizes, statistics and flags of all learners; landmarks, coefficients and Kinv of %d agents' % len(picked),
                device_ms_ratio_width_0_over={w: m0 / runs[w]['device_ms']['median'] for w in ('2', '4', '8')})


def child_batch(n_agents, steps, at, window, rounds, max_landmarks, capacity, pool_gb, only):
    import numpy as np
    _paths()
    from ranslice.config import make_config
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice, default_fading
    out = dict(agents=n_agents, rounds=rounds, max_landmarks=max_landmarks, kernels=_batch_resources())
    pool = int(pool_gb * (1 << 30))
    if only in (None, 'early'):
        g, dims, n_prbs, state, action, labels = _log('g10_kbrl_s0', steps)
        out['learners'] = n_agents * len(dims)
        ag = VecKBRL(n_agents, dims, n_prbs, accuracy_range=tuple(g['a_range']), capacity=1024, algorithm='projectron_plus',
                     pool_bytes=max(n_agents * len(dims) * (256 << 10), 64 << 20))

        def fresh():
            ag.reset(np.tile(g['init_action'], (n_agents, 1)), np.tile(g['init_sec'], (n_agents, 1)))
            return ag
        fresh().fit_steps([0], [state[:1]], [action[:1]], [labels[:1]])     # (first launches load code objects)
        out['early'] = _widths_on_a_log(fresh, n_agents, (state, action, labels), rounds, max_landmarks)
        ag.close()
    if only in (None, 'late'):
        cfg = make_config(0, n_envs=n_agents)
        dims, n_prbs, mode = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs, 'projectron_plus'
        out['learners'] = n_agents * len(dims)
        env = VecRanSlice(n_envs=n_agents, cfg=cfg, fading=default_fading(), seed=0)
        teacher, base, pupil = (VecKBRL(n_agents, dims, n_prbs, capacity=capacity, pool_bytes=pool, algorithm=mode, control_plus=True)
                                for _ in range(3))
        teacher.set_control_plus_batch(8, max_landmarks)
        ia = np.full((n_agents, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32)
        env.reset()
        teacher.reset(ia, np.full((n_agents, len(dims)), 3, dtype=np.int32))
        env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
        first, step, t0 = max(1, at - window // 2), 0, time.perf_counter()
        while step < first - 1:      # (in stretches, with a sign of life between them)
            k = min(250, first - 1 - step)
            teacher.run_resident(env, k, graph=False)
            teacher.synchronize()
            step += k
            print('step %d, %.1f s' % (step, time.perf_counter() - t0), file=sys.stderr, flush=True)
        f = env.fetch()              # one step by hand: the state the window's first action is chosen in
        teacher.step_resident(env)
        state = f['obs']
        env.step_resident()
        everyone = np.arange(n_agents, dtype=np.int32)
        base.fork_from(teacher, everyone)      # the fleet in front of the window
        log = [], [], []
        for _ in range(window):
            f = env.fetch()
            for v, x in zip(log, (state, f['actions'], f['labels'])):
                v.append(np.array(x))
            teacher.step_resident(env)
            state = f['obs']
            env.step_resident()
        teacher.synchronize()
        log = (np.stack(log[0], axis=1).astype(np.float32), np.stack(log[1], axis=1).astype(np.int32), np.stack(log[2], axis=1).astype(np.int32))

        def forked():
            pupil.fork_from(base, everyone)
            return pupil
        out['step_%d' % at] = dict(steps=[first, first + window], **_widths_on_a_log(forked, n_agents, log, rounds, max_landmarks))
        # the pupils end where the teacher's closed loop ended (update_control at width 8 leaves kb_fit_steps's bytes)
        out['step_%d' % at]['sizes_equal_the_closed_loops'] = bool(np.array_equal(pupil.dictionary_sizes(), teacher.dictionary_sizes()))
        for h in (env, teacher, base, pupil):
            h.close()
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
    ap.add_argument('--timeout', type=int, default=300)
    ap.add_argument('--only', choices=['a', 'b', 'c', 'd', 'e'])
    ap.add_argument('--at', type=int, default=500, help='leg e: the step around which the closed loop is logged')
    ap.add_argument('--window', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--max-landmarks', type=int, default=1024)
    ap.add_argument('--capacity', type=int, default=2048)
    ap.add_argument('--pool-gb', type=float, default=32.0)
    ap.add_argument('--log', choices=['early', 'late'], help='leg e: one of its two logs only')
    ap.add_argument('--batch-out', default=os.path.join(ROOT, 'profiles', 'fit_steps_batch_record.json'))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_steps_record.json'))
    a = ap.parse_args()
    if a.child in ('a', 'd'):
        return child_fleet(a.agents, a.steps, 'projectron' if a.child == 'a' else 'projectron_plus')
    if a.child == 'b':
        return child_steps_only('g10_kbrl_s0', a.agents, 256 << 10)
    if a.child == 'c':
        return child_steps_only('g15_kbrl_long_s0', 64, 4 << 20)
    if a.child == 'e':
        return child_batch(a.agents, a.steps, a.at, a.window, a.rounds, a.max_landmarks, a.capacity, a.pool_gb, a.log)
    if a.only == 'e':
        rec = dict(what="kb_fit_steps in 'projectron_plus' mode: kb_set_fit_steps_batch at widths 2, 4 and 8 against width 0 in the same "
                        'build, kernel timing on, no threshold attached')
        if os.path.exists(a.batch_out):
            with open(a.batch_out) as f:
                rec.update(json.load(f))
        extra = ['--agents', str(a.agents), '--steps', str(a.steps), '--at', str(a.at), '--window', str(a.window), '--rounds', str(a.rounds),
                 '--max-landmarks', str(a.max_landmarks), '--capacity', str(a.capacity), '--pool-gb', str(a.pool_gb)]
        rec.update(run('e', a.timeout, extra + (['--log', a.log] if a.log else [])))
        os.makedirs(os.path.dirname(a.batch_out), exist_ok=True)
        with open(a.batch_out, 'w') as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write('\n')
        return print(json.dumps(rec))
    rec = dict(statistic='one run per figure, kernel timing on, no threshold')
    if a.only and os.path.exists(a.out):
        with open(a.out) as f:
            rec.update(json.load(f))
    names = dict(a='a_fleet_20_steps', b='b_fleet_120_steps', c='c_g15_64_agents', d='d_fleet_20_steps_projectron_plus')
    for leg in ('a', 'b', 'c', 'd'):
        if a.only in (None, leg):
            rec[names[leg]] = run(leg, a.timeout, ['--agents', str(a.agents), '--steps', str(a.steps)])
            print(json.dumps(rec[names[leg]]), flush=True)
            with open(a.out, 'w') as f:
                json.dump(rec, f, indent=1)
                f.write('\n')


if __name__ == '__main__':
    main()
