"""Projectron.update ON THE DEVICE, stage by stage and path by path (csrc/kb_kbrl.hip), against tests/update_mirror.py.

  (a) one step of kb_update and of kb_fit on a ladder of dictionary sizes in ONE handle: the kernel column, d* = Kinv K_f, delta,
      the branch, every coefficient and every entry of Kinv equal the mirror's as BITS (the mirror is fed what the device held
      before the step); d* keeps the derived forward bound against exact arithmetic on the device's own Kinv.
  (b) the control loop's six ways through the same update -- the one-wave kernel, update_small_kernel, update_heavy_kernel and
      the chip-wide rounds under several cuts of their work line -- leave the same bytes.
  (c) the control loop and kb_fit on the augmented samples of the same log leave the same bytes.

Run with -s for the largest error / bound ratio (DESIGN.md §2 quotes it).
"""
import ctypes as C

import numpy as np
import pytest

import update_mirror as um
from test_gpu_kbrl import _fast_growing_samples

pytestmark = pytest.mark.gpu

GAMMA, ETA, N_PRBS = 1.0, 0.1, 200


def _bind(L):
    """the accessors of the test build (csrc/kb_probe.hip; not part of ranslice._lib's product surface)"""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.kb_dev_get_update_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int32, ip, dp, dp, dp]
    L.kb_dev_get_update_rows.restype = C.c_int
    L.kb_dev_get_scores.argtypes = [vp, dp, dp, ip]
    L.kb_dev_get_scores.restype = C.c_int


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def dev_agent(monkeypatch, *a, **kw):
    from ranslice.kbrl_dev import VecKBRL
    monkeypatch.setenv('RANSLICE_DEV_BUILD', '1')
    ag = VecKBRL(*a, **kw)
    _bind(ag.L)
    return ag


def update_rows(ag, e, s, m, with_parts=True):
    """(K_f [m], d* [m], the tiles' partial sums {(b_i, b_j): 128 doubles}) as the last update of learner (e, s) left them"""
    nb = (m + 63) >> 6
    kf, ds, parts = np.zeros(max(m, 1)), np.zeros(max(m, 1)), np.zeros(max(128 * nb * (nb + 1) // 2, 1))
    got = C.c_int32(-1)
    rc = ag.L.kb_dev_get_update_rows(ag.h, e, s, m, C.byref(got), _p(kf, C.c_double), _p(ds, C.c_double),
                                     _p(parts, C.c_double) if with_parts else None)
    assert rc == 0 and got.value >= m, (rc, got.value, m)
    tiles = [(bi, bj) for bi in range(nb) for bj in range(bi + 1)]
    return kf[:m], ds[:m], {t: parts[128 * i:128 * i + 128] for i, t in enumerate(tiles)}


# ------------------------------------------------------------------ (a) the size ladder
LADDER10 = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 511, 512, 513, 575, 576,
            577, 640, 641]
LADDER3 = [0, 1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193]


def _stream3(n, seed=77, spread=4.0):
    """_fast_growing_samples with three state variables: a dictionary on it reaches some 220 landmarks in 3,000 samples and then
    hardly grows (the cube fills up; a wider cube grows further but leaves scores within rounding of zero, whose sign is not the
    test's subject), so the ladder of three state variables ends at 193: four blocks"""
    rng = np.random.default_rng(seed)
    xs, ys, states = [], [], []
    for i in range(n):
        if states and rng.random() < 0.5:
            s = states[rng.integers(len(states))]
        else:
            s = (rng.random(3) * spread).astype(np.float32)
        states.append(s)
        x = np.append(s, rng.integers(0, N_PRBS + 1) / N_PRBS)
        score = x[:-1].mean() * 0.8 / spread + 0.35 - x[-1]
        ys.append(-1 if score + rng.normal(0, 0.15) > 0 else 1)
        xs.append(x)
    return np.asarray(xs), np.asarray(ys)


def _prefix_lengths(m_after, sizes):
    """samples of the stream after which the dictionary holds exactly m landmarks, for every m of `sizes`"""
    m_after = np.asarray(m_after)
    out = []
    for m in sizes:
        at = np.nonzero(m_after == m)[0]
        assert m == 0 or at.size, 'the stream never holds %d landmarks' % m
        out.append(int(at[0]) + 1 if m else 0)
    return out


def _check_step(ag, e, s, x, want_branch, worst):
    """one kb_predict / kb_update of learner (e, s) on x with the label it does not predict, against the mirror -> the state after"""
    d = ag.dims[s] + 1
    b = ag.learner(e, s, with_kinv=True)
    m = b['m']
    kinv = b['kinv'] if m else np.zeros((0, 0))
    y_pred, f = ag.predict(e, s, x)
    y = -y_pred if y_pred else 1
    br, delta = ag.update(e, s, x, y)
    a = ag.learner(e, s, with_kinv=True)
    mir = um.step(kinv, b['coeff'], b['landmarks'], x, y, GAMMA, ETA)
    tag = ('dims %d' % (d - 1), 'm %d' % m, {1: 'projection', 2: 'insertion'}[mir['branch']])
    if m:
        kf, ds, parts = update_rows(ag, e, s, m)
        assert same(kf, mir['column']), tag + ('K_f', int((bits(kf) != bits(mir['column'])).sum()))
        if not same(ds, mir['dstar']):   # name the stage: the tiles' partial sums, or the combine
            live = lambda b: min(64, m - 64 * b)      # (columns and rows past m: whatever the tile holds, never read)
            bad = [t for t in mir['dpart'] if not same(parts[t][:live(t[1])], mir['dpart'][t][:live(t[1])])
                   or (t in mir['tpart'] and not same(parts[t][64:64 + live(t[0])], mir['tpart'][t][:live(t[0])]))]
            raise AssertionError(tag + ('d*: %d of %d outputs differ' % (int((bits(ds) != bits(mir['dstar'])).sum()), m),
                                        'partial sums differ in tiles %s' % bad[:6] if bad else
                                        'every partial sum equal: the combine'))
        if m >= 2:
            r, units = um.error_ratio(ds, kinv, kf)
            assert r <= 1.0, tag + ('accuracy of d*', r)
            worst[0], worst[1] = max(worst[0], r), max(worst[1], units)
    assert want_branch == mir['branch'] == br, tag + (br, mir['branch'], mir['delta'])
    assert bits(np.float64(delta)) == bits(np.float64(mir['delta'])), tag + ('delta', delta, mir['delta'])
    assert a['m'] == mir['m'], tag
    assert same(a['landmarks'], mir['landmarks']), tag + ('landmarks',)
    assert same(a['coeff'], mir['coeff']), tag + ('coefficients', int((bits(a['coeff']) != bits(mir['coeff'])).sum()))
    assert same(a['kinv'], mir['kinv']), tag + ('Kinv', int((bits(a['kinv']) != bits(mir['kinv'])).sum()))
    assert same(a['kinv'], a['kinv'].T), tag + ('Kinv is not symmetric',)
    return a


def _far_and_near(L, coeff, kinv, pool, rng):
    """a sample of `pool` the dictionary will insert (its residual well above eta, its kernel column not negligible) and a
    near-duplicate of a landmark (projected)"""
    m = len(coeff)
    far = pool[0]
    if m:
        for x in pool:
            k = np.exp(-GAMMA * ((L - x[None]) ** 2).sum(axis=1))
            if 1.0 - k @ (kinv @ k) > 3 * ETA and (m < 8 or k.max() > 0.05):
                far = x
                break
        else:
            raise AssertionError('no sample of the pool would be inserted at m = %d' % m)
    j = int(rng.integers(m + 1))     # (a landmark of the dictionary AFTER the insertion: it may be the new one)
    near = np.vstack([L, far[None]])[j].copy()
    near[:-1] += 0.01
    return far, near


def test_size_ladder_one_step_of_kb_update_and_kb_fit_gives_the_mirrors_bits(monkeypatch):
    """Thirty learners of ten state variables at 0 .. 641 landmarks (ten and eleven blocks: the first sizes at which
    matvec_tri_combine_wide would run a second batch of eight) and sixteen of three state variables at 0 .. 193, grown with kb_fit
    from prefixes of one stream per kind in ONE handle; the same ladder a second time in the handle's other replicas (the twin).
    Every learner takes an insertion and then a projection through kb_predict / kb_update, its twin through kb_fit: K_f, d*, delta,
    branch, coefficients and Kinv are the mirror's bits, the twin's the learner's."""
    n10, n3 = len(LADDER10), len(LADDER3)
    ag = dev_agent(monkeypatch, 2 * n10 + 1, [10, 3], N_PRBS, capacity=1024, gamma=GAMMA, eta=ETA)
    try:
        zero = np.zeros((ag.n_envs, 2), dtype=np.int32)
        ag.reset(zero, zero)
        streams = [_fast_growing_samples(4600), _stream3(3000)]
        pilot = ag.n_envs - 1       # one learner per kind takes the whole stream and says where every size is reached
        r = ag.fit([(pilot, 0), (pilot, 1)], [streams[0][0], streams[1][0]], [streams[0][1], streams[1][1]])
        cut = [_prefix_lengths(r['m'][0], LADDER10), _prefix_lengths(r['m'][1], LADDER3)]
        learners = [(e + t * n10, s) for t in (0, 1) for s, n in ((0, n10), (1, n3)) for e in range(n)]
        sizes = [(LADDER10, LADDER3)[s][e % n10] for e, s in learners]
        r = ag.fit(learners, [streams[s][0][:cut[s][e % n10]] for e, s in learners],
                   [streams[s][1][:cut[s][e % n10]] for e, s in learners])
        got = ag.dictionary_sizes()
        assert [int(got[e, s]) for e, s in learners] == sizes
        rng = np.random.default_rng(3)
        worst = [0.0, 0.0]
        for (e, s), m in zip(learners[:n10 + n3], sizes):
            b = ag.learner(e, s, with_kinv=True)
            tw = ag.learner(e + n10, s, with_kinv=True)
            assert all(m == 0 or same(b[k], tw[k]) for k in ('landmarks', 'coeff', 'kinv')), ('the twin differs before the step', s, m)
            pool = streams[s][0][cut[s][e]:][:400]
            far, near = _far_and_near(b['landmarks'], b['coeff'], b['kinv'] if m else None, pool, rng)
            for x, want in ((far, 2), (near, 1)):
                a = _check_step(ag, e, s, x, want, worst)
                y_pred, f = ag.predict(e + n10, s, x)
                rt = ag.fit([(e + n10, s)], [x[None]], [np.array([-y_pred if y_pred else 1])])
                tw = ag.learner(e + n10, s, with_kinv=True)
                assert int(rt['branch'][0][0]) == want and tw['m'] == a['m'], ('kb_fit', s, m, want)
                for k in ('landmarks', 'coeff', 'kinv'):
                    assert same(a[k], tw[k]), ('kb_fit leaves other bits than kb_update', k, s, m, want)
                if m:
                    ru, rf = update_rows(ag, e, s, m, False), update_rows(ag, e + n10, s, m, False)
                    assert same(ru[0], rf[0]) and same(ru[1], rf[1]), ('kb_fit: K_f or d*', s, m, want)
        print('size ladder: d* error / bound %.3g, largest error %.3g u S_i (bound at 641 landmarks: %.3g u S_i)'
              % (worst[0], worst[1], um.bound_units(641)))
    finally:
        ag.close()


# ------------------------------------------------------------------ (b), (c) the control loop, path by path
AGENTS, STEPS = 24, 60
SETTINGS = {
    'production': None,                                   # the product's library at its defaults
    'rounds1': dict(KBRL_ROUNDS='1'),
    'rounds3': dict(KBRL_ROUNDS='3'),
    'rounds3_grid1': dict(KBRL_ROUNDS='3', KBRL_STREAM_GRID='1'),
    'rounds3_grid3': dict(KBRL_ROUNDS='3', KBRL_STREAM_GRID='3'),
    'rounds3_grid61': dict(KBRL_ROUNDS='3', KBRL_STREAM_GRID='61'),
    'one_wave': dict(KBRL_HEAVY_M='1000000'),             # every learner inline on one wave
    'mixed': dict(KBRL_HEAVY_M='300'),                    # below 300 landmarks inline, the others queued (rounds, then a workgroup each)
}
_runs = {}


def _offset(e):
    """where agent e starts in the recording.  (Agents 0 and 10 start 11 and 22 steps later than the others' rule: from 200 and
    1030 one decision of theirs scores within rounding of zero, which test_control_loop_equals_kb_fit_... excludes.)"""
    return 200 + 83 * e + {0: 11, 10: 22}.get(e, 0)


def _plan(golden_dir):
    """the recording, and per learner (e, s) the sample list that pre-grows it: draws from the recording's own states (any step,
    any slice) with an allocation on the label's side of the recorded one -- between 900 and 13,000 of them, some 100 .. 650
    landmarks -- and then every state the agent is about to be taught on, once under each label at two allocations 61 apart: one
    of the two is a mistake, so the state is inserted or lies within eta of the dictionary's span, and no candidate of the run
    scores within rounding of zero"""
    if 'plan' not in _runs:
        import os
        g = dict(np.load(os.path.join(golden_dir, 'g15_kbrl_long_s0.npz')))
        S = g['state'].reshape(len(g['state']), 5, 10).astype(np.float64)
        learners = [(e, s) for e in range(AGENTS) for s in range(5)]
        X, Y = [], []
        for t, (e, s) in enumerate(learners):
            rng = np.random.default_rng(1000 + t)
            n = int(np.linspace(900, 13000, len(learners))[(37 * t) % len(learners)])
            st, sl = rng.integers(0, len(S), n), rng.integers(0, 5, n)
            a, lab = g['action_in'][st, sl].astype(np.int64), g['labels'][st, sl].astype(np.int64)
            u = rng.random(n)
            a = np.where(lab == 1, a + np.floor(u * (N_PRBS + 1 - a)), np.floor(u * (a + 1))).astype(np.int64)
            win = np.repeat(_offset(e) + np.arange(STEPS + 1), 2)
            aw = g['action_in'][win, s].astype(np.int64)       # label +1 at the higher allocation, -1 at one 61 below: an odd
            aw = np.where(aw >= 100, aw, aw + 61) - 61 * (np.arange(len(win)) % 2)   # distance, no candidate half-way
            X.append(np.vstack([np.column_stack([S[st, sl], a / float(N_PRBS)]), np.column_stack([S[win, s], aw / float(N_PRBS)])]))
            Y.append(np.concatenate([lab, np.tile([1, -1], STEPS + 1)]))
        _runs['plan'] = (g, learners, X, Y)
    return _runs['plan']


def _digest(L):
    import hashlib
    return tuple(hashlib.sha256(np.ascontiguousarray(L[k]).tobytes()).hexdigest() for k in ('landmarks', 'coeff', 'kinv'))


def _make(golden_dir, knobs, dev):
    """a fresh handle of 24 agents of scenario 0 with the pre-grown dictionaries; the knobs are read when it is created"""
    from ranslice.kbrl_dev import VecKBRL
    g, learners, X, Y = _plan(golden_dir)
    with pytest.MonkeyPatch.context() as mp:
        for k in ('KBRL_ROUNDS', 'KBRL_STREAM_GRID', 'KBRL_HEAVY_M', 'RANSLICE_DEV_BUILD'):
            mp.delenv(k, raising=False)
        if dev:
            mp.setenv('RANSLICE_DEV_BUILD', '1')
        for k, v in (knobs or {}).items():
            mp.setenv(k, v)
        ag = VecKBRL(AGENTS, [10] * 5, N_PRBS, accuracy_range=tuple(g['a_range']), capacity=4096, gamma=GAMMA, eta=ETA)
    if dev:
        _bind(ag.L)
    ag.reset(np.tile(g['init_action'], (AGENTS, 1)), np.tile(g['init_sec'], (AGENTS, 1)))
    ag.fit(learners, X, Y)
    return ag


def _control_run(golden_dir, name):
    """STEPS teacher-forced update_control / select_action steps on the recording, agent e from _offset(e) on -> what every step
    returned and what it left"""
    if name in _runs:
        return _runs[name]
    g, learners, _, _ = _plan(golden_dir)
    dev = SETTINGS[name] is not None
    ag = _make(golden_dir, SETTINGS[name], dev)
    try:
        idx = np.array([_offset(e) for e in range(AGENTS)])
        out = dict(sizes=[ag.dictionary_sizes()], hits=[], actions=[], adjusted=[], F=[])
        for i in range(STEPS):
            at = idx + i
            out['hits'].append(ag.update_control(g['state'][at], g['action_in'][at], g['labels'][at]))
            act, adj = ag.select_action(g['state'][at + 1])
            out['actions'].append(act)
            out['adjusted'].append(adj)
            out['sizes'].append(ag.dictionary_sizes())
            if dev:
                F = np.zeros((ag.n_envs * ag.S, 256))
                assert ag.L.kb_dev_get_scores(ag.h, _p(F, C.c_double), None, None) == 0
                out['F'].append(F[:, :N_PRBS + 1].tobytes())
        for k in ('sizes', 'hits', 'actions', 'adjusted'):
            out[k] = np.array(out[k])
        out['final'] = [_digest(ag.learner(e, s, with_kinv=True)) for e, s in learners]
        out['work'] = ag._repair_raw()
    finally:
        ag.close()
    _runs[name] = out
    return out


@pytest.mark.parametrize('name', [n for n in SETTINGS if n != 'production'])
def test_every_control_path_leaves_the_same_bytes(golden_dir, name):
    """120 learners of 100 .. 650 landmarks, more than the eight large ones after which the rounds open on their own, so a wave of
    the two streaming kernels covers several learners, starts and ends inside a dictionary's tiles and takes the tail of one and
    the head of the next; KBRL_STREAM_GRID moves those cuts (4, 12 and 244 waves).  Against the product's library at its
    defaults: hits, actions, `adjusted` and sizes at every step, and landmarks, coefficients and Kinv of every learner at the end, as
    bytes; against the first test-build setting also the scores F of every candidate at every step."""
    ref, run = _control_run(golden_dir, 'production'), _control_run(golden_dir, name)
    for k in ('hits', 'actions', 'adjusted', 'sizes'):
        same_steps = (ref[k].reshape(len(ref[k]), -1) == run[k].reshape(len(run[k]), -1)).all(axis=1)
        assert same_steps.all(), (name, k, 'first at step', int(np.argmin(same_steps)))
    bad = [(t, int(ref['sizes'][-1].reshape(-1)[t])) for t, (u, v) in enumerate(zip(ref['final'], run['final'])) if u != v]
    assert not bad, (name, 'learners (task, landmarks) whose landmarks / coefficients / Kinv differ', bad[:8])
    f0 = _control_run(golden_dir, 'rounds1')['F']
    diff = [i for i, (u, v) in enumerate(zip(f0, run['F'])) if u != v]
    assert not diff, (name, 'F differs from KBRL_ROUNDS=1 at steps', diff[:8])
    w = run['work']
    if name.startswith('rounds'):
        assert w[0] > 0 and w[1] > 0 and w[2] > 0 and w[3] > 0, (name, 'a streaming kernel of the rounds had no work', w[:4])
    if name.startswith('rounds3'):
        w3 = _control_run(golden_dir, 'rounds3')['work']
        assert w[:2] == w3[:2], (name, 'tiles and units of the work line depend on the grid', w[:4], w3[:4])
    if name == 'one_wave':   # (nothing is queued; in 'mixed' the learners of 300 landmarks and more are, and the rounds open for them)
        assert w[0] == 0 and w[1] == 0, (name, 'the rounds ran', w[:4])


def test_control_loop_equals_kb_fit_on_its_augmented_samples(golden_dir):
    """§8f's argument: the control loop's repairs are Projectron.update on the augmented samples in order, so kb_fit of those lists
    (ranslice.kbrl_dev.augmented_samples) on a twin handle leaves the same landmarks, coefficients and Kinv, as bytes.  The two
    sides decide from differently formed scores (the binned F against predict_column's sum), and on an exact tie the control loop
    draws where kb_fit always updates: no decision of the run may have |f| within 1e-9 (1 + sum |k c|) of zero -- asserted on
    kb_fit's own f with sum |k c| <= |c|_1 (k <= 1), |c|_1 taken four times its larger value before and after the run.  The
    lists also say what the run contained: insertions and projections on dictionaries of 192 and of 320 landmarks and more."""
    from ranslice.kbrl_dev import augmented_samples
    g, learners, _, _ = _plan(golden_dir)
    ref = _control_run(golden_dir, 'production')
    ag = _make(golden_dir, None, False)
    try:
        c1 = np.array([np.abs(ag.learner(e, s)['coeff']).sum() for e, s in learners])
        X, Y = [], []
        for e in range(AGENTS):
            at = _offset(e) + np.arange(STEPS)
            xe, ye = augmented_samples(g['state'][at], g['action_in'][at], g['labels'][at], [10] * 5, N_PRBS)
            X += xe
            Y += ye
        r = ag.fit(learners, X, Y)
        assert (ag.dictionary_sizes() == ref['sizes'][-1]).all()
        fin = [ag.learner(e, s, with_kinv=True) for e, s in learners]
        c1 = np.maximum(c1, [np.abs(L['coeff']).sum() for L in fin])
        closest = min(float(np.abs(f).min() / (1e-9 * (1 + 4 * c))) for f, c in zip(r['f'], c1))
        count = {}
        for br, m in zip(r['branch'], r['m']):
            for lo in (192, 320):
                count['insertions', lo] = count.get(('insertions', lo), 0) + int(((br == 2) & (m - 1 >= lo)).sum())
                count['projections', lo] = count.get(('projections', lo), 0) + int(((br == 1) & (m >= lo)).sum())
        s0, s1 = ref['sizes'][0].reshape(-1), ref['sizes'][-1].reshape(-1)
        print('control run: sizes %d .. %d before, %d .. %d after; %s; learners that crossed 192: %d, 320: %d; closest decision '
              '%.3g bands from zero' % (s0.min(), s0.max(), s1.min(), s1.max(), sorted(count.items()),
                                        int(((s0 < 192) & (s1 >= 192)).sum()), int(((s0 < 320) & (s1 >= 320)).sum()), closest))
        assert closest > 1.0, 'a decision of the run is within rounding of zero (%.3g of the band): choose other offsets' % closest
        bad = [(t, L['m']) for t, L in enumerate(fin) if _digest(L) != ref['final'][t]]
        assert not bad, ('learners (task, landmarks) that differ between the control loop and kb_fit', bad[:8])
        assert all(v > 0 for v in count.values()), count
        assert s0.min() < 192 and ((s0 >= 192) & (s0 < 320)).any() and s0.max() >= 320
    finally:
        ag.close()
