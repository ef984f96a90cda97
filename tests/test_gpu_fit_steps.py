"""kb_fit_steps on the device: logs of control steps taught with the augmentation done by the kernel, against the parent's path on a
twin handle -- the same kb_create, kb_reset and seeds, taught by VecKBRL.fit(..., *augmented_samples(...)) -- bit for bit:
landmarks, coefficients, all of Kinv, sizes, statistics, flags (test_gpu_fit.py's _same_handles).  Nothing is compared with
fit_steps itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ranslice.config import make_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_ip, _dp, _fp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
POOL = 256 << 20


def _load(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    cfg = make_config(int(g['scenario']))
    log = (np.asarray(g['state'], dtype=np.float32), np.asarray(g['action_in'], dtype=np.int64), np.asarray(g['labels'], dtype=np.int64))
    return g, [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs, log


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=''):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), what


def _same_learner(la, lb, what=''):
    assert la['m'] == lb['m'], what
    for k in ('landmarks', 'coeff', 'kinv'):
        _same_bits(la[k], lb[k], (what, k))


def _same_handles(a, b):
    """dictionaries (landmarks, coefficients, ALL of Kinv), sizes, statistics and flags of two handles, bit for bit"""
    assert np.array_equal(a.dictionary_sizes(), b.dictionary_sizes())
    assert a.stats() == b.stats()
    assert a.flagged_replicas() == b.flagged_replicas()
    for e in range(a.n_envs):
        for s in range(a.S):
            _same_learner(a.learner(e, s, with_kinv=True), b.learner(e, s, with_kinv=True), (e, s))


def _handles(k, n_envs, dims, n_prbs, g=None, capacity=1024, algorithm='projectron', seeds=None):
    """k handles created and reset alike"""
    from ranslice.kbrl_dev import VecKBRL
    hs = []
    for _ in range(k):
        h = VecKBRL(n_envs, dims, n_prbs, capacity=capacity, pool_bytes=POOL, algorithm=algorithm,
                    **(dict(accuracy_range=tuple(g['a_range'])) if g is not None else {}))
        ia = np.tile(g['init_action'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 10)
        sf = np.tile(g['init_sec'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 3)
        h.reset(ia, sf, seeds=seeds)
        hs.append(h)
    return hs


def _samples(state, action, labels, dims, n_prbs):
    """the parent's statement of a log: per learner augmented_samples of the rows it does not skip (label 0), and the samples per row"""
    from ranslice.kbrl_dev import augmented_samples
    state, action, labels = np.asarray(state, dtype=np.float32), np.asarray(action, dtype=np.int64), np.asarray(labels, dtype=np.int64)
    X, Y, cnt = [], [], []
    whole = augmented_samples(state, action, labels, dims, n_prbs) if (labels != 0).all() else None
    for s in range(len(dims)):
        keep = labels[:, s] != 0
        xs, ys = whole or augmented_samples(state[keep], np.clip(action[keep], 0, n_prbs), np.where(labels[keep] == 0, 1, labels[keep]),
                                            dims, n_prbs)
        c = np.where(labels[:, s] == 1, n_prbs - action[:, s] + 1, np.where(labels[:, s] == -1, action[:, s] + 1, 0))
        assert c.sum() == len(ys[s])
        X.append(xs[s])
        Y.append(ys[s])
        cnt.append(c)
    return X, Y, cnt


def _teach_twin(h, agents, state, action, labels, chunk=0):
    """VecKBRL.fit of augmented_samples of the logs -> {(e, s): fit's outputs for that learner}, {(e, s): samples per row}"""
    learners, X, Y, cnt = [], [], [], {}
    for e, st, ac, lb in zip(agents, state, action, labels):
        xs, ys, cs = _samples(st, ac, lb, h.dims, h.n_prbs)
        for s in range(h.S):
            learners.append((e, s))
            X.append(xs[s])
            Y.append(ys[s])
            cnt[(e, s)] = cs[s]
    out = h.fit(learners, X, Y, chunk=chunk)
    return {ls: {k: out[k][i] for k in out} for i, ls in enumerate(learners)}, cnt


def _row_summaries(per, cnt, m_before=0, upto=2):
    """what fit's per-sample outputs say about every row: changed (branches 1 .. upto), grown (branch 2 and the size rose), m_after"""
    br, m = per['branch'], per['m']
    m_prev = np.concatenate([[m_before], m[:-1]])
    ends = np.cumsum(cnt)
    changed, grown, m_after = (np.zeros(len(cnt), dtype=np.int64) for _ in range(3))
    cur = m_before
    for r, (a, b) in enumerate(zip(ends - cnt, ends)):
        changed[r] = ((br[a:b] >= 1) & (br[a:b] <= upto)).sum()
        grown[r] = ((br[a:b] == 2) & (m[a:b] > m_prev[a:b])).sum()
        cur = m[b - 1] if b > a else cur
        m_after[r] = cur
    return changed, grown, m_after


def _check_summaries(out_i, per, cnt, e, S, upto=2):
    for s in range(S):
        ch, gr, ma = _row_summaries(per[(e, s)], cnt[(e, s)], upto=upto)
        assert np.array_equal(out_i['changed'][:, s], ch), s
        assert np.array_equal(out_i['grown'][:, s], gr), s
        assert np.array_equal(out_i['m'][:, s], ma), s


def _kernel_bound():
    """KB_STEPS_PRE of the build: dictionaries beyond it take the kernel's other path"""
    text = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'kb_kbrl.hip')).read()
    return int(re.search(r'#define KB_STEPS_PRE (\d+)', text).group(1))


# ---------------------------------------------------------------------------------------------- G10: the recordings

@pytest.fixture(scope='module', params=['g10_kbrl_s0', 'g10_kbrl_s2'])
def g10(request, golden_dir):
    """the twin of a whole G10 recording (s0: 120 steps, n_prbs 200, five learners of 10 variables; s2: 150 steps, n_prbs 100,
    learners of 10 and 3 variables): one agent taught by fit on augmented_samples, kept for every test that compares with it"""
    g, dims, n_prbs, log = _load(golden_dir, request.param)
    twin, = _handles(1, 1, dims, n_prbs, g)
    per, cnt = _teach_twin(twin, [0], *[[v] for v in log])
    yield request.param, g, dims, n_prbs, log, twin, per, cnt
    twin.close()


def test_the_recordings_hold_what_the_tests_need(golden_dir):
    """(CPU arithmetic on the fixtures) s0: single-sample rows of both kinds, a dictionary past one shell; s2: mixed widths"""
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g10_kbrl_s0')
    assert state.shape == (120, 50) and n_prbs == 200 and dims == [10] * 5
    assert int(((action == 0) & (labels == -1)).sum()) == 7 and int(((action == 200) & (labels == 1)).sum()) == 1
    assert len(g['landmarks2']) == 67
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g10_kbrl_s2')
    assert state.shape == (150, 22) and n_prbs == 100 and dims == [10, 3, 3, 3, 3]


@pytest.mark.parametrize('chunk', [0, 1, 7, 120])
def test_g10_bits_of_the_twin(g10, chunk):
    """all steps of a G10 recording on one agent, whatever the chunk: the twin's bits, the twin's row summaries, the twin's
    counters; the reference's recorded landmarks exactly and its coefficients within 1e-8 / 1e-9 (test_fit_augment.py's)"""
    name, g, dims, n_prbs, log, twin, per, cnt = g10
    h, = _handles(1, 1, dims, n_prbs, g)
    out = h.fit_steps([0], *[[v] for v in log], chunk=chunk)
    _same_handles(twin, h)
    _check_summaries({k: v[0] for k, v in out.items()}, per, cnt, 0, len(dims))
    wt, wh = twin.fit_time_ms(), h.fit_time_ms()
    for k in ('samples', 'mistakes', 'insertions', 'kernel_evals'):   # (the f_at columns are not counted)
        assert wt[k] == wh[k], k
    assert wh['samples'] == sum(int(c.sum()) for c in cnt.values())
    for s in range(len(dims)):
        L = h.learner(0, s)
        np.testing.assert_array_equal(L['landmarks'], np.atleast_2d(g['landmarks%d' % s]))
        np.testing.assert_allclose(L['coeff'], g['coeff%d' % s], rtol=1e-8, atol=1e-9)
    # what happens INSIDE rows (the twin's per-sample sizes): a learner's first landmark is inserted by a candidate that further
    # candidates of the same row follow -- they run in the float32 regime of one landmark --, later landmarks likewise, and the
    # row in which a learner passes from one landmark to two begins with one.  (In both recordings every learner's SECOND
    # landmark comes from a single-sample row; test_the_second_landmark_in_the_middle_of_a_row makes that case by hand.)
    first_mid = later_mid = one_to_two = False
    for s in range(len(dims)):
        m = per[(0, s)]['m']
        m_prev = np.concatenate([[0], m[:-1]])
        last_of_row = np.zeros(len(m), dtype=bool)
        last_of_row[np.cumsum(cnt[(0, s)])[cnt[(0, s)] > 0] - 1] = True
        first_mid |= bool(((m_prev == 0) & (m == 1) & ~last_of_row).any())
        later_mid |= bool(((m_prev >= 2) & (m > m_prev) & ~last_of_row).any())
        ma = np.concatenate([[0], out['m'][0][:, s]])
        one_to_two |= bool(((ma[:-1] == 1) & (ma[1:] >= 2)).any())
    assert first_mid and later_mid and one_to_two
    if name == 'g10_kbrl_s0':
        assert h.dictionary_sizes()[0, 2] >= 65   # (a second shell)
    h.close()


def test_the_second_landmark_in_the_middle_of_a_row():
    """two hand-made rows on one state, for a learner of 10 and one of 3 variables: +1 at 40 inserts the first landmark with its
    first candidate, -1 at 30 on the SAME state meets f > 0 with its first candidate (a = 0) and inserts the second one, and 30
    candidates follow -- the size passes from 1 to 2 in the middle of a row (asserted on the twin's outputs), the float32 regime
    ends between two candidates, and the new landmark's prefix is formed there"""
    dims, n_prbs = [10, 3], 50
    rng = np.random.default_rng(11)
    state = np.repeat(rng.random((1, 13)).astype(np.float32), 2, axis=0)
    action, labels = np.array([[40, 40], [30, 30]]), np.array([[1, 1], [-1, -1]])
    twin, h = _handles(2, 1, dims, n_prbs, capacity=128)
    per, cnt = _teach_twin(twin, [0], [state], [action], [labels])
    for s in range(2):
        m = per[(0, s)]['m']
        assert cnt[(0, s)].tolist() == [11, 31] and m[0] == 1 and m[10] == 1 and m[11] == 2   # 1 -> 2 with the row's first candidate
    out = h.fit_steps([0], [state], [action], [labels])
    _same_handles(twin, h)
    _check_summaries({k: v[0] for k, v in out.items()}, per, cnt, 0, 2)
    assert (out['f_at'][0][1] > 0.0).all() and (out['y_at'][0][1] == 1).all()      # the -1 row's extra column: f at a = 30
    twin.close()
    h.close()


def test_f_at_is_the_score_before_the_row(golden_dir):
    """f_at of the first 12 rows of G10 s0 against kb_score on a third handle that is taught the rows one fit at a time and scored
    at (state, action / n_prbs) before each; y_at is its sign, 0 where the dictionary is empty"""
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g10_kbrl_s0')
    T, S = 12, len(dims)
    h, third = _handles(2, 1, dims, n_prbs, g)
    out = h.fit_steps([0], [state[:T]], [action[:T]], [labels[:T]])
    learners = [(0, s) for s in range(S)]
    offs = np.concatenate([[0], np.cumsum(dims)])
    empty_seen = False
    for r in range(T):
        q = [np.concatenate([state[r, offs[s]:offs[s + 1]].astype(np.float64), [action[r, s] / n_prbs]])[None] for s in range(S)]
        f, yp = third.score(learners, q)
        sizes = third.dictionary_sizes()[0]
        for s in range(S):
            _same_bits(out['f_at'][0][r, s], f[s][0], (r, s))
            want = 0 if sizes[s] == 0 else int(np.sign(f[s][0]))
            assert out['y_at'][0][r, s] == want == yp[s][0], (r, s)
            empty_seen |= sizes[s] == 0
        X, Y, _ = _samples(state[r:r + 1], action[r:r + 1], labels[r:r + 1], dims, n_prbs)
        third.fit(learners, X, Y)
    assert empty_seen and (out['f_at'][0] != 0.0).any()
    _same_handles(third, h)
    h.close()
    third.close()


# ---------------------------------------------------------------------------------------------- ragged logs, untouched learners

def test_ragged_logs_and_untouched_learners(golden_dir):
    """6 agents, four listed with 0, 1, 2 and 40 rows, label entries set to 0 and one learner's entries all 0: the unlisted agents,
    the zero-row agent and the all-skipped learner keep their contents and the cache of their last kb_predict; the taught
    learners equal the twin and have lost that cache"""
    from ranslice import _lib
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g10_kbrl_s0')
    S = len(dims)
    twin, h = _handles(2, 6, dims, n_prbs, g)
    # some history first, by the parent's path on both handles, so that untouched learners hold something
    pre = _samples(state[100:104], action[100:104], labels[100:104], dims, n_prbs)
    for x in (twin, h):
        x.fit([(e, s) for e in range(6) for s in range(S)], pre[0] * 6, pre[1] * 6)
    m_pre = h.dictionary_sizes()[0].copy()   # (every agent holds the same)
    assert (m_pre > 0).all()
    agents, rows = [4, 1, 5, 2], [0, 1, 2, 40]
    st = [state[:n] for n in rows]
    ac = [action[:n] for n in rows]
    lb = [labels[:n].copy() for n in rows]
    lb[3][:, 3] = 0            # learner 3 of agent 2 skips every row
    lb[3][5:9, 0] = 0          # learner 0 of agent 2 skips four
    lb[3][0, 1] = 0
    lb[2][1, 4] = 0
    ac[3] = ac[3].copy()
    ac[3][6, 0] = n_prbs + 50  # (an action nobody reads: its label is 0)
    still = [(e, s) for e in (0, 3, 4) for s in range(S)] + [(2, 3)]
    taught = [(1, 0), (5, 4), (2, 0), (2, 4)]
    offs = np.concatenate([[0], np.cumsum(dims)])
    point = lambda s: np.concatenate([state[50, offs[s]:offs[s + 1]].astype(np.float64), [0.5]])
    fs = {}
    for x in (twin, h):
        for e, s in still + taught:
            fs[(e, s)] = x.predict(e, s, point(s))[1]
    before = {es: h.learner(*es, with_kinv=True) for es in still}
    out = h.fit_steps(agents, st, ac, lb)
    per, cnt = _teach_twin(twin, agents, st, [np.clip(a, 0, n_prbs) for a in ac], lb)
    _same_handles(twin, h)
    for i, e in enumerate(agents):
        assert out['m'][i].shape == (rows[i], S)
        for s in range(S):
            ch, gr, ma = _row_summaries(per[(e, s)], cnt[(e, s)], m_before=int(m_pre[s]))
            assert np.array_equal(out['changed'][i][:, s], ch) and np.array_equal(out['grown'][i][:, s], gr), (e, s)
            assert np.array_equal(out['m'][i][:, s], ma), (e, s)
    skipped = lb[3] == 0
    assert (out['f_at'][3][skipped] == 0.0).all() and (out['y_at'][3][skipped] == 0).all() and (out['changed'][3][skipped] == 0).all()
    assert (out['m'][3][:, 3] == before[(2, 3)]['m']).all()
    for es in still:
        _same_learner(h.learner(*es, with_kinv=True), before[es], es)
        h.update(es[0], es[1], point(es[1]), -1 if fs[es] > 0 else 1)      # still accepted: the cache of its kb_predict is there
    for e, s in taught:
        with pytest.raises(_lib.RanSliceError) as err:
            h.update(e, s, point(s), 1)
        assert err.value.code == _lib.RS_ESTATE
        h.predict(e, s, point(s))
        h.update(e, s, point(s), 1)
    twin.close()
    h.close()


# ---------------------------------------------------------------------------------------------- Projectron++

@pytest.mark.parametrize('chunk', [0, 3])
@pytest.mark.parametrize('name,steps,need', [('g10_kbrl_s0', 40, {3, 4}), ('g10_kbrl_s2', 60, {1, 2, 3, 4})])
def test_projectron_plus(golden_dir, name, steps, need, chunk):
    """a prefix of each G10 recording in 'projectron_plus' mode: the twin's bits in that mode, and the margin rule really ran"""
    g, dims, n_prbs, log = _load(golden_dir, name)
    log = [v[:steps] for v in log]
    twin, h = _handles(2, 1, dims, n_prbs, g, algorithm='projectron_plus')
    per, cnt = _teach_twin(twin, [0], *[[v] for v in log])
    assert need <= set(np.concatenate([p['branch'] for p in per.values()]).tolist())
    out = h.fit_steps([0], *[[v] for v in log], chunk=chunk)
    _same_handles(twin, h)
    _check_summaries({k: v[0] for k, v in out.items()}, per, cnt, 0, len(dims), upto=3)
    twin.close()
    h.close()


# ---------------------------------------------------------------------------------------------- saturation, ties, large dictionaries

def test_saturation_at_the_capacity(golden_dir):
    """capacity 64 on G10 s0, whose learner 2 would reach 67: branch counts, flag bits and the final dictionaries are the twin's"""
    g, dims, n_prbs, log = _load(golden_dir, 'g10_kbrl_s0')
    twin, h = _handles(2, 1, dims, n_prbs, g, capacity=64)
    per, cnt = _teach_twin(twin, [0], *[[v] for v in log])
    out = h.fit_steps([0], *[[v] for v in log])
    _same_handles(twin, h)
    _check_summaries({k: v[0] for k, v in out.items()}, per, cnt, 0, len(dims))
    assert h.dictionary_sizes()[0, 2] == 64 and out['m'][0][-1, 2] == 64
    fa, fb = twin.flagged_replicas(), h.flagged_replicas()
    assert fa == fb and fb['saturated'] == [0] and fb['pool_full'] == []
    twin.close()
    h.close()


def test_ties_draw_from_the_learners_stream():
    """rows whose state lies 1e3 and more from every landmark of a populated dictionary (test_gpu_fit.py's construction, as log
    rows): f == 0.0 exactly, the first sample of such a row draws from the learner's stream and is inserted; a -1 row's f_at column
    is a tie too and takes NO draw.  The dictionaries are the twin's and the streams stand at the same position afterwards"""
    rng = np.random.default_rng(5)
    dims, n_prbs = [3], 200
    near = rng.random((12, 3)).astype(np.float32)
    far = np.array([[1e3 * (i + 2)] * 3 for i in range(10)], dtype=np.float32)
    state = np.concatenate([near, far])
    action = np.concatenate([rng.integers(90, 110, 12), [198, 1] * 5])[:, None]
    labels = np.concatenate([np.where(rng.random(12) < 0.5, 1, -1), [1, -1] * 5])[:, None]
    seeds = np.array([0x1234567887654321], dtype=np.uint64)
    twin, h = _handles(2, 1, dims, n_prbs, capacity=256, seeds=seeds)
    per, cnt = _teach_twin(twin, [0], [state], [action], [labels])
    out = h.fit_steps([0], [state], [action], [labels], chunk=4)
    p = per[(0, 0)]
    firsts = (np.cumsum(cnt[(0, 0)]) - cnt[(0, 0)])[12:]
    assert (p['f'][firsts] == 0.0).all() and (p['m'][firsts - 1] > 0).all()      # exact ties against a populated dictionary
    assert set(p['y_pred'][firsts].tolist()) == {1, -1}                          # draws, not a constant
    assert (p['branch'][firsts] == 2).all()
    assert (out['f_at'][0][12:, 0] == 0.0).all() and (out['y_at'][0][12:, 0] == 0).all()
    assert (out['grown'][0][12:, 0] >= 1).all()
    _same_handles(twin, h)
    later = np.array([7e4] * 4)
    draws = [(twin.predict(0, 0, later), h.predict(0, 0, later)) for _ in range(6)]
    assert all(u == v and u[1] == 0.0 and u[0] in (1, -1) for u, v in draws)
    twin.close()
    h.close()


def test_dictionaries_beyond_the_prefix_store(golden_dir):
    """the shortest prefix of G15 that takes a learner past the landmarks whose prefixes the kernel keeps in LDS (chosen from the
    recording's set_size): both of the column's paths, and the passage between them, with the twin's bits"""
    bound = _kernel_bound()
    assert bound < 496
    g, dims, n_prbs, log = _load(golden_dir, 'g15_kbrl_long_s0')
    steps = int(np.nonzero((np.asarray(g['set_size'], dtype=np.int64) > bound).any(axis=1))[0][0]) + 1
    log = [v[:steps] for v in log]
    twin, h = _handles(2, 1, dims, n_prbs, g)
    _teach_twin(twin, [0], *[[v] for v in log])
    out = h.fit_steps([0], *[[v] for v in log])
    _same_handles(twin, h)
    assert h.dictionary_sizes().max() > bound and out['m'][0].max() > bound
    assert (out['m'][0][0] <= bound).all()
    twin.close()
    h.close()


# ---------------------------------------------------------------------------------------------- many workgroups, downstream

def test_agents_do_not_meet(golden_dir):
    """64 agents given the same 30 rows in one call (320 workgroups): every agent's dictionaries are agent 0's, and agent 0's are
    the twin's"""
    g, dims, n_prbs, log = _load(golden_dir, 'g10_kbrl_s0')
    log = [v[:30] for v in log]
    S = len(dims)
    twin, = _handles(1, 1, dims, n_prbs, g)
    _teach_twin(twin, [0], *[[v] for v in log])
    h, = _handles(1, 64, dims, n_prbs, g)
    out = h.fit_steps(np.arange(64), *[np.broadcast_to(v, (64,) + v.shape) for v in log])
    zero = [h.learner(0, s, with_kinv=True) for s in range(S)]
    for s in range(S):
        _same_learner(zero[s], twin.learner(0, s, with_kinv=True), s)
        assert zero[s]['m'] > 0
    for e in range(1, 64):
        for s in range(S):
            _same_learner(h.learner(e, s, with_kinv=True), zero[s], (e, s))
        _same_bits(out['f_at'][e], out['f_at'][0], e)
        for k in ('y_at', 'changed', 'grown', 'm'):
            assert np.array_equal(out[k][e], out[k][0]), (e, k)
    assert h.fit_time_ms()['samples'] == 64 * twin.fit_time_ms()['samples']
    twin.close()
    h.close()


def test_select_action_after_the_call(golden_dir):
    """downstream: select_action on the same state takes equal actions, with equal `adjusted`, on the handle and on its twin"""
    g, dims, n_prbs, log = _load(golden_dir, 'g10_kbrl_s0')
    log = [v[:60] for v in log]
    twin, h = _handles(2, 1, dims, n_prbs, g)
    _teach_twin(twin, [0], *[[v] for v in log])
    h.fit_steps([0], *[[v] for v in log])
    for st in (g['final_state'], g['state'][70], g['state'][119]):
        (act_a, adj_a), (act_b, adj_b) = twin.select_action(st[None]), h.select_action(st[None])
        assert np.array_equal(act_a, act_b) and np.array_equal(adj_a, adj_b)
    ca, cb = twin.control(), h.control()
    for k in ca:
        assert np.array_equal(ca[k], cb[k]), k
    twin.close()
    h.close()


# ---------------------------------------------------------------------------------------------- refusals

def _raw(h, agent, first, rows, action=None, labels=None, chunk=0):
    agent = np.ascontiguousarray(agent, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=np.int64)
    n = max(rows, 1)
    state = np.full((n, h.nv), 0.25, dtype=np.float32)
    action = np.ascontiguousarray(np.full((n, h.S), 3) if action is None else action, dtype=np.int32)
    labels = np.ascontiguousarray(np.ones((n, h.S)) if labels is None else labels, dtype=np.int32)
    rc = h.L.kb_fit_steps(h.h, agent.ctypes.data_as(_ip), len(agent), first.ctypes.data_as(C.POINTER(C.c_int64)),
                          state.ctypes.data_as(_fp), action.ctypes.data_as(_ip), labels.ctypes.data_as(_ip), chunk,
                          None, None, None, None, None)
    return rc, h.L.kb_last_error(h.h).decode()


def test_refusals():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    ag = VecKBRL(3, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    rc, why = _raw(ag, [0], [0, 2], 2)
    assert rc == _lib.RS_ESTATE and 'kb_reset' in why
    ag.reset(np.full((3, 2), 10), np.full((3, 2), 2))
    rc, why = _raw(ag, [0, 2], [0, 2, 3], 3)                            # (a good call, so that the handle holds something)
    assert rc == _lib.RS_OK, why
    assert ag.dictionary_sizes().sum() > 0
    blob = ag.save_state()
    two = lambda v, w=1: [[w, w], [w, v]]
    for args, word in ((dict(agent=[0, 1, 0], first=[0, 1, 2, 3], rows=3), 'twice'),
                       (dict(agent=[0, 3], first=[0, 1, 2], rows=2), 'agent'),
                       (dict(agent=[0, -1], first=[0, 1, 2], rows=2), 'agent'),
                       (dict(agent=[0, 1], first=[1, 1, 2], rows=2), 'first[0]'),
                       (dict(agent=[0, 1], first=[0, 2, 1], rows=2), 'decrease'),
                       (dict(agent=[0, 1], first=[0, 1, 2], rows=2, labels=two(2)), '+1'),
                       (dict(agent=[0, 1], first=[0, 1, 2], rows=2, labels=two(-2)), '+1'),
                       (dict(agent=[0, 1], first=[0, 1, 2], rows=2, action=two(51, 3)), 'outside'),
                       (dict(agent=[0, 1], first=[0, 1, 2], rows=2, action=two(-1, 3)), 'outside'),
                       (dict(agent=[0], first=[0, 1], rows=1, chunk=-1), 'chunk')):
        rc, why = _raw(ag, **args)
        assert rc == _lib.RS_EINVAL and word in why, (args, why)
        assert ag.save_state().tobytes() == blob.tobytes(), args            # a refused call changed nothing
    rc, why = _raw(ag, [0, 1], [0, 1, 2], 2, action=two(51, 3), labels=two(0))   # off the grid, but skipped: accepted
    assert rc == _lib.RS_OK, why
    with pytest.raises(_lib.RanSliceError) as e:
        ag.fit_steps([1, 1], np.zeros((2, 1, 13)), np.full((2, 1, 2), 3), np.ones((2, 1, 2)))
    assert e.value.code == _lib.RS_EINVAL
    frozen = [ag.deploy([0, 1]), VecKBRL.load_agents(ag.export_agents([1, 0])), ag.deploy([1, 1, 0], by_reference=True)]
    for h, word in zip(frozen, ('inference-only', 'inference-only', 'by-reference')):
        rc, why = _raw(h, [0], [0, 1], 1)
        assert rc == _lib.RS_ESTATE and word in why, why
        with pytest.raises(_lib.RanSliceError) as e:
            h.fit_steps([0], np.zeros((1, 1, 13)), np.full((1, 1, 2), 3), np.ones((1, 1, 2)))
        assert e.value.code == _lib.RS_ESTATE
        h.close()
    sh = SharedVecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    sh.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    rc, why = _raw(sh, [0], [0, 1], 1)
    assert rc == _lib.RS_ESTATE and 'shared' in why
    sh.close()
    ag.close()
