"""kb_fit / kb_score on the device: the reference's recordings G9, G14 and G10 taught in ONE call each, the bits of the one-by-one
kb_predict / kb_update path sample for sample and entry for entry, and read-only scoring on every kind of handle."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from ranslice.config import make_config

pytestmark = pytest.mark.gpu
TOL = 1e-9
_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=''):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), what


def _one_by_one(ag, learners, X, Y):
    """the parent path: kb_predict, kb_update per sample; -> what fit returns"""
    out = dict(y_pred=[], f=[], branch=[], delta=[], m=[])
    for (e, s), x, y in zip(learners, X, Y):
        n = len(x)
        yp, br, ma = (np.zeros(n, dtype=np.int32) for _ in range(3))
        f, dl = np.zeros(n), np.zeros(n)
        for t in range(n):
            yp[t], f[t] = ag.predict(e, s, x[t])
            br[t], dl[t] = ag.update(e, s, x[t], int(y[t]))
            ma[t] = ag.dictionary_sizes()[e, s]
        for k, v in zip(('y_pred', 'f', 'branch', 'delta', 'm'), (yp, f, br, dl, ma)):
            out[k].append(v)
    return out


def _same_outputs(a, b):
    for k in ('y_pred', 'branch', 'm'):
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(u, v), (k, i, np.nonzero(np.asarray(u) != np.asarray(v))[0][:5])
    for k in ('f', 'delta'):
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            _same_bits(u, v, (k, i))


def _same_handles(a, b):
    """dictionaries (landmarks, coefficients, ALL of Kinv), sizes, statistics and flags of two handles, bit for bit"""
    assert np.array_equal(a.dictionary_sizes(), b.dictionary_sizes())
    assert a.stats() == b.stats()
    assert a.flagged_replicas() == b.flagged_replicas()
    for e in range(a.n_envs):
        for s in range(a.S):
            la, lb = a.learner(e, s, with_kinv=True), b.learner(e, s, with_kinv=True)
            assert la['m'] == lb['m'], (e, s)
            for k in ('landmarks', 'coeff', 'kinv'):
                _same_bits(la[k], lb[k], (e, s, k))


def _check_against_recording(out, g, tag, f_rtol=1e-8, delta_rtol=1e-7):
    """test_projectron_teacher_forced's checks, sample by sample, on what ONE fit call returned for a learner"""
    fr = g[tag + 'f']
    f, yp, br, dl, m = out
    bad = np.abs(f - fr) > np.maximum(f_rtol * np.abs(fr), TOL)    # (pytest.approx(fr, rel, abs), for all samples at once)
    assert not bad.any(), (np.nonzero(bad)[0][:5], f[bad][:5], fr[bad][:5])
    clear = np.abs(fr) > TOL
    assert np.array_equal(yp[clear], g[tag + 'ypred'][clear])
    assert np.array_equal(br, g[tag + 'branch'])
    assert np.array_equal(m, g[tag + 'm'])
    upd = br != 0
    dr = g[tag + 'delta']
    bad = upd & (np.abs(dl - dr) > np.maximum(delta_rtol * np.abs(dr), 1e-9))
    assert not bad.any(), (np.nonzero(bad)[0][:5], dl[bad][:5], dr[bad][:5])


# ---------------------------------------------------------------------------------------------- G9, G14: the recordings in one call

@pytest.fixture(scope='module')
def g9(golden_dir):
    """ONE kb_fit call on a 3-agent handle of (d11, d4) learners: agent 0 learns G9's two streams in full (1,500 / 1,200 samples),
    agent 1 the first sample of d11 (one landmark) and the first four of d4 (two landmarks), agent 2 nothing (empty dictionaries)"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    ag = VecKBRL(3, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
    ag.reset(np.full((3, 2), 10), np.full((3, 2), 3))
    learners = [(0, 0), (0, 1), (1, 0), (1, 1)]
    X = [g['d11_x'], g['d4_x'], g['d11_x'][:1], g['d4_x'][:4]]
    Y = [g['d11_y'], g['d4_y'], g['d11_y'][:1], g['d4_y'][:4]]
    out = ag.fit(learners, X, Y)
    yield ag, out, g
    ag.close()


def test_g9_in_one_call(g9):
    """both G9 streams through ONE kb_fit: every sample held to the reference's recording with test_projectron_teacher_forced's
    tolerances (f 1e-8 relative / 1e-9 absolute, sign where |f| > 1e-9, branch and size exact, delta 1e-7), then the final
    dictionaries: landmarks exact, coefficients 1e-8, Kinv 1e-8 of its scale"""
    ag, out, g = g9
    for i, tag in enumerate(('d11_', 'd4_')):
        _check_against_recording([out[k][i] for k in ('f', 'y_pred', 'branch', 'delta', 'm')], g, tag)
        L = ag.learner(0, i, with_kinv=True)
        assert L['m'] == len(np.atleast_2d(g[tag + 'landmarks']))
        np.testing.assert_array_equal(L['landmarks'], np.atleast_2d(g[tag + 'landmarks']))
        np.testing.assert_allclose(L['coeff'], g[tag + 'coeff'], rtol=1e-8, atol=1e-9)
        kinv = g[tag + 'kinv']
        np.testing.assert_allclose(L['kinv'], kinv, rtol=1e-8, atol=1e-8 * np.abs(kinv).max())
    assert ag.dictionary_sizes().tolist() == [[160, 19], [1, 2], [0, 0]]
    w = ag.fit_time_ms()
    assert w['samples'] == 1500 + 1200 + 1 + 4
    assert w['insertions'] == 160 + 19 + 1 + 2
    assert w['mistakes'] == sum(int((b != 0).sum()) for b in out['branch'])


def test_g14_in_one_call(golden_dir):
    """G14 through ONE kb_fit: 7,000 samples to 790 landmarks -- twelve shell boundaries, the triangle storage -- against the
    recording with test_projectron_long_golden_to_790_landmarks' tolerances: f 1e-8, delta 1e-7, coefficients 1e-7, the Kinv
    digest 1e-6; Kinv symmetric bit for bit"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g14_projectron_long')
    ag = VecKBRL(1, [10], 200, capacity=4096, pool_bytes=256 << 20)
    ag.reset([[10]], [[3]])
    out = ag.fit([(0, 0)], [g['x']], [g['y']])
    _check_against_recording([out[k][0] for k in ('f', 'y_pred', 'branch', 'delta', 'm')], g, '')
    L = ag.learner(0, 0, with_kinv=True)
    assert L['m'] == len(g['landmarks']) == 790
    np.testing.assert_array_equal(L['landmarks'], g['landmarks'])
    np.testing.assert_allclose(L['coeff'], g['coeff'], rtol=1e-7, atol=1e-8)
    kinv = L['kinv']
    scale = np.abs(g['kinv_rows']).max()
    np.testing.assert_allclose(kinv[::16], g['kinv_rows'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(np.diag(kinv), g['kinv_diag'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(kinv @ g['kinv_probes'], g['kinv_kp'], rtol=1e-6, atol=1e-6 * np.abs(g['kinv_kp']).max())
    assert np.array_equal(kinv, kinv.T)
    p = ag.pool()
    assert p['saturated'] == 0 and p['pool_full'] == 0
    ag.close()


# ---------------------------------------------------------------------------------------------- bits against the one-by-one path

def _mixed_streams(golden_dir):
    g9_, g14 = _load(golden_dir, 'g9_projectron'), _load(golden_dir, 'g14_projectron_long')
    learners = [(0, 0), (0, 1), (1, 0)]
    X = [g9_['d11_x'][:400], g9_['d4_x'][:400], g14['x'][:200]]
    Y = [g9_['d11_y'][:400], g9_['d4_y'][:400], g14['y'][:200]]
    return learners, X, Y


@pytest.fixture(scope='module')
def one_by_one_mixed(golden_dir):
    """handle A: the first 400 of G9's d11 stream, 400 of its d4 stream and the first 200 of G14 (a third learner), sample by sample"""
    from ranslice.kbrl_dev import VecKBRL
    learners, X, Y = _mixed_streams(golden_dir)
    a = VecKBRL(2, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
    a.reset(np.full((2, 2), 10), np.full((2, 2), 3))
    ref = _one_by_one(a, learners, X, Y)
    yield a, ref
    a.close()


@pytest.mark.parametrize('chunk', [1, 7, 0])
def test_bits_against_the_one_by_one_path(golden_dir, one_by_one_mixed, chunk):
    """handle B, one kb_fit, same seeds: every returned f, y_pred, branch, delta, m and the whole of every dictionary (landmarks,
    coefficients, Kinv), the statistics, flags and sizes are those of handle A bit for bit -- across 1 -> 2 landmarks and
    64 -> 65 (a second shell), whatever the chunk"""
    from ranslice.kbrl_dev import VecKBRL
    a, ref = one_by_one_mixed
    learners, X, Y = _mixed_streams(golden_dir)
    b = VecKBRL(2, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
    b.reset(np.full((2, 2), 10), np.full((2, 2), 3))
    out = b.fit(learners, X, Y, chunk=chunk)
    assert ref['m'][0][0] == 1 and ref['m'][0].max() >= 65 and (ref['m'][0] == 2).any()
    _same_outputs(out, ref)
    _same_handles(a, b)
    # the cache of the last predict is gone: an update without a fresh predict is refused, as after any change of the dictionary
    from ranslice import _lib
    with pytest.raises(_lib.RanSliceError) as e:
        b.update(0, 0, X[0][0], 1)
    assert e.value.code == _lib.RS_ESTATE
    b.close()


def test_ragged_lists_and_untouched_learners(golden_dir):
    """6 agents x 2 learners, sample counts {0, 1, 2, 65, 130}, four learners not listed: the unlisted and the zero-sample learners
    are bit for bit what they were (dictionaries with Kinv, control state), the others equal the one-by-one path"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    src = {0: (g['d11_x'], g['d11_y']), 1: (g['d4_x'], g['d4_y'])}
    hs = []
    for _ in range(2):
        h = VecKBRL(6, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
        h.reset(np.full((6, 2), 10), np.full((6, 2), 3))
        hs.append(h)
    a, b = hs
    # some history first, so that untouched learners hold something: 12 samples for every learner of the even agents
    pre = [(e, s) for e in (0, 2, 4) for s in (0, 1)]
    PX = [src[s][0][100 * e:100 * e + 12] for e, s in pre]
    PY = [src[s][1][100 * e:100 * e + 12] for e, s in pre]
    _same_outputs(b.fit(pre, PX, PY), _one_by_one(a, pre, PX, PY))
    counts = {(0, 0): 65, (0, 1): 0, (1, 0): 1, (1, 1): 2, (2, 0): 130, (3, 1): 65, (4, 0): 0, (5, 1): 130}
    learners = list(counts)
    X = [src[s][0][700:700 + n] for (e, s), n in counts.items()]
    Y = [src[s][1][700:700 + n] for (e, s), n in counts.items()]
    still = [(e, s) for e in range(6) for s in range(2) if counts.get((e, s), 0) == 0]
    assert len(still) == 6
    before = {es: b.learner(*es, with_kinv=True) for es in still}
    ctl_before = b.control()
    out = b.fit(learners, X, Y)
    ref = _one_by_one(a, learners, X, Y)
    _same_outputs(out, ref)
    _same_handles(a, b)
    for es in still:
        now = b.learner(*es, with_kinv=True)
        assert now['m'] == before[es]['m']
        for k in ('landmarks', 'coeff', 'kinv'):
            _same_bits(now[k], before[es][k], (es, k))
    ctl = b.control()
    for k in ctl:
        assert np.array_equal(ctl[k], ctl_before[k]), k
    # a zero-sample learner keeps the cache of its last predict too, and scoring leaves it alone: its update is still accepted
    yp, f = b.predict(4, 0, src[0][0][3])
    b.fit([(4, 0), (5, 0)], [src[0][0][:0], src[0][0][:3]], [src[0][1][:0], src[0][1][:3]])
    assert b.score([(4, 0)], [src[0][0][3:4]])[0][0][0] == f
    b.update(4, 0, src[0][0][3], -1 if f > 0 else 1)
    a.close()
    b.close()


def test_ties_draw_from_the_learners_stream(golden_dir):
    """samples 1e3 and more away from a populated dictionary in every coordinate: every kernel value underflows, f == 0.0 exactly,
    and y_pred is the learner's tie stream -- the draws of the one-by-one path under the same seeds, and the stream stands at
    the same position afterwards"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    far = np.array([[1e3 * (i + 2)] * 4 for i in range(10)])     # far from the dictionary AND from each other (they are inserted)
    X = [np.concatenate([g['d4_x'][:30], far])]
    Y = [np.concatenate([g['d4_y'][:30], np.array([1, -1] * 5, dtype=np.int8)])]
    seeds = np.array([0x1234567887654321], dtype=np.uint64)
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [3], 200, capacity=256, pool_bytes=64 << 20)
        h.reset([[10]], [[3]], seeds=seeds)
        hs.append(h)
    a, b = hs
    ref = _one_by_one(a, [(0, 0)], X, Y)
    out = b.fit([(0, 0)], X, Y, chunk=4)
    _same_outputs(out, ref)
    assert (out['f'][0][30:] == 0.0).all() and (out['m'][0][29] > 0)
    assert set(out['y_pred'][0][30:].tolist()) == {1, -1}          # draws, not a constant
    assert (out['branch'][0][30:] == 2).all()                      # delta = 1: each far sample becomes a landmark
    _same_handles(a, b)
    later = np.array([7e4] * 4)
    draws = [(a.predict(0, 0, later), b.predict(0, 0, later)) for _ in range(6)]
    assert all(u == v and u[1] == 0.0 and u[0] in (1, -1) for u, v in draws)
    a.close()
    b.close()


def test_saturation_at_the_capacity(golden_dir):
    """capacity 64 and a stream that would insert 100: branch codes, flag bits and the final dictionary are the one-by-one path's"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    X, Y = [g['d11_x'][:600]], [g['d11_y'][:600]]
    assert g['d11_m'][599] > 90
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [10], 200, capacity=64, pool_bytes=64 << 20)
        h.reset([[10]], [[3]])
        hs.append(h)
    a, b = hs
    ref = _one_by_one(a, [(0, 0)], X, Y)
    out = b.fit([(0, 0)], X, Y)
    _same_outputs(out, ref)
    assert out['m'][0][-1] == 64 and (out['branch'][0][out['m'][0] == 64] != 2)[1:].all()
    _same_handles(a, b)
    fa, fb = a.flagged_replicas(), b.flagged_replicas()
    assert fa == fb and fb['saturated'] == [0] and fb['pool_full'] == []
    a.close()
    b.close()


def test_off_grid_and_non_float32_coordinates(golden_dir):
    """samples whose last coordinate is off the candidate grid and whose state coordinates are not float32 values, mixed with ones
    that are: the marks (f32bad, grid index, chains) are what kb_update leaves -- the dictionaries agree bit for bit and a following
    select_action takes the same actions on both handles"""
    from ranslice.kbrl_dev import VecKBRL
    rng = np.random.default_rng(77)
    n_prbs, n = 50, 120
    X, Y = [], []
    for d in (10, 3):
        st = rng.random((n, d))
        st[::2] = st[::2].astype(np.float32)                        # every other sample: float32 observations
        last = rng.integers(0, n_prbs + 1, n) / n_prbs
        last[::3] = rng.random(len(last[::3]))                      # every third: off the grid
        x = np.concatenate([st, last[:, None]], axis=1)
        X.append(x)
        Y.append(np.where(x[:, :d].mean(axis=1) < x[:, d] + 0.2, 1, -1).astype(np.int8))
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [10, 3], n_prbs, capacity=256, pool_bytes=64 << 20)
        h.reset([[10, 10]], [[2, 2]])
        hs.append(h)
    a, b = hs
    learners = [(0, 0), (0, 1)]
    ref = _one_by_one(a, learners, X, Y)
    out = b.fit(learners, X, Y, chunk=50)
    _same_outputs(out, ref)
    assert out['m'][0][-1] > 10 and out['m'][1][-1] > 5
    _same_handles(a, b)
    for k in range(4):
        state = rng.random((1, 13)).astype(np.float32)
        (act_a, adj_a), (act_b, adj_b) = a.select_action(state), b.select_action(state)
        assert np.array_equal(act_a, act_b) and np.array_equal(adj_a, adj_b), k
    ca, cb = a.control(), b.control()
    for k in ca:
        assert np.array_equal(ca[k], cb[k]), k
    a.close()
    b.close()


def test_closed_loop_after_a_fit(golden_dir):
    """the augmented G10 log (120 recorded steps of 5 learners) fitted into a 1-agent handle: the landmarks are the reference's
    recorded landmarks0..4 exactly, the coefficients within 1e-8; then select_action on G10's final state takes the action of the
    oracle agent taught the same samples"""
    from ranslice.kbrl_dev import VecKBRL, augmented_samples
    g = _load(golden_dir, 'g10_kbrl_s0')
    cfg = make_config(0)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    X, Y = augmented_samples(g['state'], g['action_in'], g['labels'], dims, n_prbs)
    ag = VecKBRL(1, dims, n_prbs, accuracy_range=tuple(g['a_range']), pool_bytes=256 << 20)
    ag.reset(g['init_action'][None], g['init_sec'][None])
    ag.fit([(0, s) for s in range(len(dims))], X, Y)
    oa = po.OracleKBRL(dims, n_prbs, g['init_action'], g['init_sec'], accuracy_range=tuple(g['a_range']))
    oa.set_seed(0)
    for s in range(len(dims)):
        for x, y in zip(X[s], Y[s]):
            oa.predict(s, x)
            oa.update(s, x, int(y))
    for s in range(len(dims)):
        L = ag.learner(0, s)
        np.testing.assert_array_equal(L['landmarks'], np.atleast_2d(g['landmarks%d' % s]))
        np.testing.assert_allclose(L['coeff'], g['coeff%d' % s], rtol=1e-8, atol=1e-9)
    act, adj = ag.select_action(g['final_state'][None])
    oact, oadj = oa.select_action(g['final_state'])
    assert np.array_equal(act[0], oact) and adj[0] == oadj
    ag.close()


# ---------------------------------------------------------------------------------------------- refusals

def _raw_fit(h, task, first, n_rows, y=None, chunk=0):
    task = np.ascontiguousarray(task, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=np.int64)
    x = np.full((max(n_rows, 1), 16), 0.25)
    y = np.ones(max(n_rows, 1), dtype=np.int8) if y is None else np.ascontiguousarray(y, dtype=np.int8)
    rc = h.L.kb_fit(h.h, task.ctypes.data_as(_ip), len(task), first.ctypes.data_as(C.POINTER(C.c_int64)), x.ctypes.data_as(_dp),
                    y.ctypes.data_as(C.POINTER(C.c_int8)), chunk, None, None, None, None, None)
    return rc, h.L.kb_last_error(h.h).decode()


def test_refusals(golden_dir):
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    ag = VecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    rc, why = _raw_fit(ag, [0], [0, 2], 2)
    assert rc == _lib.RS_ESTATE and 'kb_reset' in why
    ag.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    for args, word in ((dict(task=[0, 1, 0], first=[0, 1, 2, 3], n_rows=3), 'twice'),
                       (dict(task=[0, 1], first=[0, 1, 2], n_rows=2, y=[1, 0]), '+1'),
                       (dict(task=[0, 1], first=[0, 1, 2], n_rows=2, y=[1, 2]), '+1'),
                       (dict(task=[0, 1], first=[0, 2, 1], n_rows=2), 'decrease'),
                       (dict(task=[0, 4], first=[0, 1, 2], n_rows=2), 'learner'),
                       (dict(task=[0], first=[0, 1], n_rows=1, chunk=-1), 'chunk')):
        rc, why = _raw_fit(ag, **args)
        assert rc == _lib.RS_EINVAL and word in why, (args, why)
    assert ag.dictionary_sizes().sum() == 0                        # a refused call taught nothing
    with pytest.raises(_lib.RanSliceError) as e:
        ag.fit([(0, 0), (0, 0)], [np.zeros((1, 11))] * 2, [[1], [1]])
    assert e.value.code == _lib.RS_EINVAL
    ag.fit([(0, 0), (1, 1)], [np.full((3, 11), 0.5), np.full((2, 4), 0.5)], [[1, -1, 1], [-1, 1]])
    frozen = [ag.deploy([0, 1]), VecKBRL.load_agents(ag.export_agents([1, 0])), ag.deploy([1, 1, 0], by_reference=True)]
    for h, word in zip(frozen, ('inference-only', 'inference-only', 'by-reference')):
        rc, why = _raw_fit(h, [0], [0, 1], 1)
        assert rc == _lib.RS_ESTATE and word in why, why
        with pytest.raises(_lib.RanSliceError) as e:
            h.fit([(0, 0)], [np.zeros((1, 11))], [[1]])
        assert e.value.code == _lib.RS_ESTATE
        h.close()
    sh = SharedVecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    sh.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    rc, why = _raw_fit(sh, [0], [0, 1], 1)
    assert rc == _lib.RS_ESTATE and 'shared' in why
    with pytest.raises(_lib.RanSliceError) as e:
        sh.fit([(0, 0)], [np.zeros((1, 11))], [[1]])
    assert e.value.code == _lib.RS_ESTATE
    f, yp = sh.score([(0, 0), (1, 1)], [np.zeros((2, 11)), np.zeros((1, 4))])   # score works there (empty dictionaries)
    assert [v.tolist() for v in f] == [[0.0, 0.0], [0.0]] and [v.tolist() for v in yp] == [[0, 0], [0]]
    sh.close()
    ag.close()


# ---------------------------------------------------------------------------------------------- kb_score

def _queries(g):
    """query sets of 1, 7, 8, 9 and 100 points (the edges of an 8-query block) for each of the five kinds of dictionary of the g9
    handle -- 160, 19, 1, 2 and 0 landmarks --, so every task repeats five times; each set of 9 or more holds a point 1e3 away
    (every kernel value underflows: an exact tie)"""
    learners, X = [], []
    for k, nq in enumerate((1, 7, 8, 9, 100)):
        for e, s in ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1)):
            src = g['d11_x'] if s == 0 else g['d4_x']
            x = src[50 * k + 7 * e:50 * k + 7 * e + nq].copy()
            if nq >= 9:
                x[nq - 2] = 1e3
            learners.append((e, s))
            X.append(x)
    return learners, X


def test_score_on_a_learning_handle(g9):
    """f is kb_predict's bit for bit, query by query, on dictionaries of 160, 19, 1, 2 and 0 landmarks; the handle's kb_save_state
    bytes are the same before and after the call; y_pred is 0 on an underflow tie and on the empty dictionary"""
    ag, _, g = g9
    learners, X = _queries(g)
    before = ag.save_state()
    f, yp = ag.score(learners, X)
    after = ag.save_state()
    assert np.array_equal(before, after)
    for (e, s), x, fi, yi in zip(learners, X, f, yp):
        m = ag.dictionary_sizes()[e, s]
        want = np.array([ag.predict(e, s, q)[1] for q in x])
        _same_bits(fi, want, (e, s, len(x)))
        assert np.array_equal(yi, np.sign(fi).astype(np.int32))
        if m == 0:
            assert (fi == 0.0).all() and (yi == 0).all()
        if len(x) >= 9:
            assert fi[len(x) - 2] == 0.0 and yi[len(x) - 2] == 0
        if m > 2:
            assert (fi != 0.0).sum() >= len(x) - 1 and set(yi.tolist()) <= {1, -1, 0}


def test_score_on_deployed_handles(g9):
    """kb_deploy and kb_deploy_ref of the g9 handle with agent 0 three times in the index: the scores are the source's bit for
    bit; kb_predict on the by-reference handle is still refused"""
    from ranslice import _lib
    ag, _, g = g9
    index = [0, 1, 0, 2, 0]
    learners, X = _queries(g)
    f_src, yp_src = ag.score(learners, X)
    by_agent = {}
    for (e, s), x, f, yp in zip(learners, X, f_src, yp_src):
        by_agent.setdefault((e, s), []).append((x, f, yp))
    for by_ref in (False, True):
        d = ag.deploy(index, by_reference=by_ref)
        dl, dX, want = [], [], []
        for j, e in enumerate(index):
            for s in range(2):
                for x, f, yp in by_agent[(e, s)]:
                    dl.append((j, s))
                    dX.append(x)
                    want.append((f, yp))
        fd, ypd = d.score(dl, dX)
        for (f, yp), fi, yi in zip(want, fd, ypd):
            _same_bits(fi, f)
            assert np.array_equal(yi, yp)
        if by_ref:
            with pytest.raises(_lib.RanSliceError) as e:
                d.predict(0, 0, g['d11_x'][0])
            assert e.value.code == _lib.RS_ESTATE
        else:
            assert d.predict(2, 0, X[0][0])[1] == f_src[0][0]     # replica 2 is agent 0 again
        d.close()


def test_score_against_the_oracle(g9):
    """against OracleKBRL.predict on the dictionary its own lock-step updates built from the same 1,500 samples:
    |f - f_oracle| <= 1e-9 (1 + sum |k c|), the sign equal wherever |f| exceeds that bound"""
    ag, _, g = g9
    oa = po.OracleKBRL([10], 200, [10], [3], capacity=1024)
    oa.set_seed(0)
    for x, y in zip(g['d11_x'], g['d11_y']):
        oa.predict(0, x)
        oa.update(0, x, int(y))
    L = ag.learner(0, 0)
    assert oa.m(0) == L['m'] == 160
    rng = np.random.default_rng(5)
    Q = np.concatenate([g['d11_x'][:60], rng.random((40, 11))])
    f, yp = ag.score([(0, 0)], [Q])
    k = np.exp(-1.0 * ((L['landmarks'][None, :, :] - Q[:, None, :]) ** 2).sum(axis=2))
    bound = TOL * (1.0 + (np.abs(k * L['coeff'][None, :])).sum(axis=1))
    n_clear = 0
    for q in range(len(Q)):
        oy, of = oa.predict(0, Q[q])
        assert abs(f[0][q] - of) <= bound[q], q
        if abs(of) > bound[q]:
            assert yp[0][q] == oy, q
            n_clear += 1
    assert n_clear >= 90
