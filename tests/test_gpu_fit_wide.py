"""kb_fit's chip-wide rounds on the device (kb_set_fit_wide; csrc/kb_fit_wide.hip): twin handles, one fitted by the
one-workgroup kernel and one with the wide path on, held to EQUAL BYTES in every returned array, in every dictionary (landmarks,
coefficients, all of Kinv), in sizes, flags, statistics and kb_fit_time_ms's counters; kb_fit_wide_info equal to the counters
tests/fit_wide_mirror.py derives from where the mistakes are."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_wide_mirror as fw   # noqa: E402

pytestmark = pytest.mark.gpu


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_outputs(a, b):
    for k in ('y_pred', 'branch', 'm'):
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(u, v), (k, i, np.nonzero(np.asarray(u) != np.asarray(v))[0][:5])
    for k in ('f', 'delta'):
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            assert u.shape == v.shape and np.array_equal(_bits(u), _bits(v)), (k, i, np.nonzero(_bits(u) != _bits(v))[0][:5])


def _same_handles(a, b):
    """dictionaries (landmarks, coefficients, ALL of Kinv), sizes, flags, statistics and the last fit's counters, bit for bit; the
    control loop's repair counters untouched on both"""
    assert np.array_equal(a.dictionary_sizes(), b.dictionary_sizes())
    assert a.stats() == b.stats()
    assert a.flagged_replicas() == b.flagged_replicas()
    ta, tb = a.fit_time_ms(), b.fit_time_ms()
    for k in ('samples', 'mistakes', 'insertions', 'kernel_evals'):
        assert ta[k] == tb[k], (k, ta, tb)
    assert a._repair_raw() == b._repair_raw() == [0] * 8
    for e in range(a.n_envs):
        for s in range(a.S):
            la, lb = a.learner(e, s, with_kinv=True), b.learner(e, s, with_kinv=True)
            assert la['m'] == lb['m'], (e, s)
            for k in ('landmarks', 'coeff', 'kinv'):
                assert np.array_equal(_bits(la[k]), _bits(lb[k])), (e, s, k)


def _info(h):
    w = h.fit_wide_info()
    return [w['samples'], w['matvecs'], w['tiles'], w['scan_evals']]


def _expected(out, m0, chunk, min_landmarks, window):
    tot = [0, 0, 0, 0]
    for br, m, z in zip(out['branch'], out['m'], m0):
        c = fw.counters(br, m, z, chunk=chunk, min_landmarks=min_landmarks, window=window)
        tot = [u + v for u, v in zip(tot, c)]
    return tot


# ---------------------------------------------------------------------------------------------- all of G14, one learner

def _g14_handle():
    from ranslice.kbrl_dev import VecKBRL
    h = VecKBRL(1, [10], 200, capacity=4096, pool_bytes=256 << 20)
    h.reset([[10]], [[3]])
    return h


@pytest.fixture(scope='module')
def g14_narrow(golden_dir):
    """the narrow path's result, computed once and left alone: 7,000 samples to 790 landmarks (13 blocks, 91 tiles)"""
    g = _load(golden_dir, 'g14_projectron_long')
    a = _g14_handle()
    out = a.fit([(0, 0)], [g['x']], [g['y']])
    assert a.fit_wide == (0, 0) and _info(a) == [0, 0, 0, 0]
    assert out['m'][0][-1] == 790 and (out['m'][0] == 2).any() and (out['m'][0] == 65).any() and (out['m'][0] == 129).any()
    yield g, a, out
    a.close()


@pytest.mark.parametrize('min_landmarks,window,chunk', [(2, 0, 0), (2, 1, 7), (2, 3, 7), (65, 0, 0), (800, 0, 0)])
def test_g14_wide_is_the_narrow_path_bit_for_bit(g14_narrow, min_landmarks, window, chunk):
    """across 1 -> 2 landmarks, 64 -> 65 (a second shell), 128 -> 129 and on to 13 blocks, for the default window and chunk, for
    windows of 1 and 3 under chunks of 7, for a threshold of 65 and for one the dictionary never reaches (no rounds at all)"""
    g, a, ref = g14_narrow
    b = _g14_handle()
    b.set_fit_wide(min_landmarks, window)
    assert b.fit_wide == (min_landmarks, window)
    out = b.fit([(0, 0)], [g['x']], [g['y']], chunk=chunk)
    _same_outputs(out, ref)
    _same_handles(a, b)
    want = _expected(ref, [0], chunk, min_landmarks, window)
    assert _info(b) == want
    if min_landmarks == 800:
        assert want == [0, 0, 0, 0]
    else:
        assert want[0] > 6000 and want[1] > 700 and want[2] > 5 * want[1]   # nearly all of it went wide, through many tiles
    b.close()


# ---------------------------------------------------------------------------------------------- five learners in one call, ragged

@pytest.fixture(scope='module')
def ragged(golden_dir):
    """twin 3-agent handles of (d11, d4) learners.  Agent 2's d11 learner already holds 200 landmarks (an earlier, narrow call on
    both).  Then ONE call: G9's d11 and d4 streams (agent 0), 600 samples of G14 (agent 1, d11), no samples (agent 1, d4), the
    next 500 samples of G14 (agent 2, d11).  Threshold 65, chunks of 128: d4 stays narrow throughout, d11 and the G14 prefix change
    path at a chunk boundary, the fifth is wide from its first chunk -- narrow and wide learners share chunks, and up to three wide
    learners share the work lines."""
    from ranslice.kbrl_dev import VecKBRL
    g9, g14 = _load(golden_dir, 'g9_projectron'), _load(golden_dir, 'g14_projectron_long')
    n_pre = int(np.nonzero(g14['m'] == 200)[0][0]) + 1
    hs = []
    for _ in range(2):
        h = VecKBRL(3, [10, 3], 200, capacity=1024, pool_bytes=512 << 20)
        h.reset(np.full((3, 2), 10), np.full((3, 2), 3))
        h.fit([(2, 0)], [g14['x'][:n_pre]], [g14['y'][:n_pre]])
        hs.append(h)
    a, b = hs
    assert a.dictionary_sizes()[2, 0] == 200
    learners = [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)]
    X = [g9['d11_x'], g9['d4_x'], g14['x'][:600], g9['d4_x'][:0], g14['x'][n_pre:n_pre + 500]]
    Y = [g9['d11_y'], g9['d4_y'], g14['y'][:600], g9['d4_y'][:0], g14['y'][n_pre:n_pre + 500]]
    ref = a.fit(learners, X, Y, chunk=128)
    b.set_fit_wide(65)
    out = b.fit(learners, X, Y, chunk=128)
    yield a, b, ref, out, X
    a.close()
    b.close()


def test_five_ragged_learners_narrow_and_wide_in_one_call(ragged):
    a, b, ref, out, X = ragged
    _same_outputs(out, ref)
    _same_handles(a, b)
    want = _expected(ref, [0, 0, 0, 0, 200], 128, 65, 0)
    assert _info(b) == want
    per = [fw.counters(br, m, z, chunk=128, min_landmarks=65) for br, m, z in zip(ref['branch'], ref['m'], [0, 0, 0, 0, 200])]
    assert per[0][0] > 0 and per[1] == [0, 0, 0, 0] and per[2][0] > 0 and per[3] == [0, 0, 0, 0] and per[4][0] == 500
    assert per[0][0] < 1500 and per[2][0] < 600      # both began narrow


def test_after_a_wide_fit(ragged):
    """the cache of the last predict is gone on the learners that were taught (kb_update answers RS_ESTATE until a new kb_predict),
    a learner without samples keeps its own, and select_action on the same state takes the same actions on both handles"""
    from ranslice import _lib
    a, b, _, _, X = ragged
    for h in (a, b):
        for (e, s), x in (((0, 0), X[0][0]), ((2, 0), X[4][0])):
            with pytest.raises(_lib.RanSliceError) as err:
                h.update(e, s, x, 1)
            assert err.value.code == _lib.RS_ESTATE
    rng = np.random.default_rng(3)
    for k in range(3):
        state = rng.random((3, 13)).astype(np.float32)
        (act_a, adj_a), (act_b, adj_b) = a.select_action(state), b.select_action(state)
        assert np.array_equal(act_a, act_b) and np.array_equal(adj_a, adj_b), k
    x = X[0][5]
    assert a.predict(0, 0, x) == b.predict(0, 0, x)
    assert a.update(0, 0, x, -1) == b.update(0, 0, x, -1)


# ---------------------------------------------------------------------------------------------- ties, saturation

def test_an_exact_tie_in_the_wide_path(golden_dir):
    """samples 1e3 and more away from a populated dictionary: every kernel value underflows, f == 0.0 exactly, each is a mistake
    whose y_pred is a draw of the learner's tie stream -- the same draws as the narrow path, and the streams stand at the same
    position afterwards"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    far = np.array([[1e3 * (i + 2)] * 4 for i in range(10)])
    X = [np.concatenate([g['d4_x'][:30], far, g['d4_x'][30:40]])]
    Y = [np.concatenate([g['d4_y'][:30], np.array([1, -1] * 5, dtype=np.int8), g['d4_y'][30:40]])]
    seeds = np.array([0x1234567887654321], dtype=np.uint64)
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [3], 200, capacity=256, pool_bytes=64 << 20)
        h.reset([[10]], [[3]], seeds=seeds)
        hs.append(h)
    a, b = hs
    ref = a.fit([(0, 0)], X, Y, chunk=4)
    b.set_fit_wide(2, 3)
    out = b.fit([(0, 0)], X, Y, chunk=4)
    _same_outputs(out, ref)
    assert (out['f'][0][30:40] == 0.0).all() and out['m'][0][29] >= 2
    assert set(out['y_pred'][0][30:40].tolist()) == {1, -1} and (out['branch'][0][30:40] == 2).all()
    _same_handles(a, b)
    want = _expected(ref, [0], 4, 2, 3)
    assert _info(b) == want and want[1] >= 10
    later = np.array([7e4] * 4)
    draws = [(a.predict(0, 0, later), b.predict(0, 0, later)) for _ in range(6)]
    assert all(u == v and u[1] == 0.0 and u[0] in (1, -1) for u, v in draws)
    a.close()
    b.close()


def test_saturation_at_a_capacity_of_70(golden_dir):
    """the dictionary fills up inside the wide path: the flag bits, branch 1 from then on and the sizes are the narrow path's"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    X, Y = [g['d11_x'][:600]], [g['d11_y'][:600]]
    assert g['d11_m'][599] > 90
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [10], 200, capacity=70, pool_bytes=64 << 20)
        h.reset([[10]], [[3]])
        hs.append(h)
    a, b = hs
    ref = a.fit([(0, 0)], X, Y, chunk=64)
    b.set_fit_wide(2)
    out = b.fit([(0, 0)], X, Y, chunk=64)
    _same_outputs(out, ref)
    full = out['m'][0] == 70
    assert out['m'][0][-1] == 70 and (out['branch'][0][full] != 2)[1:].all() and (out['branch'][0][full] == 1).sum() > 5
    _same_handles(a, b)
    assert b.flagged_replicas() == dict(saturated=[0], pool_full=[])
    assert _info(b) == _expected(ref, [0], 64, 2, 0) and _info(b)[0] == 600 - 64
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- Projectron++, the classes, refusals

def test_projectron_plus_stays_narrow(golden_dir):
    """in Projectron++ mode the setting is accepted and ignored: the bytes are the narrow path's and the info is zeros"""
    from ranslice.kbrl_dev import VecKBRL
    g = _load(golden_dir, 'g9_projectron')
    X, Y = [g['d4_x'][:400]], [g['d4_y'][:400]]
    hs = []
    for _ in range(2):
        h = VecKBRL(1, [3], 200, capacity=256, pool_bytes=64 << 20, algorithm='projectron_plus')
        h.reset([[10]], [[3]])
        hs.append(h)
    a, b = hs
    ref = a.fit([(0, 0)], X, Y, chunk=50)
    b.set_fit_wide(2, 8)
    out = b.fit([(0, 0)], X, Y, chunk=50)
    _same_outputs(out, ref)
    assert (ref['branch'][0] >= 3).any() and ref['m'][0][-1] >= 2
    _same_handles(a, b)
    assert _info(b) == [0, 0, 0, 0]
    a.close()
    b.close()


def test_projectron_fit_wide_argument(golden_dir):
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import Projectron, SVvariable
    g = _load(golden_dir, 'g9_projectron')
    x, y = g['d4_x'][:300], g['d4_y'][:300]
    p, q = (Projectron(GaussianKernel(SVvariable(), 1.0)) for _ in range(2))
    yp, yq = p.fit(x, y), q.fit(x, y, wide=(2, 16))
    assert np.array_equal(yp, yq) and p.f == q.f
    assert q._agent.fit_wide == (2, 16) and p._agent.fit_wide == (0, 0)
    assert q._agent.fit_wide_info()['samples'] == 300 - 256 and p._agent.fit_wide_info()['samples'] == 0
    assert np.array_equal(_bits(p.Kinv), _bits(q.Kinv))
    q.fit(x[:3], y[:3], wide=0)
    assert q._agent.fit_wide == (0, 0)


def test_refusals_and_what_the_setting_belongs_to(golden_dir):
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    ag = VecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    ag.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    for args in ((-1, 0), (1, 0), (2, -1), (2, 257), (-5, 300)):
        with pytest.raises(_lib.RanSliceError) as e:
            ag.set_fit_wide(*args)
        assert e.value.code == _lib.RS_EINVAL, args
        assert ag.fit_wide == (0, 0)
    ag.set_fit_wide(2, 256)
    ag.set_fit_wide(320, 1)
    assert ag.fit_wide == (320, 1)
    ag.fit([(0, 0), (1, 1)], [np.full((3, 11), 0.5), np.full((2, 4), 0.5)], [[1, -1, 1], [-1, 1]])
    # host state of the handle: a checkpoint does not hold it, a handle made from this one starts with its own default
    other = VecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    other.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    other.load_state(ag.save_state())
    assert other.fit_wide == (0, 0) and ag.fit_wide == (320, 1)
    other.close()
    frozen = [ag.deploy([0, 1]), VecKBRL.load_agents(ag.export_agents([1, 0])), ag.deploy([1, 1, 0], by_reference=True)]
    for h, word in zip(frozen, ('inference-only', 'inference-only', 'by-reference')):
        assert h.fit_wide == (0, 0)
        with pytest.raises(_lib.RanSliceError) as e:
            h.set_fit_wide(64)
        assert e.value.code == _lib.RS_ESTATE and word in str(e.value)
        h.close()
    sh = SharedVecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    sh.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    assert sh.L.kb_set_fit_wide(sh.h, 64, 0) == _lib.RS_ESTATE and 'shared' in sh.L.kb_last_error(sh.h).decode()
    with pytest.raises(_lib.RanSliceError) as e:
        sh.set_fit_wide(64)
    assert e.value.code == _lib.RS_ESTATE
    sh.close()
    ag.close()
