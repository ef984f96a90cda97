"""kb_fit's chip-wide rounds in Projectron++ mode on the device (kb_set_fit_wide_plus; csrc/kb_fit_wide.hip): twin
handles in Projectron++ mode, one fitted by the one-workgroup kernel and one with kb_set_fit_wide and kb_set_fit_wide_plus on,
held to EQUAL BYTES in every returned array, in every dictionary (landmarks, coefficients, all of Kinv), in sizes, flags,
statistics and kb_fit_time_ms's counters (the checks of tests/test_gpu_fit_wide.py restated); kb_fit_wide_info equal to the
counters tests/fit_wide_plus_mirror.py derives from where the samples of branches 1-4 are.  The mat-vec count of the info --
every mistake AND every margin sample taught wide -- is what the library before this switch cannot show: its info is zeros."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_wide_plus_mirror as fwp   # noqa: E402

pytestmark = pytest.mark.gpu
PLUS = 'projectron_plus'


def _load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + '.npz'))


def _tag(golden_dir, tag):
    g = _load(golden_dir, 'g18_projectron_plus')
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + '_')}


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
        c = fwp.counters(br, m, z, chunk=chunk, min_landmarks=min_landmarks, window=window)
        tot = [u + v for u, v in zip(tot, c)]
    return tot


def _taught_wide(m_after, m0, chunk, min_landmarks):
    """mask of the samples that lie in chunks the rounds taught: those that begin with min_landmarks or more"""
    chunk = chunk or fwp.KB_FIT_CHUNK
    before = np.concatenate([[m0], np.asarray(m_after)[:-1]])
    mask = np.zeros(len(before), dtype=bool)
    for r0 in range(0, len(before), chunk):
        mask[r0:r0 + chunk] = before[r0] >= min_landmarks
    return mask


def _handle(dims, n=1, capacity=1024, algorithm=PLUS, seeds=None, pool_bytes=64 << 20):
    from ranslice.kbrl_dev import VecKBRL
    h = VecKBRL(n, dims, 200, capacity=capacity, pool_bytes=pool_bytes, algorithm=algorithm)
    h.reset(np.full((n, len(dims)), 10), np.full((n, len(dims)), 3), seeds=seeds)
    return h


def _wide(h, min_landmarks, window=0):
    h.set_fit_wide(min_landmarks, window)
    h.set_fit_wide_plus(True)
    assert h.fit_wide == (min_landmarks, window) and h.fit_wide_plus is True
    return h


def _close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.abs(a - b) > np.maximum(rtol * np.abs(b), atol)
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], a[bad][:5], b[bad][:5])


def _check_samples(out, g):
    """tests/test_gpu_projectron_plus.py's check of a fit against the recording: f 1e-8 / 1e-9, sign where |f| > 1e-9, every branch
    and size exact, delta 1e-7 / 1e-9 on the samples of branches 1-4 and 0 elsewhere"""
    _close(out['f'], g['f'], 1e-8, 1e-9, 'f')
    clear = np.abs(g['f']) > 1e-9
    assert np.array_equal(out['y_pred'][clear], g['ypred'][clear])
    assert np.array_equal(out['branch'], g['branch']), np.nonzero(out['branch'] != g['branch'])[0][:5]
    assert np.array_equal(out['m'], g['m'])
    upd = g['branch'] != 0
    _close(out['delta'][upd], g['delta'][upd], 1e-7, 1e-9, 'delta')
    assert not out['delta'][~upd].any()


# ---------------------------------------------------------------------------------------------- all of G18 rev, one learner

@pytest.fixture(scope='module')
def rev_narrow(golden_dir):
    """the narrow path's result, computed once and left alone: 2,500 samples, 1 -> 318 landmarks (five blocks, 15 tiles)"""
    g = _tag(golden_dir, 'rev')
    a = _handle([10])
    out = a.fit([(0, 0)], [g['x']], [g['y']])
    assert a.fit_wide == (0, 0) and a.fit_wide_plus is False and _info(a) == [0, 0, 0, 0]
    br, before = g['branch'], np.concatenate([[0], g['m'][:-1]])
    # what the recording holds: every branch at two landmarks or more and at 65 or more, across 64 -> 65 and 128 -> 129
    assert np.bincount(br[before >= 2], minlength=5).tolist() == [901, 71, 316, 110, 1091]
    assert np.bincount(br[before >= 65], minlength=5).tolist() == [846, 55, 253, 91, 908]
    assert g['m'][-1] == 318 and int(np.argmax(before >= 65)) == 347 and int(np.argmax(before >= 129)) == 743
    yield g, a, out
    a.close()


@pytest.mark.parametrize('min_landmarks,window,chunk', [(2, 0, 0), (2, 1, 7), (2, 3, 7), (65, 0, 0), (400, 0, 0)])
def test_rev_wide_is_the_narrow_path_bit_for_bit(rev_narrow, min_landmarks, window, chunk):
    """for the default window and chunk, for windows of 1 and 3 under chunks of 7, for a threshold of 65 and for one the dictionary
    never reaches (no rounds at all).  The info's mat-vecs are the samples of branches 1-4 among those taught wide: margin samples
    went through the rounds.  (The library without kb_set_fit_wide_plus reports zeros here.)"""
    g, a, ref = rev_narrow
    b = _wide(_handle([10]), min_landmarks, window)
    out = b.fit([(0, 0)], [g['x']], [g['y']], chunk=chunk)
    _same_outputs(out, ref)
    _same_handles(a, b)
    want = _expected(ref, [0], chunk, min_landmarks, window)
    info = _info(b)
    assert info == want
    br = ref['branch'][0]
    mask = _taught_wide(ref['m'][0], 0, chunk, min_landmarks)
    if min_landmarks == 400:
        assert not mask.any() and info == [0, 0, 0, 0]
    else:
        assert info[0] == int(mask.sum()) > 1900   # (threshold 65 under chunks of 256: from sample 512 on)
        assert info[1] == int((br[mask] != 0).sum())
        assert info[1] > int(((br[mask] == 1) | (br[mask] == 2)).sum()) > 0   # more mat-vecs than projections + insertions
        assert all((br[mask] == c).any() for c in range(5))
        assert info[2] > 5 * info[1]                                          # through many tiles
    # the wide handle against the recording itself, as tests/test_gpu_projectron_plus.py holds the narrow one for this tag
    _check_samples({k: v[0] for k, v in out.items()}, g)
    L = b.learner(0, 0, with_kinv=True)
    assert L['m'] == len(g['landmarks']) == 318
    np.testing.assert_array_equal(L['landmarks'], g['landmarks'])
    np.testing.assert_allclose(L['coeff'], g['coeff'], rtol=1e-7, atol=1e-8)
    kinv = L['kinv']
    scale = np.abs(g['kinv_rows']).max()
    np.testing.assert_allclose(kinv[::16], g['kinv_rows'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(np.diag(kinv), g['kinv_diag'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(kinv @ g['kinv_probes'], g['kinv_kp'], rtol=1e-6, atol=1e-6 * np.abs(g['kinv_kp']).max())
    assert np.array_equal(kinv, kinv.T)
    b.close()


# ---------------------------------------------------------------------------------------------- G18 d4, threshold 2

@pytest.mark.parametrize('window,chunk', [(0, 0), (3, 4)])
def test_d4_with_a_threshold_of_two(golden_dir, window, chunk):
    """18 landmarks: the rounds on small dictionaries, one block, one tile.  With chunks of 4 the rounds begin at sample 4 -- all
    1,196 samples predicted against two landmarks or more -- and sample 4 is the recording's exact f == 0 against a populated
    dictionary: a tie draw inside the rounds (sample 3, the other one, meets a single landmark and stays sequential)"""
    g = _tag(golden_dir, 'd4')
    a, b = _handle([3]), _wide(_handle([3]), 2, window)
    ref = a.fit([(0, 0)], [g['x']], [g['y']], chunk=chunk)
    out = b.fit([(0, 0)], [g['x']], [g['y']], chunk=chunk)
    _same_outputs(out, ref)
    _same_handles(a, b)
    info = _info(b)
    assert info == _expected(ref, [0], chunk, 2, window)
    br = ref['branch'][0]
    mask = _taught_wide(ref['m'][0], 0, chunk, 2)
    assert info[1] == int((br[mask] != 0).sum()) > int(((br[mask] == 1) | (br[mask] == 2)).sum())
    assert (out['f'][0][3:5] == 0.0).all() and out['m'][0][3] == 2
    if chunk == 4:
        assert info[0] == 1196 and mask[4] and not mask[3]
    _check_samples({k: v[0] for k, v in out.items()}, g)
    assert b.learner(0, 0)['m'] == 18
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- four learners in one call, ragged

@pytest.fixture(scope='module')
def ragged(golden_dir):
    """twin 3-agent handles of (d11, d4) learners in Projectron++ mode.  Agent 2's d11 learner already holds 100 landmarks (an
    earlier, narrow call on both).  Then ONE call: the first 600 samples of rev and all of d4 (agent 0), no samples (agent 1, d4),
    the next 400 samples of rev (agent 2, d11).  Threshold 65, chunks of 128: d4 stays narrow throughout, the rev prefix passes 65
    landmarks at sample 347 and changes path at the chunk boundary 384, the last learner is wide from its first chunk."""
    rev, d4 = _tag(golden_dir, 'rev'), _tag(golden_dir, 'd4')
    n_pre = int(np.nonzero(rev['m'] == 100)[0][0]) + 1
    hs = []
    for _ in range(2):
        h = _handle([10, 3], n=3, pool_bytes=256 << 20)
        h.fit([(2, 0)], [rev['x'][:n_pre]], [rev['y'][:n_pre]])
        hs.append(h)
    a, b = hs
    assert a.dictionary_sizes()[2, 0] == 100 and _info(b) == [0, 0, 0, 0]
    learners = [(0, 0), (0, 1), (1, 1), (2, 0)]
    X = [rev['x'][:600], d4['x'], d4['x'][:0], rev['x'][n_pre:n_pre + 400]]
    Y = [rev['y'][:600], d4['y'], d4['y'][:0], rev['y'][n_pre:n_pre + 400]]
    ref = a.fit(learners, X, Y, chunk=128)
    _wide(b, 65)
    out = b.fit(learners, X, Y, chunk=128)
    yield a, b, ref, out, X
    a.close()
    b.close()


def test_four_ragged_learners_narrow_and_wide_in_one_call(ragged):
    a, b, ref, out, X = ragged
    _same_outputs(out, ref)
    _same_handles(a, b)
    m0 = [0, 0, 0, 100]
    assert _info(b) == _expected(ref, m0, 128, 65, 0)
    per = [fwp.counters(br, m, z, chunk=128, min_landmarks=65) for br, m, z in zip(ref['branch'], ref['m'], m0)]
    assert per[0][0] == 600 - 384 and per[1] == [0, 0, 0, 0] and per[2] == [0, 0, 0, 0] and per[3][0] == 400
    for i in (0, 3):   # margin samples went through the rounds on both wide learners
        br = ref['branch'][i][_taught_wide(ref['m'][i], m0[i], 128, 65)]
        assert per[i][1] == int((br != 0).sum()) > int(((br == 1) | (br == 2)).sum())


def test_after_a_wide_fit(ragged):
    """the cache of the last predict is gone on the learners that were taught (kb_update answers RS_ESTATE until a new kb_predict),
    and select_action on the same state takes the same actions on both handles"""
    from ranslice import _lib
    a, b, _, _, X = ragged
    for h in (a, b):
        for (e, s), x in (((0, 0), X[0][0]), ((2, 0), X[3][0])):
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
    """tests/test_gpu_fit_wide.py's construction in Projectron++ mode: samples 1e3 and more away from a populated dictionary, every
    kernel value underflows, f == 0.0 exactly, the margin is 0 -- a mistake whose y_pred is a draw of the learner's tie stream: the
    same draws as the narrow path, and the streams stand at the same position afterwards"""
    g = _load(golden_dir, 'g9_projectron')
    far = np.array([[1e3 * (i + 2)] * 4 for i in range(10)])
    X = [np.concatenate([g['d4_x'][:30], far, g['d4_x'][30:40]])]
    Y = [np.concatenate([g['d4_y'][:30], np.array([1, -1] * 5, dtype=np.int8), g['d4_y'][30:40]])]
    seeds = np.array([0x1234567887654321], dtype=np.uint64)
    a, b = (_handle([3], capacity=256, seeds=seeds) for _ in range(2))
    ref = a.fit([(0, 0)], X, Y, chunk=4)
    _wide(b, 2, 3)
    out = b.fit([(0, 0)], X, Y, chunk=4)
    _same_outputs(out, ref)
    assert (out['f'][0][30:40] == 0.0).all() and out['m'][0][29] >= 2
    assert set(out['y_pred'][0][30:40].tolist()) == {1, -1} and (out['branch'][0][30:40] == 2).all()
    assert (out['branch'][0] >= 3).any()
    _same_handles(a, b)
    want = _expected(ref, [0], 4, 2, 3)
    assert _info(b) == want and want[1] >= 10
    later = np.array([7e4] * 4)
    draws = [(a.predict(0, 0, later), b.predict(0, 0, later)) for _ in range(6)]
    assert all(u == v and u[1] == 0.0 and u[0] in (1, -1) for u, v in draws)
    a.close()
    b.close()


def test_saturation_at_a_capacity_of_70(golden_dir):
    """the dictionary fills up inside the wide path: the flag bits, branch 1 from then on and the sizes are the narrow path's, and
    the margin rule goes on against the full dictionary (it asks for no capacity): samples of branches 3 / 4 after the fill"""
    g = _load(golden_dir, 'g9_projectron')
    X, Y = [g['d11_x'][:600]], [g['d11_y'][:600]]
    a, b = (_handle([10], capacity=70) for _ in range(2))
    ref = a.fit([(0, 0)], X, Y, chunk=64)
    _wide(b, 2)
    out = b.fit([(0, 0)], X, Y, chunk=64)
    _same_outputs(out, ref)
    full = out['m'][0] == 70
    br = out['branch'][0]
    assert out['m'][0][-1] == 70 and (br[full] != 2)[1:].all() and (br[full] == 1).sum() > 5
    assert (br[full] >= 3).sum() > 5
    _same_handles(a, b)
    assert b.flagged_replicas() == dict(saturated=[0], pool_full=[])
    assert _info(b) == _expected(ref, [0], 64, 2, 0) and _info(b)[0] == 600 - 64
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- the switch

def test_off_by_default_projectron_plus_stays_narrow(golden_dir):
    """kb_set_fit_wide alone, in Projectron++ mode: the info is zeros, as before the switch existed; turned on and off again: too"""
    g = _tag(golden_dir, 'd4')
    X, Y = [g['x'][:400]], [g['y'][:400]]
    a, b = _handle([3]), _handle([3])
    ref = a.fit([(0, 0)], X, Y, chunk=50)
    b.set_fit_wide(2, 8)
    assert b.fit_wide_plus is False
    b.set_fit_wide_plus(True)
    b.set_fit_wide_plus(False)
    assert b.fit_wide_plus is False
    out = b.fit([(0, 0)], X, Y, chunk=50)
    _same_outputs(out, ref)
    _same_handles(a, b)
    assert _info(b) == [0, 0, 0, 0]
    # and the switch alone, without kb_set_fit_wide, teaches nothing wide either
    c = _handle([3])
    c.set_fit_wide_plus(True)
    _same_outputs(c.fit([(0, 0)], X, Y, chunk=50), ref)
    assert _info(c) == [0, 0, 0, 0]
    for h in (a, b, c):
        h.close()


def test_no_effect_in_projectron_mode(golden_dir):
    """in Projectron mode the switch changes nothing against kb_set_fit_wide alone: equal bytes and equal info"""
    g = _load(golden_dir, 'g9_projectron')
    X, Y = [g['d4_x'][:400]], [g['d4_y'][:400]]
    a, b = (_handle([3], algorithm='projectron') for _ in range(2))
    a.set_fit_wide(2, 8)
    _wide(b, 2, 8)
    ref = a.fit([(0, 0)], X, Y, chunk=50)
    out = b.fit([(0, 0)], X, Y, chunk=50)
    _same_outputs(out, ref)
    _same_handles(a, b)
    assert ref['branch'][0].max() <= 2
    assert _info(a) == _info(b) and _info(b)[0] == 350 and _info(b)[1] == int((ref['branch'][0][50:] != 0).sum())
    a.close()
    b.close()


def test_projectron_plus_object_hands_its_attribute_over(golden_dir):
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import ProjectronPlus, SVvariable
    g = _tag(golden_dir, 'd4')
    x, y = g['x'][:300], g['y'][:300]
    p, q = (ProjectronPlus(GaussianKernel(SVvariable(), 1.0)) for _ in range(2))
    q.wide_plus = True
    yp, yq = p.fit(x, y, wide=(2, 16)), q.fit(x, y, wide=(2, 16))
    assert np.array_equal(yp, yq) and p.f == q.f
    assert p._agent.fit_wide == q._agent.fit_wide == (2, 16)
    assert p._agent.fit_wide_plus is False and q._agent.fit_wide_plus is True
    assert p._agent.fit_wide_info()['samples'] == 0 and q._agent.fit_wide_info()['samples'] == 300 - 256
    assert np.array_equal(_bits(p.Kinv), _bits(q.Kinv))
    q.wide_plus = False
    q.fit(x[:3], y[:3])
    assert q._agent.fit_wide_plus is False


def test_refusals_and_what_the_switch_belongs_to():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    ag = _handle([10, 3], n=2, capacity=128)
    for bad in (2, -1, 7):
        with pytest.raises(_lib.RanSliceError) as e:
            ag.set_fit_wide_plus(bad)
        assert e.value.code == _lib.RS_EINVAL, bad
        assert ag.fit_wide_plus is False
    ag.set_fit_wide(2)
    ag.set_fit_wide_plus()
    assert ag.fit_wide_plus is True
    ag.fit([(0, 0), (1, 1)], [np.full((3, 11), 0.5), np.full((2, 4), 0.5)], [[1, -1, 1], [-1, 1]])
    # host state of the handle: a checkpoint does not hold it, a handle made from this one starts with its own default
    other = _handle([10, 3], n=2, capacity=128)
    other.load_state(ag.save_state())
    assert other.fit_wide_plus is False and ag.fit_wide_plus is True
    other.close()
    forked = _handle([10, 3], n=3, capacity=128)
    forked.fork_from(ag, [1, 0, 1])
    assert forked.fit_wide_plus is False and forked.fit_wide == (0, 0) and ag.fit_wide_plus is True
    forked.close()
    frozen = [ag.deploy([0, 1]), VecKBRL.load_agents(ag.export_agents([1, 0])), ag.deploy([1, 1, 0], by_reference=True)]
    for h, word in zip(frozen, ('inference-only', 'inference-only', 'by-reference')):
        assert h.fit_wide_plus is False
        with pytest.raises(_lib.RanSliceError) as e:
            h.set_fit_wide_plus(True)
        assert e.value.code == _lib.RS_ESTATE and word in str(e.value)
        h.close()
    sh = SharedVecKBRL(2, [10, 3], 50, capacity=128, pool_bytes=64 << 20)
    sh.reset(np.full((2, 2), 10), np.full((2, 2), 2))
    assert sh.L.kb_set_fit_wide_plus(sh.h, 1) == _lib.RS_ESTATE and 'shared' in sh.L.kb_last_error(sh.h).decode()
    with pytest.raises(_lib.RanSliceError) as e:
        sh.set_fit_wide_plus(True)
    assert e.value.code == _lib.RS_ESTATE
    sh.close()
    ag.close()
