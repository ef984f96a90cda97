"""Projectron++ on the device (kb_set_algorithm) against the reference's recording G18
(tests/golden/g18_projectron_plus.npz: ProjectronPlus of projectron.py:66-107 on G9's d4 stream and on G14's revisit stream cut
to 2,500 samples).  Every branch (0 nothing, 1 projection, 2 insertion, 3 margin update, 4 margin test without update) and
dictionary size is held exactly; values carry the tolerances tests/test_gpu_kbrl.py::test_projectron_teacher_forced applies to
G9 -- f 1e-8 relative / 1e-9 absolute, delta 1e-7 / 1e-9, coefficients and Kinv 1e-8 -- and, for the 318-landmark stream, G14's
(coefficients 1e-7, the Kinv digest 1e-6 of its scale).  The float64 mirror of the rule (tests/test_plus_mirror.py) reproduces
the recording with deviation 0, so the reference leaves no rounding-order floor to add to them."""
import os

import numpy as np
import pytest

from ranslice.config import make_config

pytestmark = pytest.mark.gpu
TOL = 1e-9


def _tag(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, 'g18_projectron_plus.npz'))
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + '_')}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b, what=''):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(_bits(a), _bits(b)), what


def _close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.abs(a - b) > np.maximum(rtol * np.abs(b), atol)
    print('%s: max |dev| %.3g' % (what, np.abs(a - b).max() if a.size else 0.0))
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], a[bad][:5], b[bad][:5])


def _agent(d, algorithm='projectron_plus', n=1):
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(n, [d - 1], 200, capacity=1024, pool_bytes=64 << 20, algorithm=algorithm)
    ag.reset(np.full((n, 1), 10), np.full((n, 1), 3))
    return ag


def _one_by_one(ag, x, y, after=None):
    """kb_predict, kb_update per sample on learner (0, 0) -> dict of arrays; after: list that takes the coefficients after every
    margin update"""
    n = len(x)
    out = dict(y_pred=np.zeros(n, dtype=np.int32), f=np.zeros(n), branch=np.zeros(n, dtype=np.int32), delta=np.zeros(n),
               m=np.zeros(n, dtype=np.int32))
    for t in range(n):
        out['y_pred'][t], out['f'][t] = ag.predict(0, 0, x[t])
        out['branch'][t], out['delta'][t] = ag.update(0, 0, x[t], int(y[t]))
        out['m'][t] = ag.dictionary_sizes()[0, 0]
        if after is not None and out['branch'][t] == 3:
            after.append(ag.learner(0, 0)['coeff'])
    return out


def _check_samples(out, g):
    """f, sign (where |f| > 1e-9), branch, size, delta of every sample against the recording"""
    _close(out['f'], g['f'], 1e-8, TOL, 'f')
    clear = np.abs(g['f']) > TOL
    assert np.array_equal(out['y_pred'][clear], g['ypred'][clear])
    assert np.array_equal(out['branch'], g['branch']), np.nonzero(out['branch'] != g['branch'])[0][:5]
    assert np.array_equal(out['m'], g['m'])
    upd = g['branch'] != 0
    _close(out['delta'][upd], g['delta'][upd], 1e-7, 1e-9, 'delta')
    assert not out['delta'][~upd].any()


def _counts(g):
    br = g['branch']
    return len(br), int(((br >= 1) & (br <= 3)).sum()), int((br == 2).sum())


# ---------------------------------------------------------------------------------------------- d4, sample by sample

@pytest.fixture(scope='module')
def d4(golden_dir):
    """G18's d4 stream through kb_predict / kb_update in Projectron++ mode, all 1,200 samples; what the tests need is taken here,
    so that none of them depends on what another does to the handle"""
    g = _tag(golden_dir, 'd4')
    ag = _agent(4)
    assert ag.algorithm == 'projectron_plus'
    after = []
    out = _one_by_one(ag, g['x'], g['y'], after)
    rec = dict(out=out, after=after, final=ag.learner(0, 0, with_kinv=True), stats=ag.stats())
    yield ag, g, rec
    ag.close()


def test_d4_sample_by_sample(d4):
    """every f, sign, branch, delta and size; the coefficient vector after each of the 147 margin updates; the final dictionary"""
    _, g, rec = d4
    _check_samples(rec['out'], g)
    assert len(rec['after']) == len(g['coeff_after']) == 147
    for i, (c, r) in enumerate(zip(rec['after'], g['coeff_after'])):
        assert not r[len(c):].any(), i
        np.testing.assert_allclose(c, r[:len(c)], rtol=1e-8, atol=1e-9, err_msg='margin update %d' % i)
    L = rec['final']
    assert L['m'] == len(g['landmarks']) == 18
    np.testing.assert_array_equal(L['landmarks'], g['landmarks'])
    np.testing.assert_allclose(L['coeff'], g['coeff'], rtol=1e-8, atol=1e-9)
    np.testing.assert_allclose(L['kinv'], g['kinv'], rtol=1e-8, atol=1e-8 * np.abs(g['kinv']).max())
    # (the stream holds margin tests while a single landmark is held: the float32 regime of loss and slack)
    m_before = np.concatenate([[0], g['m'][:-1]])
    assert ((g['branch'] >= 3) & (m_before == 1)).any()


def test_statistics_one_by_one(d4):
    """a mistake of the per-learner statistics is a sample that changed the dictionary: branches 1-3"""
    _, g, rec = d4
    n, mistakes, grown = _counts(g)
    assert rec['stats'][:3] == [n, mistakes, grown]


# ---------------------------------------------------------------------------------------------- rev, one kb_fit

@pytest.fixture(scope='module')
def rev(golden_dir):
    g = _tag(golden_dir, 'rev')
    ag = _agent(11)
    out = ag.fit([(0, 0)], [g['x']], [g['y']])
    rec = dict(out={k: v[0] for k, v in out.items()}, final=ag.learner(0, 0, with_kinv=True), stats=ag.stats(), work=ag.fit_time_ms())
    yield ag, g, rec
    ag.close()


def test_rev_in_one_fit_call(rev):
    """2,500 samples to 318 landmarks (past the second shell at 65 and past 256) in ONE kb_fit, default chunk"""
    _, g, rec = rev
    _check_samples(rec['out'], g)
    L = rec['final']
    assert L['m'] == len(g['landmarks']) == 318
    np.testing.assert_array_equal(L['landmarks'], g['landmarks'])
    np.testing.assert_allclose(L['coeff'], g['coeff'], rtol=1e-7, atol=1e-8)
    kinv = L['kinv']
    scale = np.abs(g['kinv_rows']).max()
    np.testing.assert_allclose(kinv[::16], g['kinv_rows'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(np.diag(kinv), g['kinv_diag'], rtol=1e-6, atol=1e-6 * scale)
    np.testing.assert_allclose(kinv @ g['kinv_probes'], g['kinv_kp'], rtol=1e-6, atol=1e-6 * np.abs(g['kinv_kp']).max())
    assert np.array_equal(kinv, kinv.T)


def test_statistics_of_a_fit(rev):
    _, g, rec = rev
    n, mistakes, grown = _counts(g)
    assert rec['stats'][:3] == [n, mistakes, grown]
    w = rec['work']
    assert (w['samples'], w['mistakes'], w['insertions']) == (n, mistakes, grown)
    assert w['kernel_evals'] == int(np.concatenate([[0], g['m'][:-1]]).sum())   # landmarks held when each sample arrived


# ---------------------------------------------------------------------------------------------- fit == one by one, bit for bit

@pytest.fixture(scope='module')
def rev_prefix(golden_dir):
    """the prefix of rev that ends just after the dictionary passes 65 landmarks, one by one in Projectron++ mode"""
    g = _tag(golden_dir, 'rev')
    n = int(np.argmax(g['m'] > 65)) + 1
    assert g['m'][n - 1] == 66 and ((g['branch'][:n] == 3).sum() > 0) and ((g['branch'][:n] == 4).sum() > 0)
    a = _agent(11)
    ref = _one_by_one(a, g['x'][:n], g['y'][:n])
    rec = dict(ref=ref, final=a.learner(0, 0, with_kinv=True), stats=a.stats())
    yield g, n, rec
    a.close()


@pytest.mark.parametrize('chunk', [0, 7])
def test_fit_equals_one_by_one_bit_for_bit(rev_prefix, chunk):
    """the claim test_gpu_fit.py makes for Projectron: f and delta bit for bit, the dictionaries equal as bytes (landmarks,
    coefficients, all of Kinv), whatever the chunk"""
    g, n, rec = rev_prefix
    b = _agent(11)
    out = b.fit([(0, 0)], [g['x'][:n]], [g['y'][:n]], chunk=chunk)
    ref = rec['ref']
    for k in ('y_pred', 'branch', 'm'):
        assert np.array_equal(out[k][0], ref[k]), k
    for k in ('f', 'delta'):
        _same_bits(out[k][0], ref[k], k)
    L = b.learner(0, 0, with_kinv=True)
    assert L['m'] == rec['final']['m'] == 66
    for k in ('landmarks', 'coeff', 'kinv'):
        _same_bits(L[k], rec['final'][k], k)
    assert b.stats()[:3] == rec['stats'][:3]
    b.close()


# ---------------------------------------------------------------------------------------------- the default mode is unmoved

@pytest.mark.parametrize('path', ['one_by_one', 'fit'])
def test_projectron_mode_unmoved_by_a_switch(golden_dir, path):
    """a handle switched to Projectron++ and back, then taught the first 300 samples of G9's d4 stream, equals a fresh handle bit
    for bit (the algorithm is host state: nothing of it stays behind), and takes no margin branch"""
    g = np.load(os.path.join(golden_dir, 'g9_projectron.npz'))
    x, y = g['d4_x'][:300], g['d4_y'][:300]
    res = []
    for switched in (True, False):
        ag = _agent(4, algorithm='projectron')
        if switched:
            ag.set_algorithm('projectron_plus')
            assert ag.algorithm == 'projectron_plus'
            ag.set_algorithm('projectron')
        assert ag.algorithm == 'projectron'
        out = _one_by_one(ag, x, y) if path == 'one_by_one' else {k: v[0] for k, v in ag.fit([(0, 0)], [x], [y]).items()}
        res.append((out, ag.learner(0, 0, with_kinv=True), ag.stats()))
        ag.close()
    (oa, la, sa), (ob, lb, sb) = res
    assert np.array_equal(oa['branch'], g['d4_branch'][:300]) and oa['branch'].max() <= 2
    for k in ('y_pred', 'branch', 'm'):
        assert np.array_equal(oa[k], ob[k]), k
    for k in ('f', 'delta'):
        _same_bits(oa[k], ob[k], k)
    for k in ('landmarks', 'coeff', 'kinv'):
        _same_bits(la[k], lb[k], k)
    assert sa == sb


# ---------------------------------------------------------------------------------------------- downstream of a trained learner

def test_downstream_of_a_projectron_plus_learner(d4):
    """what follows training only needs landmarks, coefficients and Kinv: kb_score equals kb_predict's f bit for bit, on the
    handle and on its deployment; select_action works; update_control is refused while in Projectron++ mode and accepted after
    set_algorithm('projectron')"""
    from ranslice import _lib
    ag, g, _ = d4
    q = g['x'][::19][:64]
    assert len(q) == 64
    f_pred = np.array([ag.predict(0, 0, p)[1] for p in q])
    f, _ = ag.score([(0, 0)], [q])
    _same_bits(f[0], f_pred, 'score on the learning handle')
    dep = ag.deploy([0])
    f2, _ = dep.score([(0, 0)], [q])
    _same_bits(f2[0], f_pred, 'score on the deployment')
    with pytest.raises(_lib.RanSliceError) as e:   # the algorithm did not travel, and a deployment takes none
        dep.set_algorithm('projectron_plus')
    assert e.value.code == _lib.RS_ESTATE and dep.algorithm == 'projectron'
    dep.close()
    state = q[:1, :3].astype(np.float32)
    action, _ = ag.select_action(state)
    assert 0 <= action[0, 0] <= 200
    sizes = ag.dictionary_sizes().copy()
    with pytest.raises(_lib.RanSliceError) as e:
        ag.update_control(state, action, [[1]])
    assert e.value.code == _lib.RS_ESTATE and 'Projectron++' in str(e.value)
    assert np.array_equal(ag.dictionary_sizes(), sizes)
    ag.set_algorithm('projectron')
    hits = ag.update_control(state, action, [[1]])
    assert hits.shape == (1, 1)
    with pytest.raises(_lib.RanSliceError) as e:
        ag._check(ag.L.kb_set_algorithm(ag.h, 2))
    assert e.value.code == _lib.RS_EINVAL and ag.algorithm == 'projectron'


def test_resident_loop_in_projectron_plus_mode():
    """kb_step_resident / kb_run_resident with learning on answer RS_ESTATE; with set_learning(False) the loop selects as before;
    back in Projectron mode it learns again"""
    from ranslice import _lib
    from ranslice.fading import synth_fading
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice
    n = 4
    cfg = make_config(1, n_envs=n)
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=[synth_fading(t, 512) for t in range(3)], seed=5)
    ag = VecKBRL(n, dims, cfg.n_prbs, capacity=256, pool_bytes=64 << 20, algorithm='projectron_plus')
    ia = np.full((n, len(dims)), 10, dtype=np.int32)
    env.reset()
    ag.reset(ia, np.full((n, len(dims)), 3))
    env.step(ia)
    for call in (lambda: ag.step_resident(env), lambda: ag.run_resident(env, 3, graph=False), lambda: ag.run_resident(env, 4, graph=True)):
        with pytest.raises(_lib.RanSliceError) as e:
            call()
        assert e.value.code == _lib.RS_ESTATE and 'Projectron++' in str(e.value)
    assert ag.stats()[0] == 0 and ag.dictionary_sizes().sum() == 0
    ag.set_learning(False)
    ag.run_resident(env, 3, graph=False)
    ag.set_learning(True)
    ag.set_algorithm('projectron')
    ag.run_resident(env, 3, graph=False)
    ag.synchronize()
    ag.close()
    env.close()
