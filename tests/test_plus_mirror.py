"""The Projectron++ rule without a GPU: the float64 restatement tests/plus_mirror.py replays both tags of the reference's
recording G18 (tests/golden/g18_projectron_plus.npz; tools/gen_golden_plus.py) and must take every decision the reference took:
each sample's branch (0 nothing, 1 projection, 2 insertion, 3 margin update, 4 margin test without update) and dictionary size
exactly, f / delta / slack and the final dictionary to the tolerances tests/test_gpu_kbrl.py::test_projectron_teacher_forced
applies to G9 (f 1e-8 relative / 1e-9 absolute, delta 1e-7 / 1e-9, coefficients and Kinv 1e-8).  This pins the recording and the
prose of the rule (the float32 roundings while one landmark is held included) to each other.

Measured: the mirror reproduces the recording with deviation 0 in every one of these quantities (it forms the reference's NumPy
expressions in the reference's order), so the reference's rounding-order floor against this restatement is zero and the G9
tolerances stand as they are for the device tests.

The recording's own quality (asserted here as the generator asserts it): at least 100 margin updates per tag, a margin test
while a single landmark is held in d4, every decision at least 1e-6 from its threshold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plus_mirror as pm   # noqa: E402

ETA = 0.1
TOL = 1e-9


def _tag(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, 'g18_projectron_plus.npz'))
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + '_')}


def _close(a, b, rtol, atol, what):
    bad = np.abs(a - b) > np.maximum(rtol * np.abs(b), atol)
    print('%s: max |dev| %.3g' % (what, np.abs(a - b).max() if len(a) else 0.0))
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], a[bad][:5], b[bad][:5])


@pytest.fixture(scope='module', params=['d4', 'rev'])
def replayed(request, golden_dir):
    g = _tag(golden_dir, request.param)
    after = []
    mir, out = pm.replay(g['x'], g['y'], g['ties'], eta=ETA,
                         on_sample=lambda i, m, b: after.append(m.c.copy()) if b == 3 else None)
    return request.param, g, mir, out, after


def test_recording_conditions(replayed):
    tag, g, _, _, _ = replayed
    br, m = g['branch'], g['m']
    assert (br == 3).sum() >= 100
    margin, mistake = br >= 3, (br == 1) | (br == 2)
    assert np.abs(g['slack'][margin]).min() > 1e-6
    assert np.abs(g['delta'][mistake] - ETA).min() > 1e-6
    assert np.isnan(g['delta'][br == 0]).all() and np.isnan(g['slack'][~margin]).all()
    assert not np.isnan(g['delta'][br != 0]).any() and not np.isnan(g['slack'][margin]).any()
    assert np.array_equal((br == 3), margin & (g['slack'] > 0))
    assert np.array_equal(np.diff(np.concatenate([[0], m])) == 1, br == 2)   # only an insertion grows the dictionary
    if tag == 'd4':
        m_before = np.concatenate([[0], m[:-1]])
        assert (margin & (m_before == 1)).sum() >= 1      # the float32 regime meets the margin rule
        assert m[-1] == 18 and g['coeff_after'].shape == ((br == 3).sum(), 18) and g['kinv'].shape == (18, 18)
    else:
        assert m[-1] == 318 and m.max() > 256 and (m == 65).any()


def test_mirror_takes_every_decision_of_the_reference(replayed):
    tag, g, mir, out, _ = replayed
    assert np.array_equal(out['branch'], g['branch'])
    assert np.array_equal(out['m'], g['m'])
    _close(out['f'], g['f'], 1e-8, TOL, tag + ' f')
    clear = np.abs(g['f']) > TOL
    assert np.array_equal(out['ypred'][clear], g['ypred'][clear])
    upd = g['branch'] != 0
    _close(out['delta'][upd], g['delta'][upd], 1e-7, 1e-9, tag + ' delta')
    margin = g['branch'] >= 3
    _close(out['slack'][margin], g['slack'][margin], 1e-7 / ETA, 1e-9 / ETA, tag + ' slack')   # slack carries delta / eta
    assert np.isnan(out['delta'][~upd]).all() and np.isnan(out['slack'][~margin]).all()


def test_mirror_ends_with_the_reference_dictionary(replayed):
    tag, g, mir, out, after = replayed
    assert np.array_equal(mir.L, np.atleast_2d(g['landmarks']))
    _close(mir.c, g['coeff'], 1e-8, 1e-9, tag + ' coeff')
    if tag == 'd4':
        kinv = g['kinv']
        _close(mir.P.ravel(), kinv.ravel(), 1e-8, 1e-8 * np.abs(kinv).max(), 'd4 kinv')
        assert len(after) == len(g['coeff_after'])
        for c, r in zip(after, g['coeff_after']):
            assert not r[len(c):].any()
            np.testing.assert_allclose(c, r[:len(c)], rtol=1e-8, atol=1e-9)
    else:   # G14's digest and tolerances (tests/test_gpu_kbrl.py: 1e-6 of the scale)
        scale = np.abs(g['kinv_rows']).max()
        _close(mir.P[::16].ravel(), g['kinv_rows'].ravel(), 1e-6, 1e-6 * scale, 'rev kinv rows')
        _close(np.diag(mir.P), g['kinv_diag'], 1e-6, 1e-6 * scale, 'rev kinv diagonal')
        kp = g['kinv_kp']
        _close((mir.P @ g['kinv_probes']).ravel(), kp.ravel(), 1e-6, 1e-6 * np.abs(kp).max(), 'rev kinv probes')


def test_projectron_mode_of_the_mirror_is_g9(golden_dir):
    """with the margin rule off the same restatement replays G9's d4 recording of Projectron: the two rules share everything else"""
    g = np.load(os.path.join(golden_dir, 'g9_projectron.npz'))
    mir, out = pm.replay(g['d4_x'], g['d4_y'], g['d4_ties'], plus=False, eta=ETA)
    assert np.array_equal(out['branch'], g['d4_branch']) and np.array_equal(out['m'], g['d4_m'])
    _close(out['f'], g['d4_f'], 1e-8, TOL, 'g9 d4 f')
    _close(mir.c, g['d4_coeff'], 1e-8, 1e-9, 'g9 d4 coeff')
