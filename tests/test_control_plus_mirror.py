"""The closed control loop in Projectron++ mode without a GPU: tests/control_plus_mirror.py (update_control, select_action and
adjust_action restated in NumPy over tests/plus_mirror.py's learners) replays the reference's recording G19
(tests/golden/g19_control_plus.npz; tools/gen_golden_control_plus.py) teacher-forced and must take every decision the reference
took: hits, selected actions, adjusted, margins, security factors and sizes at every step, the branch of every sample of the
augmentation (0 nothing, 1 projection, 2 insertion, 3 margin update, 4 margin test without update) exactly; f at the executed
allocation, the accuracy tables and the final dictionaries to the tolerances tests/test_plus_mirror.py applies to G9 / G18 (f
1e-8 relative / 1e-9 absolute, coefficients and Kinv 1e-8).  This pins the recording and the prose of the mode
to each other.

The recording's own quality (asserted here as far as the fixture holds the figures): no tie draw, every branch of the rule
present, the first 40 steps take the dictionaries through the float32 regime of one landmark, later steps one past a shell."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_plus_mirror as cm   # noqa: E402


def _close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    bad = np.abs(a - b) > np.maximum(rtol * np.abs(b), atol)
    print('%s: max |dev| %.3g' % (what, np.abs(a - b).max() if len(a) else 0.0))
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], a[bad][:5], b[bad][:5])


@pytest.fixture(scope='module')
def replayed(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g19_control_plus.npz'))
    dims, n_prbs = [10] * 5, 200
    draws = iter(g['ties'])
    mir = cm.ControlMirror(dims, n_prbs, g['init_action'], g['init_sec'], accuracy_range=tuple(g['a_range']), tie=lambda: next(draws))
    steps = len(g['state'])
    nxt = np.concatenate([g['state'][1:], g['final_state'][None]])
    rec = dict(hits=[], action_out=[], adjusted=[], margins=[], security=[], set_size=[])
    for i in range(steps):
        rec['hits'].append(mir.update_control(g['state'][i], g['action_in'][i], g['labels'][i]))
        act, adj = mir.select_action(nxt[i])
        rec['action_out'].append(act)
        rec['adjusted'].append(adj)
        rec['margins'].append(mir.margins.copy())
        rec['security'].append(mir.security.copy())
        rec['set_size'].append([h.m for h in mir.learners])
    return g, mir, {k: np.asarray(v) for k, v in rec.items()}


def test_recording_conditions(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g19_control_plus.npz'))
    assert g['state'].shape == (300, 50) and int(g['scenario']) == 0 and len(g['ties']) == 0
    counts = np.where(g['labels'] == 1, 200 - g['action_in'].astype(np.int64) + 1, g['action_in'].astype(np.int64) + 1)
    br = [g['branch%d' % s] for s in range(5)]
    assert [len(b) for b in br] == counts.sum(axis=0).tolist()
    assert (np.bincount(np.concatenate(br), minlength=5) > 0).all() and np.concatenate(br).max() == 4
    for s in range(5):   # only an insertion grows a dictionary
        assert int((br[s] == 2).sum()) == g['set_size'][-1, s] == len(g['coeff%d' % s]) == len(g['kinv%d' % s])
    m = np.concatenate([np.zeros((1, 5), dtype=np.int64), g['set_size'].astype(np.int64)])
    assert ((m[:41][:-1] <= 1) & (m[:41][1:] >= 1)).any()            # the first 40 steps: the float32 regime of one landmark
    assert ((m[:-1] <= 64) & (m[1:] >= 65)).any() and m[-1].max() >= 66   # later: past one shell
    assert g['f0'].shape == (300, 5) and (g['f0'][0] == 0.0).all() and (g['f0'][1:] != 0.0).any()


def test_mirror_takes_every_decision_of_the_reference(replayed):
    g, mir, rec = replayed
    for k in ('hits', 'action_out', 'adjusted', 'margins', 'security', 'set_size'):
        same = (rec[k] == g[k]).reshape(len(rec[k]), -1).all(axis=1)
        assert same.all(), (k, 'first at step', int(np.nonzero(~same)[0][0]))
    for s in range(5):
        got = np.asarray(mir.branches[s], dtype=np.int8)
        assert np.array_equal(got, g['branch%d' % s]), (s, np.nonzero(got != g['branch%d' % s])[0][:5])


def test_mirror_values(replayed):
    g, mir, rec = replayed
    _close(np.asarray(mir.f0), g['f0'], 1e-8, 1e-9, 'f at the executed allocation')
    _close(mir.accuracies, g['acc'], 1e-12, 0.0, 'accuracy tables')
    for s, h in enumerate(mir.learners):
        assert np.array_equal(h.L, np.atleast_2d(g['landmarks%d' % s]))
        _close(h.c, g['coeff%d' % s], 1e-8, 1e-9, 'coeff %d' % s)
        kinv = g['kinv%d' % s]
        _close(h.P, kinv, 1e-8, 1e-8 * np.abs(kinv).max(), 'kinv %d' % s)
