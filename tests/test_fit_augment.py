"""ranslice.kbrl_dev.augmented_samples (host, numpy) against the oracle and the reference's recording G10: the per-learner sample
lists it makes of a control log ARE the samples update_control's augmentation loop teaches (kbrl_control.py:103-112), in order."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from ranslice.config import make_config
from ranslice.kbrl_dev import augmented_samples


def _g10(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g10_kbrl_s0.npz'))
    cfg = make_config(0)
    return g, [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs


def test_augmented_log_teaches_what_update_control_teaches(golden_dir):
    """two oracle agents on G10's 120 recorded steps of 5 learners: one through update_control, one through predict / update on
    augmented_samples of the same log.  The oracle's update_control IS that loop, so sizes, landmarks, coefficients and Kinv are
    IDENTICAL; and the landmarks are the reference's recorded ones exactly, its coefficients within 1e-8."""
    g, dims, n_prbs = _g10(golden_dir)
    cap = 1024   # no dictionary fills (asserted below): the oracle's build-defined stop at a full dictionary never acts
    a = po.OracleKBRL(dims, n_prbs, g['init_action'], g['init_sec'], accuracy_range=tuple(g['a_range']), capacity=cap)
    b = po.OracleKBRL(dims, n_prbs, g['init_action'], g['init_sec'], accuracy_range=tuple(g['a_range']), capacity=cap)
    a.set_seed(0)
    b.set_seed(0)
    steps = len(g['state'])
    assert steps == 120 and len(dims) == 5
    for i in range(steps):
        a.update_control(g['state'][i], g['action_in'][i], g['labels'][i])
    X, Y = augmented_samples(g['state'], g['action_in'], g['labels'], dims, n_prbs)
    for s in range(len(dims)):
        assert X[s].shape == (len(Y[s]), dims[s] + 1) and X[s].dtype == np.float64 and Y[s].dtype == np.int8
        for x, y in zip(X[s], Y[s]):
            b.predict(s, x)
            b.update(s, x, int(y))
    for s in range(len(dims)):
        assert 0 < a.m(s) == b.m(s) < cap
        np.testing.assert_array_equal(a.landmarks(s), b.landmarks(s))
        np.testing.assert_array_equal(a.coeff(s), b.coeff(s))
        np.testing.assert_array_equal(a.kinv(s), b.kinv(s))
        np.testing.assert_array_equal(b.landmarks(s), np.atleast_2d(g['landmarks%d' % s]))
        np.testing.assert_allclose(b.coeff(s), g['coeff%d' % s], rtol=1e-8, atol=1e-9)
    assert a.error() == 0 and b.error() == 0


def test_shape_and_order_of_hand_made_steps():
    dims, n = [10, 3], 6
    state = np.arange(3 * 13, dtype=np.float32).reshape(3, 13) / 7   # float32 observations, widened exactly
    action = np.array([[2, 0], [6, 6], [0, 3]])
    labels = np.array([[1, -1], [-1, 1], [1, -1]])
    X, Y = augmented_samples(state, action, labels, dims, n)
    assert len(X) == len(Y) == 2
    # learner 0 (dims 10): +1 from 2 -> 2..6, -1 at n_prbs -> 0..6, +1 at 0 -> 0..6
    want_a0 = [2, 3, 4, 5, 6] + list(range(7)) + list(range(7))
    want_y0 = [1] * 5 + [-1] * 7 + [1] * 7
    want_t0 = [0] * 5 + [1] * 7 + [2] * 7
    assert X[0].shape == (19, 11) and Y[0].tolist() == want_y0
    np.testing.assert_array_equal(X[0][:, 10], np.array(want_a0) / n)
    np.testing.assert_array_equal(X[0][:, :10], state[want_t0, :10].astype(np.float64))
    # learner 1 (dims 3): -1 at 0 -> the single allocation 0, +1 at n_prbs -> the single allocation 6, -1 at 3 -> 0..3
    want_a1 = [0, 6, 0, 1, 2, 3]
    assert X[1].shape == (6, 4) and Y[1].tolist() == [-1, 1, -1, -1, -1, -1]
    np.testing.assert_array_equal(X[1][:, 3], np.array(want_a1) / n)
    np.testing.assert_array_equal(X[1][:, :3], state[[0, 1, 2, 2, 2, 2], 10:13].astype(np.float64))
    # the last coordinate is the reference's a / n_prbs, bit for bit
    assert X[0][0, 10] == 2 / 6 and X[1][5, 3] == 3 / 6
    # no steps: empty lists of the right widths; labels other than +1 / -1 and actions off the grid are refused
    X0, Y0 = augmented_samples(np.zeros((0, 13)), np.zeros((0, 2)), np.zeros((0, 2)), dims, n)
    assert X0[0].shape == (0, 11) and X0[1].shape == (0, 4) and len(Y0[0]) == len(Y0[1]) == 0
    with pytest.raises(ValueError):
        augmented_samples(state, action, np.zeros((3, 2)), dims, n)
    with pytest.raises(ValueError):
        augmented_samples(state, action + 7, labels, dims, n)
