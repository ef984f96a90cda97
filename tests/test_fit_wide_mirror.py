"""The round structure of kb_fit's wide path without a GPU (tests/fit_wide_mirror.py): on G9's d4 stream and the
first 1,500 samples of G14, teaching by rounds -- whatever the window, the chunk and the threshold -- leaves exactly what the
sequential loop leaves: every y_pred, branch and size, and every f, delta, coefficient, Kinv entry and the cached kernel column
with deviation 0.  The counters the rounds count on their way are those `counters` derives from the branch codes and sizes alone,
which is what the device test compares kb_fit_wide_info with."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_wide_mirror as fw   # noqa: E402
import plus_mirror as pm       # noqa: E402

SETTINGS = list(itertools.product((1, 3, 64), (7, 256), (2, 65)))   # window, chunk, min_landmarks


def _ties():
    """a fixed stream of draws, restarted for every run"""
    rng = np.random.default_rng(11)
    return lambda: int(rng.integers(0, 2)) * 2 - 1


@pytest.fixture(scope='module', params=['g9_d4', 'g14_1500'])
def stream(request, golden_dir):
    if request.param == 'g9_d4':
        g = np.load(os.path.join(golden_dir, 'g9_projectron.npz'))
        x, y = g['d4_x'], g['d4_y']
    else:
        g = np.load(os.path.join(golden_dir, 'g14_projectron_long.npz'))
        x, y = g['x'][:1500], g['y'][:1500]
    mir, out, info = fw.fit(x, y, tie=_ties())
    assert info == [0, 0, 0, 0]
    return request.param, x, y, mir, out


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                                                 np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def test_sequential_mode_is_the_replay(stream):
    """min_landmarks = 0 is plus_mirror.replay's loop (branch 0 reports delta 0 here, as kb_fit does)"""
    _, x, y, mir, out = stream
    ref, rout = pm.replay(x, y, ties=iter(_ties(), None), plus=False)
    for k in ('f', 'ypred', 'branch', 'm'):
        assert np.array_equal(out[k], rout[k]), k
    assert _same(out['delta'], np.where(rout['branch'] == 0, 0.0, rout['delta']))
    assert _same(mir.c, ref.c) and _same(mir.P, ref.P)


@pytest.mark.parametrize('window,chunk,min_landmarks', SETTINGS)
def test_rounds_leave_the_sequential_result(stream, window, chunk, min_landmarks):
    name, x, y, seq, sout = stream
    mir, out, info = fw.fit(x, y, chunk=chunk, min_landmarks=min_landmarks, window=window, tie=_ties())
    for k in ('ypred', 'branch', 'm'):
        assert np.array_equal(out[k], sout[k]), k
    for k in ('f', 'delta'):
        assert _same(out[k], sout[k]), k
    assert _same(mir.L, seq.L) and _same(mir.c, seq.c) and _same(mir.P, seq.P)
    assert mir.f == seq.f and _same(mir.kf, seq.kf)
    # the counters: counted by the rounds, and derived from where the mistakes are
    assert info == fw.counters(sout['branch'], sout['m'], 0, chunk=chunk, min_landmarks=min_landmarks, window=window)
    wide_from = next((r0 for r0 in range(0, len(x), chunk) if r0 and sout['m'][r0 - 1] >= min_landmarks), None)
    if wide_from is None:
        assert info == [0, 0, 0, 0]
    else:
        # once wide, always wide (a dictionary never shrinks): the rounds taught everything from that chunk on
        assert info[0] == len(x) - wide_from
        assert info[1] == int((sout['branch'][wide_from:] != 0).sum())
        assert info[3] >= int(np.concatenate([[0], sout['m'][:-1]])[wide_from:].sum())   # at least every sample once
        if window == 1:
            assert info[3] == int(np.concatenate([[0], sout['m'][:-1]])[wide_from:].sum())   # a window of one never rescans


def test_the_streams_reach_the_cases(stream):
    name, x, y, _, sout = stream
    if name == 'g14_1500':
        assert sout['m'].max() >= 129     # past two shell boundaries: both thresholds are crossed inside the stream
    else:
        assert 2 <= sout['m'].max() < 65  # the threshold of 65 is never reached: that setting stays sequential
