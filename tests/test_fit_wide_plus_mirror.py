"""The round structure of kb_fit's wide path in Projectron++ mode without a GPU (tests/fit_wide_plus_mirror.py):
on G18's d4 stream (1,200 samples) and the first 1,200 samples of G18's rev stream, teaching by rounds -- whatever the window,
the chunk and the threshold -- leaves exactly what plus_mirror.replay(..., plus=True) leaves: every y_pred, branch and size, and
every f, delta, coefficient, Kinv entry and the cached kernel column with deviation 0.  The counters the rounds count on their way
are those `counters` derives from the branch codes and sizes alone, which is what the device test compares kb_fit_wide_info
with; they also state the choice made after branch 4 (every round scans again: nothing of a window is used twice)."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_wide_plus_mirror as fwp   # noqa: E402
import plus_mirror as pm             # noqa: E402

SETTINGS = list(itertools.product((1, 3, 64), (7, 256), (2, 65)))   # window, chunk, min_landmarks


def _draws(g):
    """the recorded tie draws, restarted for every run"""
    it = iter(g['ties'])
    return lambda: next(it)


@pytest.fixture(scope='module', params=['d4', 'rev_1200'])
def stream(request, golden_dir):
    tag = request.param.split('_')[0]
    z = np.load(os.path.join(golden_dir, 'g18_projectron_plus.npz'))
    g = {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + '_')}
    x, y = g['x'][:1200], g['y'][:1200]
    assert len(x) == 1200
    seq, sout = pm.replay(x, y, g['ties'], plus=True)
    assert np.array_equal(sout['branch'], g['branch'][:1200]) and np.array_equal(sout['m'], g['m'][:1200])
    sout['delta'] = np.where(sout['branch'] == 0, 0.0, sout['delta'])   # branch 0 reports delta 0, as kb_fit does
    return request.param, g, x, y, seq, sout


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.uint64),
                                                 np.ascontiguousarray(b, dtype=np.float64).view(np.uint64))


def test_sequential_mode_is_the_replay(stream):
    _, g, x, y, seq, sout = stream
    mir, out, info = fwp.fit(x, y, tie=_draws(g))
    assert info == [0, 0, 0, 0]
    for k in ('ypred', 'branch', 'm'):
        assert np.array_equal(out[k], sout[k]), k
    for k in ('f', 'delta'):
        assert _same(out[k], sout[k]), k
    assert _same(mir.L, seq.L) and _same(mir.c, seq.c) and _same(mir.P, seq.P)


@pytest.mark.parametrize('window,chunk,min_landmarks', SETTINGS)
def test_rounds_leave_the_sequential_result(stream, window, chunk, min_landmarks):
    name, g, x, y, seq, sout = stream
    mir, out, info = fwp.fit(x, y, chunk=chunk, min_landmarks=min_landmarks, window=window, tie=_draws(g))
    for k in ('ypred', 'branch', 'm'):
        assert np.array_equal(out[k], sout[k]), k
    for k in ('f', 'delta'):
        assert _same(out[k], sout[k]), k
    assert _same(mir.L, seq.L) and _same(mir.c, seq.c) and _same(mir.P, seq.P)
    assert mir.f == seq.f and _same(mir.kf, seq.kf)
    # the counters: counted by the rounds, and derived from where the samples of branches 1-4 are
    assert info == fwp.counters(sout['branch'], sout['m'], 0, chunk=chunk, min_landmarks=min_landmarks, window=window)
    before = np.concatenate([[0], sout['m'][:-1]])
    wide_from = next((r0 for r0 in range(0, len(x), chunk) if before[r0] >= min_landmarks), None)
    if wide_from is None:
        assert info == [0, 0, 0, 0]
    else:
        # once wide, always wide (a dictionary never shrinks): the rounds taught everything from that chunk on
        br = sout['branch'][wide_from:]
        assert info[0] == len(x) - wide_from
        assert info[1] == int((br != 0).sum())       # a mat-vec for every mistake AND every margin sample, branch 4 included
        assert info[1] > int(((br == 1) | (br == 2)).sum()) and (br == 3).any() and (br == 4).any()
        every_sample_once = int(before[wide_from:].sum())
        assert info[3] >= every_sample_once
        if window == 1:
            assert info[3] == every_sample_once   # a window of one never rescans
        elif window == 64 and chunk == 256:
            # no reuse after branch 4: a round that ended in one is followed by a scan of a whole window again
            assert info[3] > every_sample_once + int((br == 4).sum())


def test_the_streams_reach_the_cases(stream):
    name, g, x, y, _, sout = stream
    assert set(np.unique(sout['branch'])) == {0, 1, 2, 3, 4}
    if name == 'rev_1200':
        assert sout['m'].max() >= 129     # past two shell boundaries: both thresholds are crossed inside the stream
    else:
        assert sout['m'].max() == 18      # the threshold of 65 is never reached: that setting stays sequential
        # exact ties against a populated dictionary: sample 3 meets one landmark (sequential), sample 4 two (a round, threshold 2)
        assert (sout['f'][3:5] == 0.0).all() and sout['m'][2] == 1 and sout['m'][3] == 2
