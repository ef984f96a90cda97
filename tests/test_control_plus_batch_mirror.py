"""The group walk without a GPU: tests/control_plus_batch_mirror.py replays the reference's recording G19
(tests/golden/g19_control_plus.npz) teacher-forced at widths 2, 4 and 8 and must not deviate AT ALL from the ungrouped replay
(width 0) -- the f of every sample, every branch, f at the executed allocation, hits, selected actions, adjusted, margins,
security factors, sizes, the accuracy tables, the landmarks, the coefficients and Kinv are compared as bytes: d* of a column
depends on the landmarks and Kinv alone, which only an insertion changes, and an insertion ends its group.  The ungrouped replay
itself takes the recording's branches (tests/test_control_plus_mirror.py holds tests/control_plus_mirror.py to the rest).

expected_work, which computes kb_control_plus_batch_info's eight counters from a recording alone, is held to the mirror's own
counts at every width and at an arena limit that G19's dictionaries cross."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_plus_batch_mirror as bm   # noqa: E402

_cache = {}


def _replay(golden_dir, width, max_landmarks=1024):
    key = (width, max_landmarks)
    if key in _cache:
        return _cache[key]
    g = np.load(os.path.join(golden_dir, 'g19_control_plus.npz'))
    draws = iter(g['ties'])
    mir = bm.BatchControlMirror([10] * 5, 200, g['init_action'], g['init_sec'], accuracy_range=tuple(g['a_range']),
                                tie=lambda: next(draws), width=width, max_landmarks=max_landmarks)
    nxt = np.concatenate([g['state'][1:], g['final_state'][None]])
    rec = dict(hits=[], action_out=[], adjusted=[], margins=[], security=[], set_size=[])
    for i in range(len(g['state'])):
        rec['hits'].append(mir.update_control(g['state'][i], g['action_in'][i], g['labels'][i]))
        act, adj = mir.select_action(nxt[i])
        rec['action_out'].append(act)
        rec['adjusted'].append(adj)
        rec['margins'].append(mir.margins.copy())
        rec['security'].append(mir.security.copy())
        rec['set_size'].append([h.m for h in mir.learners])
    _cache[key] = g, mir, {k: np.asarray(v) for k, v in rec.items()}
    return _cache[key]


def _bytes(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes()


def test_ungrouped_replay_takes_the_recordings_branches(golden_dir):
    g, mir, rec = _replay(golden_dir, 0)
    for s in range(5):
        assert np.array_equal(np.asarray(mir.branches[s], dtype=np.int8), g['branch%d' % s])
    for k in ('hits', 'action_out', 'adjusted', 'margins', 'security', 'set_size'):
        assert np.array_equal(rec[k], g[k]), k
    assert mir.work == [0] * 8


@pytest.mark.parametrize('width', [2, 4, 8])
def test_grouped_replay_has_deviation_zero(golden_dir, width):
    _, ref, rec0 = _replay(golden_dir, 0)
    _, mir, rec = _replay(golden_dir, width)
    for k in rec0:
        assert np.array_equal(rec[k], rec0[k]), k
    assert _bytes(mir.f0) == _bytes(ref.f0)
    assert _bytes(mir.accuracies) == _bytes(ref.accuracies)
    for s in range(5):
        assert mir.branches[s] == ref.branches[s], s
        assert _bytes(mir.f[s]) == _bytes(ref.f[s]), s
        a, b = mir.learners[s], ref.learners[s]
        assert _bytes(a.L) == _bytes(b.L) and _bytes(a.c) == _bytes(b.c) and _bytes(a.P) == _bytes(b.P), s
    # the walk did group: passes were made, groups were skipped, insertions cut groups
    w = mir.work
    assert w[0] > 0 and w[1] > 0 and w[2] > 0 and w[5] > 0 and w[6] > 0 and w[0] == w[1] + w[2]


@pytest.mark.parametrize('width,max_landmarks', [(2, 1024), (4, 1024), (8, 1024), (8, 64)])
def test_expected_work_is_the_mirrors_count(golden_dir, width, max_landmarks):
    g, mir, _ = _replay(golden_dir, width, max_landmarks)
    br = [g['branch%d' % s] for s in range(5)]
    want = bm.expected_work(br, [0] * 5, g['action_in'], g['labels'], width, max_landmarks)
    print(width, max_landmarks, want)
    assert [int(v) for v in mir.work] == want
    assert want[0] == want[1] + want[2] and want[4] - want[5] + want[6] <= sum(len(b) for b in br)
    if max_landmarks == 64:   # G19 ends past one shell: candidates of the larger dictionaries went one by one, with a mat-vec
        assert want[7] > 0 and want[6] > bm.expected_work(br, [0] * 5, g['action_in'], g['labels'], width, 1024)[6]
        _, ref, _ = _replay(golden_dir, 0)
        for s in range(5):
            assert mir.branches[s] == ref.branches[s] and _bytes(mir.learners[s].P) == _bytes(ref.learners[s].P)


def test_expected_work_on_a_hand_made_recording():
    """one learner, n_prbs = 9, two rows: label -1 at action 4 (5 candidates) from 1 landmark, label +1 at action 3 (7 candidates)"""
    br = [np.array([2, 0, 4, 2, 0, 0, 0, 0, 0, 3, 0, 1])]
    # row 0: m = 1 -> one by one (branch 2, m = 2); group of 4 [0, 4, 2, 0]: a pass, cut behind position 2, one column discarded, m = 3;
    #        the last candidate alone: a group of 1, skipped.  row 1: groups [0, 0, 0, 0] skipped, [3, 0, 1] a pass
    w = bm.expected_work(br, [1], [[4], [3]], [[-1], [1]], 4, 64, n_prbs=9)
    assert w == [4, 2, 2, 2, 7, 1, 1, 1]
