"""tests/shared_plus_batch_mirror.py against the one-by-one mirror and the sequential learner, no GPU: the
segmented apply of a growing shared dictionary takes growing_apply_plus's branches and ends within section 8q's tolerances of it,
and the two deliberately wrong variants show.

Tolerances (teacher-forced): f within 1e-9 (1 + sum |k c|), coefficients within 1e-8 relative to the largest,
Kinv within 1e-8 of its largest entry.  No sample the mirror applies may lie within update_mirror.CLEARANCE of a threshold -- the
margin against 0 and 1, the slack against 0, the two smallest terms of alpha against each other, and for a mistake below the capacity
max(1 - A[p][p], 0) and residual_delta against eta: a condition on the inputs, whose seeds were chosen so that NONE does."""
import numpy as np
import pytest

import shared_mirror as shm
import shared_plus_batch_mirror as sbm
import shared_plus_mirror as spm
import update_mirror as um

GAMMA, ETA, N_PRBS = 1.0, 0.1, 200
SEEDS = {10: 41, 3: 43}
_cache = {}


def grown(dims):
    if dims not in _cache:
        sizes = sorted({c[0] for c in sbm.BATCH_CASES if c[1] == dims})
        _cache[dims] = shm.oracle_grown(dims, N_PRBS, sizes, SEEDS[dims], GAMMA, ETA)[0]
    return _cache[dims]


def case_inputs(case):
    if case not in _cache:
        m, dims, n, ins, extra = case
        Kinv, coeff, L = grown(dims)[m]
        props, seq = sbm.batch_list(Kinv, coeff, L, N_PRBS, n, ins, m + extra, GAMMA, ETA, seed=m + n)
        seg = sbm.segmented_apply_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, dims + 1, ETA, m + extra, 2)
        one = spm.growing_apply_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, dims + 1, ETA, m + extra)
        _cache[case] = (Kinv, coeff, L, props, seq, seg, one)
    return _cache[case]


@pytest.mark.parametrize('case', sbm.BATCH_CASES)
def test_segments_take_the_one_by_one_branches(case):
    m, dims, n, ins, extra = case
    Kinv, coeff, L, props, seq, seg, one = case_inputs(case)
    assert seg['engaged'] and seg['near'] == 0, ('applied samples within CLEARANCE of a threshold: the seeds were to leave none', seg['near'])
    assert seg['branch'].tolist() == one['branch'].tolist() == seq, (seg['branch'].tolist(), one['branch'].tolist(), seq)
    # the list is what it was built to be
    grow = [i for i in ins][:extra]
    assert [p for p in range(n) if seg['branch'][p] == 2] == grow, (seg['branch'].tolist(), ins)
    assert seg['m'] == one['m'] == m + len(grow) and seg['n_grow'] == len(grow)
    assert seg['sat'] == (len(ins) > extra)
    assert seg['work'] == [1, len(grow) + (0 if grow and grow[-1] == n - 1 else 1), sum(n - f for f in [0] + [g + 1 for g in grow] if f < n),
                           len(grow)], seg['work']
    assert seg['seg'].tolist() == [sum(1 for g in grow if g < p) for p in range(n)]
    # f of the one-by-one mirror is a fresh k . coeff; the walk's is F0 + a chain of fused multiply-adds
    X, y, _, _ = shm.unpack(props, n, dims + 1, N_PRBS)
    mir = spm.CappedPlusMirror(capacity=m + extra, gamma=GAMMA, eta=ETA)
    mir.L, mir.c, mir.P = L.copy(), coeff.copy(), Kinv.copy()
    for p in range(n):
        mir.predict(X[p])
        scale = float(np.abs(mir.kf * mir.c).sum())
        assert abs(seg['f'][p] - one['f'][p]) <= 1e-9 * (1.0 + scale), (p, seg['f'][p], one['f'][p])
        mir.update(X[p], int(y[p]))
    assert seg['landmarks'].tobytes() == one['landmarks'].tobytes()
    assert np.abs(seg['coeff'] - one['coeff']).max() <= 1e-8 * np.abs(one['coeff']).max()
    assert np.abs(seg['kinv'] - one['kinv']).max() <= 1e-8 * np.abs(one['kinv']).max()
    assert seg['n_changed'] == sum(1 for b in seq if b in (1, 2, 3)) and seg['n_work'] == sum(1 for b in seq if b)


def test_every_branch_and_term_occurs():
    brs, won = set(), set()
    for case in sbm.BATCH_CASES:
        seg = case_inputs(case)[5]
        brs |= set(int(b) for b in seg['branch'])
        won |= {int(np.argmin(t)) for t in seg['terms'] if t is not None}
    assert brs == {0, 1, 2, 3, 4} and won == {0, 1, 2}, (brs, won)


WRONG_CASES = [(c, w) for c in sbm.BATCH_CASES for w in sbm.WRONG
               if c[3] and min(c[3]) < c[2] - 1 and (w == 'stale_f0' or min(c[3]) >= 3)]


@pytest.mark.parametrize('case,wrong', WRONG_CASES)
def test_a_wrong_variant_changes_the_coefficients(case, wrong):
    """F0 kept over an insertion, or g carried into the next segment, must show in the coefficients of every list that holds an
    insertion followed by at least one applied sample (carry_g: and behind one -- g is still 0.0 when the list's first applied
    sample is the insertion itself, and carrying it changes nothing)"""
    m, dims, n, ins, extra = case
    Kinv, coeff, L, props, seq, seg, one = case_inputs(case)
    grew = [p for p in range(n) if seg['branch'][p] == 2]
    assert any(seg['branch'][q] in (1, 2, 3) for q in range(grew[0] + 1, n)), 'no applied sample behind the insertion'
    if wrong == 'carry_g':
        assert any(seg['branch'][q] in (1, 3) for q in range(grew[0])), 'no applied sample before the insertion'
    bad = sbm.segmented_apply_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, dims + 1, ETA, m + extra, 2, wrong=wrong)
    assert bad['coeff'].shape != seg['coeff'].shape or (bad['coeff'] != seg['coeff']).any()


def test_a_list_that_is_not_engaged_goes_as_before():
    m, dims, n, ins, extra = sbm.BATCH_CASES[3]
    Kinv, coeff, L, props, seq, seg, one = case_inputs(sbm.BATCH_CASES[3])
    low = sbm.segmented_apply_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, dims + 1, ETA, m + extra, m + 1)
    assert not low['engaged'] and low['work'] == [0, 0, 0, 0]
    assert low['coeff'].tobytes() == one['coeff'].tobytes() and low['kinv'].tobytes() == one['kinv'].tobytes()
    full = sbm.segmented_apply_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, dims + 1, ETA, m, 2)
    want = spm.full_batch_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, ETA)
    assert not full['engaged'] and full['coeff'].tobytes() == want['coeff'].tobytes() and full['m'] == m
