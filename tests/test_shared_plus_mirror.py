"""tests/shared_plus_mirror.py against the sequential learner (tests/plus_mirror.py), no GPU: the walk of a list over a dictionary at
its capacity, the one-by-one apply of a dictionary that grows, whole rounds of 24 replicas, and the two deliberately wrong walks
(DESIGN.md section 8q).

Tolerances (teacher-forced): f within 1e-9 (1 + sum |k c|), coefficients within 1e-8 relative to the largest,
Kinv within 1e-8 of its largest entry.  A sample the sequential learner decides within update_mirror.CLEARANCE of a threshold
(the margin against 0 and 1, the slack against 0, the two smallest terms of alpha against each other) would be left out of the
comparison; the lists come from update_mirror's case picker and the rounds' seeds were chosen so that NONE is, and the tests say
so when that breaks."""
import numpy as np
import pytest

import shared_mirror as shm
import shared_plus_mirror as spm
import update_mirror as um

GAMMA, ETA, N_PRBS = 1.0, 0.1, 200
SEEDS = {10: 41, 3: 43}
_cache = {}


def grown(dims):
    if dims not in _cache:
        sizes = sorted({m for m, d, _ in spm.PLUS_CASES if d == dims})
        _cache[dims] = shm.oracle_grown(dims, N_PRBS, sizes, SEEDS[dims], GAMMA, ETA)[0]
    return _cache[dims]


def case_inputs(m, dims, n):
    key = ('list', m, dims, n)
    if key not in _cache:
        Kinv, coeff, L = grown(dims)[m]
        props, cases = spm.plus_list(Kinv, coeff, L, N_PRBS, n, GAMMA, ETA, seed=m + n)
        _cache[key] = (Kinv, coeff, L, props, cases, spm.full_batch_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, ETA))
    return _cache[key]


def sequential(Kinv, coeff, L, props, n_prbs, capacity):
    """the list through ONE capped PlusMirror in order -> (f, branch, near [n], scale [n], the learner)"""
    m, d = np.asarray(L).shape
    mir = spm.CappedPlusMirror(capacity=capacity, gamma=GAMMA, eta=ETA)
    if m:
        mir.L, mir.c, mir.P = np.array(L, dtype=np.float64), np.array(coeff, dtype=np.float64), np.array(Kinv, dtype=np.float64).reshape(m, m)
    X, y, _, _ = shm.unpack(props, len(props), d, n_prbs)
    f, br, near, scale = np.zeros(len(X)), np.zeros(len(X), dtype=np.int32), np.zeros(len(X), dtype=bool), np.zeros(len(X))
    for p in range(len(X)):
        near[p] = mir.m > 0 and spm.near_threshold(mir, X[p], int(y[p]), um.CLEARANCE)
        _, f[p] = mir.predict(X[p])
        scale[p] = float(np.abs(mir.kf * mir.c).sum()) if mir.m else 0.0
        br[p] = mir.update(X[p], int(y[p]))[0]
    return f, br, near, scale, mir


@pytest.mark.parametrize('m,dims,n', spm.PLUS_CASES)
def test_full_batch_plus_is_the_sequential_learner(m, dims, n):
    Kinv, coeff, L, props, cases, mir = case_inputs(m, dims, n)
    f, br, near, scale, seq = sequential(Kinv, coeff, L, props, N_PRBS, m)
    assert not near.any(), ('samples within CLEARANCE of a threshold: the picker was to leave none', int(near.sum()), n)
    assert (mir['branch'] == br).all(), ('branches', mir['branch'].tolist(), br.tolist())
    assert (np.abs(mir['f'] - f) <= 1e-9 * (1.0 + scale)).all(), float((np.abs(mir['f'] - f) / (1.0 + scale)).max())
    assert np.abs(mir['coeff'] - seq.c).max() <= 1e-8 * np.abs(seq.c).max()
    assert mir['n_changed'] == int(((br == 1) | (br == 3)).sum()) and mir['n_work'] == int((br > 0).sum())
    # |w_p| <= 1, so the bounds shared_mirror derives for d* and A (and through them for f_p) carry over to this walk
    assert (np.abs(mir['w']) <= 1.0).all() and (mir['w'][(br == 0) | (br == 4)] == 0.0).all()
    ex = shm.exact_full_batch(Kinv, coeff, mir['KF'], mir['y'])
    B = um.bound_units(m, 'col') + um.exact_units(m)
    ld = np.longdouble
    rd = float((np.abs(mir['DS'].astype(ld) - ex['ds']) / np.maximum(B * um.U * ex['S'], ld(1e-4000))).max())
    ra = float((np.abs(mir['A'].astype(ld) - ex['A']) / ex['EA']).max())
    fx, Ef = spm.exact_f_plus(coeff, mir['KF'], mir['w'], ex)      # f_p = F0_p + sum_{q < p} w_q A[p][q] with the walk's own weights
    rf = float((np.abs(mir['f'].astype(ld) - fx) / Ef).max())
    assert rd <= 1.0 and ra <= 1.0 and rf <= 1.0, (rd, ra, rf)
    print('capacity %d, %d proposals: error / bound d* %.3g, A %.3g, f_p %.3g' % (m, n, rd, ra, rf))
    if n >= 15:      # the list is what it was built to be (test_every_branch_and_term_occurs_somewhere: the rest, over all lists)
        assert {1, 3, 4} <= set(int(b) for b in br), sorted(set(br.tolist()))
        won = {int(np.argmin(t)) for t in mir['terms'] if t is not None}
        assert {0, 2} <= won, ('terms of alpha that won', won, cases)


def test_every_branch_and_term_occurs_somewhere():
    """branch 2 cannot occur in a dictionary at its capacity (growing_apply_plus covers it); over all lists the others do, and so
    does every term of alpha"""
    brs, won = set(), set()
    for m, dims, n in spm.PLUS_CASES:
        mir = case_inputs(m, dims, n)[5]
        brs |= set(int(b) for b in mir['branch'])
        won |= {int(np.argmin(t)) for t in mir['terms'] if t is not None}
    assert brs == {0, 1, 3, 4} and won == {0, 1, 2}, (brs, won)


@pytest.mark.parametrize('m,dims,n', [c for c in spm.PLUS_CASES if c[2] >= 15])
@pytest.mark.parametrize('wrong', spm.WRONG)
def test_a_wrong_walk_changes_the_coefficients(m, dims, n, wrong):
    """weighting a margin step with y instead of alpha y, or forming its loss from F0_p without g_p, must show in the coefficients of
    every list that has a margin step (with alpha < 1; behind an applied proposal) before its last proposal"""
    Kinv, coeff, L, props, cases, mir = case_inputs(m, dims, n)
    steps = [p for p in range(n - 1) if mir['branch'][p] == 3]
    if wrong == 'weight_y':
        assert any(abs(mir['w'][p]) < 1.0 for p in steps), 'no margin step with alpha < 1 before the last proposal'
    else:
        assert any(mir['f'][p] != mir['F0'][p] for p in steps), 'no margin step behind an applied proposal'
    bad = spm.full_batch_plus(Kinv, coeff, L, props, GAMMA, N_PRBS, ETA, wrong=wrong)
    assert (bad['coeff'] != mir['coeff']).any()


@pytest.mark.parametrize('dims,n', [(10, 64), (3, 65)])
def test_growing_apply_plus_is_the_sequential_learner_from_empty(dims, n):
    """a stream from empty through every branch: the first sample inserts (the empty dictionary), the float32 regime of one landmark,
    then projections, insertions and margin steps as they come"""
    states, actions, labels = shm.round_inputs(n, [dims], 50, 1, seed=SEEDS[dims] + 1)[0]       # (states close enough to interact)
    X = np.column_stack([states.astype(np.float64), actions[:, 0] / 50.0])
    Y = labels[:, 0]
    props = np.zeros((len(X), 18))
    for i in range(len(X)):
        props[i, 0], props[i, 1] = i, shm.proposal_word(int(actions[i, 0]), int(Y[i]))
        props[i, 2:2 + dims] = states[i]
    g = spm.growing_apply_plus(np.zeros((0, 0)), np.zeros(0), np.zeros((0, dims + 1)), props, GAMMA, 50, dims + 1, ETA, 256)
    f, br, near, scale, seq = sequential(np.zeros((0, 0)), np.zeros(0), np.zeros((0, dims + 1)), props, 50, 256)
    assert near.sum() <= 0.01 * len(X), ('samples within CLEARANCE of a threshold', int(near.sum()))
    assert not near.any(), 'the seed was chosen so that no sample is left out'
    assert (g['branch'] == br).all(), ('branches', g['branch'].tolist(), br.tolist())
    # (ten state variables keep these samples apart: their mistakes insert; the learner of three projects some as well)
    assert set(br.tolist()) >= ({1, 2, 3, 4} if dims == 3 else {2, 3, 4}), sorted(set(br.tolist()))
    assert g['m'] == seq.m >= 3
    assert (np.abs(g['f'] - f) <= 1e-9 * (1.0 + scale)).all()
    assert np.abs(g['coeff'] - seq.c).max() <= 1e-8 * np.abs(seq.c).max()
    assert np.abs(g['kinv'] - seq.P).max() <= 1e-8 * np.abs(seq.P).max()
    assert g['landmarks'].tobytes() == seq.L.tobytes()


@pytest.mark.parametrize('budget', [4, 64])
def test_rounds_reproduce_one_sequential_learner_per_slice(budget):
    """24 replicas, dims [10, 3], 50 PRBs, 12 steps of 4 rounds from empty: the mirror's own stages (scan_plus on the device-order
    dictionaries' plain scores, collect, growing_apply_plus, commit) beside PlusRounds -- one sequential PlusMirror per slice fed the
    merged lists in order"""
    dims, N, n_prbs, rounds, steps = [10, 3], 24, 50, 4, 12
    off = [0, 10]
    ref = spm.PlusRounds(dims, n_prbs, N, GAMMA, ETA)
    state = [dict(kinv=np.zeros((0, 0)), coeff=np.zeros(0), landmarks=np.zeros((0, d + 1))) for d in dims]
    seen = dict(rounds=0, over_budget=0, branches=set())
    for step, (states, actions, labels) in enumerate(shm.round_inputs(N, dims, n_prbs, steps, seed=8)):
        ref.begin(states, actions, labels)
        cursor = np.zeros((N, 2), dtype=np.int64)
        for rnd in range(rounds):
            want, _, out = ref.scan()
            assert not out.any(), ('pairs within 1e-9 of a threshold: the seed was chosen so that none is', step, rnd)
            cstar = np.full((N, 2), -1, dtype=np.int64)
            for s in (0, 1):
                for e in range(N):
                    f, _ = shm.plain_scores(state[s]['landmarks'], state[s]['coeff'], states[e, off[s]:off[s] + dims[s]], n_prbs, GAMMA)
                    r = spm.scan_plus(f, int(labels[e, s]), int(actions[e, s]), int(cursor[e, s]), rnd, n_prbs, len(state[s]['coeff']))
                    cstar[e, s], cursor[e, s] = r['cstar'], r['cursor']
            assert (cstar == want).all(), ('proposals', step, rnd)
            cnt, lists, props = shm.collect(cstar, budget, states, labels, 0, off, dims)
            if cnt.sum() == 0:
                break
            seen['rounds'] += 1
            seen['over_budget'] += int((cnt > budget).sum())
            res = ref.apply(lists)
            for s in (0, 1):
                b = state[s]
                g = spm.growing_apply_plus(b['kinv'], b['coeff'], b['landmarks'], props[s], GAMMA, n_prbs, dims[s] + 1, ETA, 256,
                                           count=len(lists[s]))
                assert [int(v) for v in g['branch']] == [br for _, br in res[s]], ('branches', step, rnd, s)
                seen['branches'] |= set(int(v) for v in g['branch'])
                o = ref.oa[s]
                assert g['m'] == o.m and g['landmarks'].tobytes() == o.L.tobytes()
                assert np.abs(g['coeff'] - o.c).max() <= 1e-8 * np.abs(o.c).max()
                assert np.abs(g['kinv'] - o.P).max() <= 1e-8 * np.abs(o.P).max()
                state[s] = dict(kinv=g['kinv'], coeff=g['coeff'], landmarks=g['landmarks'])
            cursor = shm.commit(cstar, [len(l) for l in lists], cursor)
            ref.commit([len(l) for l in lists])
    assert ref.near <= 0.01 * ref.samples and ref.near == 0 and ref.open == 0, (ref.near, ref.samples, ref.open)
    assert seen['branches'] >= {1, 2, 3, 4} and seen['rounds'] > steps and (budget >= N or seen['over_budget'] > 0), seen
