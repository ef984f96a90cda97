"""The pruning rule of kb_prune, checked on its float64 mirror (tests/prune_mirror.py) without a GPU: after pruning to half,
the mirror's P is the inverse Gram matrix of the survivors (against a longdouble inverse), and the squared RKHS distance
between the classifier before and after every removal is c_r^2 / P[r][r].

Tolerance: the project's stated Kinv tolerance -- 1e-8 relative to the matrix's scale, 1e-6 for dictionaries
of thousands of landmarks.  The cases below hold up to 1,000 landmarks and take 1e-8.  One of them cannot meet it for a reason
that is not the pruning: the whole G14 dictionary starts with two landmarks close to each other, and the Projectron's recursion
forms its first kernel value in float32 (as the reference does), which leaves P 3.4e-8 of its scale away from the longdouble
inverse BEFORE anything is pruned (3.294e-08 before, 3.366e-08 after).  For that case the recorded distance stands in, with ten
times over it allowed (MIRROR_DISTANCE; both numbers are in profiles/prune_record.json, "mirror_vs_longdouble"), and every case
is also held to 1e-8 against the Schur complement of the mirror's OWN starting P in longdouble, which the float32 value does not
enter.
Fixture quality: at every removal the winner's key lies at least 1e-6 relative below the runner-up's (asserted, no case left
out), so the removal sequence does not hang on the last bits of P."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_mirror as pm   # noqa: E402

GAMMA = 1.0
KINV_RTOL = 1e-8
GAP = 1e-6
# the mirror's measured distance from the longdouble inverse where it exceeds KINV_RTOL (see above); the bound is 10 x this
MIRROR_DISTANCE = {('g14_projectron_long', 790, 0): 3.366e-08}
# (fixture, landmarks drawn, seed): random landmark sets of the G14 (790 landmarks) and G17 (3,143) dictionaries, pruned to half
CASES = [('g14_projectron_long', 790, 0), ('g14_projectron_long', 300, 1), ('g17_projectron_3000', 600, 2),
         ('g17_projectron_3000', 1000, 3)]


def landmark_pool(golden_dir, name):
    g = np.load(os.path.join(golden_dir, name + '.npz'))
    if 'landmarks' in g.files:
        return g['landmarks'], g['coeff']
    xs = np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1)
    return xs[g['branch'] == 2], g['coeff']


def draw(golden_dir, name, n, seed):
    L, c = landmark_pool(golden_dir, name)
    pick = np.sort(np.random.default_rng(seed).choice(len(L), size=n, replace=False))
    return L[pick], c[pick]


@pytest.mark.parametrize('name,n,seed', CASES)
def test_survivors_inverse_and_error_identity(golden_dir, name, n, seed):
    L, c = draw(golden_dir, name, n, seed)
    mr = pm.build_from_landmarks(L, c, GAMMA)
    assert mr.m == n
    P0 = mr.P.astype(np.longdouble)
    G = pm.gram_exact(L, GAMMA, np.float64)
    target = n // 2
    worst_id, worst_gap = 0.0, np.inf
    alive = list(range(n))       # original landmark behind every slot
    while mr.m > target:
        Gm = G[np.ix_(alive, alive)]
        step = mr.remove_one()
        assert step['diag_ok']
        worst_gap = min(worst_gap, step['gap'])
        assert step['gap'] >= GAP, (mr.m, step['gap'])
        # ||f_before - f_after||^2_H through the Gram matrix of the landmarks before the removal
        r, last = step['slot'], len(alive) - 1
        after = np.zeros(last + 1)
        after[:last] = mr.c
        if r != last:
            after[last] = after[r]   # undo the move: the survivor now in slot r sat in the last slot
        after[r] = 0.0
        dc = step['c_before'] - after
        err2 = float(dc @ Gm @ dc)
        want = step['cr'] ** 2 / step['q']
        worst_id = max(worst_id, abs(err2 - want) / max(want, 1e-300) if want > 1e-12 else abs(err2 - want))
        assert err2 == pytest.approx(want, rel=KINV_RTOL, abs=1e-12), mr.m
        if r != last:
            alive[r] = alive[last]
        alive.pop()
    assert [mr.ids[j] for j in range(mr.m)] == alive
    np.testing.assert_array_equal(mr.L, L[alive])
    ref = pm.inv_longdouble(pm.gram_exact(L[alive], GAMMA, np.longdouble))
    scale = float(np.abs(ref).max())
    dist = float(np.abs(mr.P.astype(np.longdouble) - ref).max()) / scale
    print('%s n=%d seed=%d: |P - inv(G)| / scale = %.3e, error identity worst %.3e, smallest gap %.3e'
          % (name, n, seed, dist, worst_id, worst_gap))
    assert dist <= (10 * MIRROR_DISTANCE[(name, n, seed)] if (name, n, seed) in MIRROR_DISTANCE else KINV_RTOL)
    gone = sorted(set(range(n)) - set(alive))
    schur = P0[np.ix_(alive, alive)] - P0[np.ix_(alive, gone)] @ pm.inv_longdouble(P0[np.ix_(gone, gone)]) @ P0[np.ix_(gone, alive)]
    own = float(np.abs(mr.P.astype(np.longdouble) - schur).max()) / scale
    print('    against the Schur complement of its own starting P: %.3e' % own)
    assert own <= KINV_RTOL
    assert np.array_equal(mr.P, mr.P.T)


def test_tie_takes_the_lowest_slot():
    """two landmarks with equal keys: the lower slot leaves first"""
    L = np.array([[0.0, 0.0], [3.0, 0.0], [0.0, 3.0], [3.0, 3.0]])
    mr = pm.build_from_landmarks(L, [1.0, 1.0, 1.0, 1.0], GAMMA)
    mr.P = np.diag([2.0, 1.0, 1.0, 2.0])
    step = mr.remove_one()
    assert step['slot'] == 0 and step['gap'] == 0.0
    mr.c = np.array([1.0, 0.5, 0.5])
    mr.P = np.diag([1.0, 1.0, 1.0])
    assert mr.remove_one()['slot'] == 1


def test_chains_invariant():
    head, link = pm.chains(np.array([3, -1, 3, 7, 3]))
    assert head[3] == 4 and head[7] == 3 and (np.delete(head, [3, 7]) == -1).all()
    assert list(link) == [-1, -1, 0, -1, 2]
