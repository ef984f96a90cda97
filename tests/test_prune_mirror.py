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
out), so the removal sequence does not hang on the last bits of P.

And the mirror against the written rule: Mirror.remove_one() equals, bit for bit, remove_one_scalar() -- one removal in Python
floats and loops, straight from the seven steps of kb_prune.hip's header, its argmin over (bit pattern of the key, slot) -- on
dictionaries of 5, 64, 65 and 70 landmarks with ties, keys of +0.0, subnormal keys, keys of +inf and the victim in the last slot."""
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


# ---- the vectorised mirror against the written rule: remove_one() == remove_one_scalar(), bit for bit
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _loaded(m, seed):
    """a mirror loaded through from_state with a genuine Kinv of m random landmarks, random coefficients and grid indices
    (some off the grid)"""
    rng = np.random.default_rng(seed)
    L = rng.random((m, 4)) * 3.0
    src = pm.build_from_landmarks(L, rng.standard_normal(m), GAMMA)
    idx = rng.integers(-1, 6, size=m)
    return pm.Mirror.from_state(src.L, src.c, src.P, idx)


def _natural(mr):
    pass


def _zero_ties(mr):
    """three keys of +0.0 (one from c = -0.0): slots 1, 3 and the last leave in that order, whatever moves in between"""
    mr.c[[1, 3]] = 0.0
    mr.c[mr.m - 1] = -0.0


def _last_slot(mr):
    """r == m - 1: nothing moves"""
    mr.c[mr.m - 1] = 0.0


def _subnormal(mr):
    """c^2 is subnormal in slots 2 and 4 (the smaller in the higher slot), and underflows to +0.0 in slot 0 behind them"""
    mr.c[2], mr.c[4], mr.c[0] = 3e-160, 2e-160, 1e-170


def _overflow(mr):
    """every c^2 overflows: all keys are +inf, the lowest slot leaves; then all but one, whose key is the only finite one"""
    mr.c[:] = np.where(np.arange(mr.m) % 2 == 0, 1e200, -1.5e190)


def _overflow_but_one(mr):
    mr.c[:] = 1e200
    mr.c[mr.m - 2] = 1e150


def _equal_nonzero(mr):
    """two equal keys that are not zero: slots 1 and m - 2 get the same small coefficient and the larger of their two diagonal
    entries (raising a diagonal entry keeps P positive definite: every later key stays a key the device admits)"""
    a, b = 1, mr.m - 2
    mr.c[a] = mr.c[b] = 1e-9
    mr.P[a, a] = mr.P[b, b] = max(mr.P[a, a], mr.P[b, b])


@pytest.mark.parametrize('edit', [_natural, _zero_ties, _last_slot, _subnormal, _overflow, _overflow_but_one, _equal_nonzero])
@pytest.mark.parametrize('m', [5, 64, 65, 70])
def test_remove_one_is_the_written_rule(m, edit):
    """three removals on dictionaries loaded through from_state: the victim, the landmarks, the coefficients, every entry of P
    and the grid indices of the NumPy mirror equal, as bytes, those of the restatement in Python floats and loops, which is
    written from the seven steps in kb_prune.hip's header and takes its argmin over (bit pattern of the key as uint64, slot).
    With keys of +0.0, subnormal keys and +inf among them this also pins that the bit pattern orders as the value does for
    every key the device admits (a finite coefficient over a finite positive diagonal entry: never negative, never NaN)."""
    mr = _loaded(m, 100 + m)
    edit(mr)
    first = None
    with np.errstate(over='ignore', invalid='ignore'):
        for n in range(3):
            keys = (mr.c * mr.c) / np.diag(mr.P)
            assert not np.isnan(keys).any() and not np.signbit(keys).any()
            assert [pm.key_bits(float(k)) for k in keys] == [int(b) for b in keys.view(np.uint64)]
            order = np.lexsort((np.arange(mr.m), keys))        # by value, then by slot
            assert sorted(range(mr.m), key=lambda j: (pm.key_bits(float(keys[j])), j)) == list(order)
            r, L, c, P, idx = pm.remove_one_scalar(mr.L.tolist(), mr.c.tolist(), mr.P.tolist(), mr.idx.tolist())
            step = mr.remove_one()
            first = step['slot'] if first is None else first
            what = (m, edit.__name__, n)
            assert step['slot'] == r == int(order[0]), what
            assert _bits(mr.L) == _bits(L), what
            assert _bits(mr.c) == _bits(c), what
            assert _bits(mr.P) == _bits(P), what
            assert mr.idx.tolist() == idx and mr.m == m - 1 - n, what
            assert np.array_equal(mr.P, mr.P.T), what
    want_first = {'_zero_ties': 1, '_last_slot': m - 1, '_subnormal': 0, '_overflow': 0, '_overflow_but_one': m - 2,
                  '_equal_nonzero': 1}
    if edit.__name__ in want_first:
        assert first == want_first[edit.__name__]


def test_from_state_carries_the_grid_indices():
    mr = pm.Mirror.from_state(np.arange(8.0).reshape(4, 2), [1.0, 0.0, 1.0, 1.0], np.eye(4), idx=[3, 5, -1, 7])
    assert mr.remove_one()['slot'] == 1
    assert mr.idx.tolist() == [3, 7, -1] and mr.ids == [0, 3, 2] and mr.L.tolist() == [[0.0, 1.0], [6.0, 7.0], [4.0, 5.0]]
    with pytest.raises(ValueError):
        pm.Mirror.from_state(np.zeros((3, 2)), np.zeros(3), np.eye(4))


def test_chains_invariant():
    head, link = pm.chains(np.array([3, -1, 3, 7, 3]))
    assert head[3] == 4 and head[7] == 3 and (np.delete(head, [3, 7]) == -1).all()
    assert list(link) == [-1, -1, 0, -1, 2]
