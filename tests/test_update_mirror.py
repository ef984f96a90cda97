"""tests/update_mirror.py on the CPU: the restated order of one Projectron.update against the oracle (its own float64 program),
against exact arithmetic, and against three other summation orders -- the inputs must be able to tell the orders apart, or a
device test that compares bits with the mirror would pass whatever the kernel did.

Dictionaries come from an OracleKBRL learner on _fast_growing_samples (tests/test_gpu_kbrl.py); at every size of SIZES the next
sample of the stream that is projected and the one that is inserted are taken through update_mirror.step from the ORACLE's state
before the step.  Run with -s for the largest error / bound ratios (DESIGN.md §2 quotes them).
"""
import numpy as np
import pytest

import update_mirror as um
from oracle import pyoracle as po
from test_gpu_kbrl import _fast_growing_samples

SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 319, 320, 321, 513]
GAMMA, ETA = 1.0, 0.1


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def contrasts(Kinv, kf, ds):
    """how many outputs of each contrasting order differ in bits from the stated one"""
    n = lambda other: int((np.asarray(other).view(np.uint64) != np.asarray(ds).view(np.uint64)).sum())
    return dict(column_walk=n(um.dstar_col(Kinv, kf)), rows_first=n(um.dstar_tri(Kinv, kf, rows_first=True)[0]),
                linear_tree=n(um.dstar_tri(Kinv, kf, linear_tree=True)[0]))


def discriminates(m, diff):
    """three blocks and more: every contrasting order must show; two blocks: the combine's order cannot (d + t == t + d), the
    other two must; one block: the tile's sums ARE the column walk, only the tree can show (required from 16 landmarks on)"""
    if m > 128:
        return all(v > 0 for v in diff.values())
    if m > 64:
        return diff['column_walk'] > 0 and diff['linear_tree'] > 0
    return m < 16 or diff['linear_tree'] > 0


class Lockstep:
    """the oracle learner and the stream; state() is what a step starts from"""

    def __init__(self):
        self.oa = po.OracleKBRL([10], 200, [10], [3], gamma=GAMMA, eta=ETA, capacity=1024)
        self.oa.set_seed(0)
        self.xs, self.ys = _fast_growing_samples(4000)
        self.i = 0

    def state(self):
        return self.oa.kinv(0), self.oa.coeff(0), self.oa.landmarks(0)

    def mistake(self, x, y):
        """predict; True when Projectron.update(x, y) will act"""
        return self.oa.predict(0, x)[1] * y <= 0


@pytest.fixture(scope='module')
def cases():
    """[(m, kind, state before, x, y, the mirror's step, oracle's (branch, delta), oracle's state after, contrast counts)] for every
    size of SIZES and both kinds, from ONE pass over the stream"""
    ls, out = Lockstep(), []
    oa = ls.oa
    for m in SIZES:
        while oa.m(0) < m:      # the stream as it comes, up to the size
            x, y = ls.xs[ls.i], int(ls.ys[ls.i])
            ls.i += 1
            oa.predict(0, x)
            oa.update(0, x, y)
        assert oa.m(0) == m, 'the stream skipped size %d' % m
        done = set()
        while oa.m(0) == m:
            x, y = ls.xs[ls.i], int(ls.ys[ls.i])
            ls.i += 1
            if not ls.mistake(x, y):
                continue
            before = ls.state()
            mir = um.step(*before, x, y, GAMMA, ETA)
            kind = {1: 'projects', 2: 'inserts'}[mir['branch']]
            diff = contrasts(before[0], mir['column'], mir['dstar']) if m >= 2 else {}
            keep = kind not in done and (m < 2 or discriminates(m, diff))
            if kind == 'inserts' and 'projects' not in done:
                # the insertion is about to leave this size and no projection of it has been taken: near-duplicates of its
                # landmarks with the label the learner does not predict are projected (delta <= eta), until one discriminates
                L = before[2]
                for j in range(m):
                    xp = L[j].copy()
                    xp[:10] = (xp[:10] + 0.01).astype(np.float32)
                    yp = -1 if oa.predict(0, xp)[1] > 0 else 1
                    b4 = ls.state()
                    mp = um.step(*b4, xp, yp, GAMMA, ETA)
                    dp = contrasts(b4[0], mp['column'], mp['dstar']) if m >= 2 else {}
                    if mp['branch'] != 1 or not (m < 2 or discriminates(m, dp)):
                        continue
                    out.append((m, 'projects', b4, xp, yp, mp, oa.update(0, xp, yp), ls.state(), dp))
                    done.add('projects')
                    break
                assert 'projects' in done, 'no projection that tells the orders apart at size %d' % m
                if not ls.mistake(x, y):     # (the cached prediction is the stream's sample again; the projection may have
                    continue                 # put it right)
                before = ls.state()
                mir = um.step(*before, x, y, GAMMA, ETA)
                diff = contrasts(before[0], mir['column'], mir['dstar']) if m >= 2 else {}
                kind = {1: 'projects', 2: 'inserts'}[mir['branch']]
                keep = kind not in done and (m < 2 or discriminates(m, diff))
            res = oa.update(0, x, y)
            if keep:
                out.append((m, kind, before, x, y, mir, res, ls.state(), diff))
                done.add(kind)
        assert done == {'projects', 'inserts'}, 'size %d: only %s told the orders apart -- pick another stream' % (m, sorted(done))
    return out


def test_every_size_has_both_kinds(cases):
    assert sorted({(m, k) for m, k, *_ in cases}) == sorted((m, k) for m in SIZES for k in ('inserts', 'projects'))


def test_mirror_agrees_with_the_oracle(cases):
    """branch and size exactly; delta, coefficients and Kinv within the tolerances the device is held to against the reference's
    recording (G9, tests/test_gpu_kbrl.py: delta 1e-7, coefficients 1e-8 + 1e-9, Kinv 1e-8 of its entry + 1e-8 of its scale)"""
    for m, kind, before, x, y, mir, (obr, odl), after, _ in cases:
        assert mir['branch'] == obr == {'projects': 1, 'inserts': 2}[kind], (m, kind)
        assert mir['m'] == len(after[1]) == m + (obr == 2), (m, kind)
        assert mir['delta'] == pytest.approx(odl, rel=1e-7, abs=1e-9), (m, kind)
        np.testing.assert_array_equal(mir['landmarks'], after[2])
        np.testing.assert_allclose(mir['coeff'], after[1], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(mir['kinv'], after[0], rtol=1e-8, atol=1e-8 * np.abs(after[0]).max())


def test_mirror_and_oracle_keep_their_forward_bounds(cases):
    """|d* - Kinv K_f| <= bound_units u S_i for the stated order, and for the oracle's row walk (restated: the oracle hands out no
    d*; a projection shows it: coeff + y d* of the restated walk must be the oracle's new coefficients bit for bit)"""
    worst, most = dict(tri=0.0, col=0.0, rows=0.0), dict(tri=0.0, col=0.0, rows=0.0)
    for m, kind, before, x, y, mir, _, after, _ in cases:
        if m < 2:
            assert mir['dstar'].tolist() == mir['column'].tolist()
            continue
        Kinv, kf = before[0], mir['column']
        # (the oracle sums the squared distance pairwise, as numpy does: its own kernel column)
        kfo = po.detmath('EXP_INLINE', -GAMMA * np.array([po.pairwise_sum(r) for r in (before[2] - x[None]) ** 2]))
        dr = um.dstar_rows(Kinv, kfo)
        if kind == 'projects':
            assert same_bits(before[1] + float(y) * dr, after[1]), (m, 'the row walk is not the oracle')
        for order, ds, k in (('tri', mir['dstar'], kf), ('col', um.dstar_col(Kinv, kf), kf), ('rows', dr, kfo)):
            r, units = um.error_ratio(ds, Kinv, k, order)
            assert r <= 1.0, (m, kind, order, r)
            worst[order] = max(worst[order], r)
            most[order] = max(most[order], units)
    print('d* error / bound: stated order %.3g, column walk %.3g, oracle row walk %.3g; largest error in units of u S_i: %.3g, %.3g, '
          '%.3g' % (worst['tri'], worst['col'], worst['rows'], most['tri'], most['col'], most['rows']))


def test_inputs_tell_the_orders_apart(cases):
    for m, kind, before, x, y, mir, _, _, diff in cases:
        if m >= 2:
            assert discriminates(m, diff), (m, kind, diff)
    big = [d for m, *_, d in cases if m > 128]
    print('outputs that differ from the stated order, least over the cases of three blocks and more: column walk %d, rows first %d, '
          'linear tree %d' % tuple(min(d[k] for d in big) for k in ('column_walk', 'rows_first', 'linear_tree')))


def test_new_kinv_is_symmetric_bit_for_bit(cases):
    for m, kind, _, _, _, mir, _, _, _ in cases:
        assert same_bits(mir['kinv'], mir['kinv'].T), (m, kind)


def test_a_wrong_order_shows_in_the_partials():
    """the switches the device test's diagnosis relies on: chains over index mod 4 change the tiles' partial sums, the combine's
    order leaves them alone"""
    rng = np.random.default_rng(5)
    A = rng.normal(size=(200, 200))
    K, kf = A @ A.T, rng.random(200)
    ds, dp, tp = um.dstar_tri(K, kf)
    ds4, dp4, tp4 = um.dstar_tri(K, kf, classes=4)
    dsr, dpr, tpr = um.dstar_tri(K, kf, rows_first=True)
    assert not same_bits(ds, ds4) and any(not same_bits(dp[t], dp4[t]) for t in dp)
    assert not same_bits(ds, dsr) and all(same_bits(dp[t], dpr[t]) for t in dp) and all(same_bits(tp[t], tpr[t]) for t in tp)
    assert um.error_ratio(ds4, K, kf)[0] <= 1.0     # (wrong order, still accurate: only the bits can tell)
