"""tests/update_mirror.py on the CPU: the restated order of one Projectron.update against the oracle (its own float64 program),
against exact arithmetic, and against three other summation orders -- the inputs must be able to tell the orders apart, or a
device test that compares bits with the mirror would pass whatever the kernel did.

Dictionaries come from an OracleKBRL learner on _fast_growing_samples (tests/test_gpu_kbrl.py); at every size of SIZES the next
sample of the stream that is projected and the one that is inserted are taken through update_mirror.step from the ORACLE's state
before the step.  Run with -s for the largest error / bound ratios (DESIGN.md §2 quotes them).

Below them the same for ONE ProjectronPlus.update (update_mirror.step_plus): it replays the reference's recording G18 walking
alone, keeps its derived bounds against exact arithmetic (exact_plus, plus_bounds) on every margin sample of those replays, and
its contrast switches show on the inputs tests/test_gpu_plus_chain.py uses (DESIGN.md §8i quotes the ratios).
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


# ------------------------------------------------------------------ Projectron++: step_plus
def _tag(golden_dir, tag):
    import os
    g = np.load(os.path.join(golden_dir, 'g18_projectron_plus.npz'))
    return {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + '_')}


def _close(a, b, rtol, atol, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    bad = np.abs(a - b) > np.maximum(rtol * np.abs(b), atol)
    assert not bad.any(), (what, np.nonzero(bad)[0][:5], a[bad][:5], b[bad][:5])


@pytest.fixture(scope='module', params=['d4', 'rev'])
def walked(request, golden_dir):
    """step_plus from the empty dictionary through all 1,200 samples of G18's d4 stream, and through samples 0 .. 440 of its rev
    stream (past 64 -> 65 landmarks), fed nothing but its own state -> (tag, recording, [(state before, stages)])"""
    g = _tag(golden_dir, request.param)
    n = 1200 if request.param == 'd4' else 441
    state = (np.zeros((0, 0)), np.zeros(0), np.zeros((0, g['x'].shape[1])))
    steps = []
    for i in range(n):
        r = um.step_plus(*state, g['x'][i], int(g['y'][i]), GAMMA, ETA)
        r['y'] = int(g['y'][i])
        steps.append((state, r))
        state = (r['kinv'], r['coeff'], r['landmarks'])
    return request.param, g, steps


def test_step_plus_replays_the_recording_walking_alone(walked):
    """every branch and size equals the recording; f, delta and the final coefficients within the tolerances
    tests/test_gpu_projectron_plus.py holds the device to (f 1e-8 / 1e-9, delta 1e-7 / 1e-9; coefficients 1e-8 / 1e-9 on d4, with
    the vector after each of its 147 margin updates and the final Kinv, and 1e-7 / 1e-8 on rev -- there against the float64
    restatement tests/plus_mirror.py on the same prefix, which tests/test_plus_mirror.py holds to the whole recording)"""
    import plus_mirror as pm
    tag, g, steps = walked
    n = len(steps)
    br = np.array([r['branch'] for _, r in steps])
    assert np.array_equal(br, g['branch'][:n]), np.nonzero(br != g['branch'][:n])[0][:5]
    assert np.array_equal([r['m'] for _, r in steps], g['m'][:n])
    _close([r['f'] for _, r in steps], g['f'][:n], 1e-8, 1e-9, tag + ' f')
    upd = br != 0
    _close(np.array([r['delta'] for _, r in steps])[upd], g['delta'][:n][upd], 1e-7, 1e-9, tag + ' delta')
    assert not np.array([r['delta'] for _, r in steps])[~upd].any()
    margin = br >= 3
    _close(np.array([r['slack'] for _, r in steps])[margin], g['slack'][:n][margin], 1e-7 / ETA, 1e-9 / ETA, tag + ' slack')
    last = steps[-1][1]
    if tag == 'd4':
        assert np.array_equal(last['landmarks'], g['landmarks'])
        np.testing.assert_allclose(last['coeff'], g['coeff'], rtol=1e-8, atol=1e-9)
        np.testing.assert_allclose(last['kinv'], g['kinv'], rtol=1e-8, atol=1e-8 * np.abs(g['kinv']).max())
        after = [r['coeff'] for _, r in steps if r['branch'] == 3]
        assert len(after) == len(g['coeff_after']) == 147
        for c, ref in zip(after, g['coeff_after']):
            np.testing.assert_allclose(c, ref[:len(c)], rtol=1e-8, atol=1e-9)
        assert any(r['branch'] >= 3 and len(b[1]) == 1 for b, r in steps)       # the float32 regime meets the margin rule
    else:
        mir, _ = pm.replay(g['x'][:n], g['y'][:n], g['ties'], eta=ETA, gamma=GAMMA)
        assert last['m'] == mir.m == g['m'][n - 1] > 65 and np.array_equal(last['landmarks'], mir.L)
        np.testing.assert_allclose(last['coeff'], mir.c, rtol=1e-7, atol=1e-8)
        assert np.bincount(br[338:438], minlength=5).tolist() == [21, 4, 13, 8, 54] and g['m'][337] < 64 < 65 < g['m'][437] == 74


def test_step_plus_keeps_its_bounds_against_exact_arithmetic(walked):
    """on every margin sample of the replays: f and the new coefficients within plus_bounds of exact_plus on the same doubles (d*
    within bound_units); where the exact margin and slack are clear of their thresholds by more than the bound the branch is the
    exact one, and where the exact terms of alpha are clear of each other the winning term is"""
    tag, g, steps = walked
    worst, seen = dict(f=0.0, coeff=0.0, dstar=0.0), dict(branch=0, won=0, margin=0)
    for (Kinv, c, L), r in steps:
        if r['branch'] < 3:
            continue
        m, y = len(c), r['y']
        ex = um.exact_plus(Kinv, r['column'], c, y, ETA)
        bd = um.plus_bounds(ex, m, ETA)
        rt = um.plus_ratios(dict(f=r['f'], coeff=r['coeff'] if r['branch'] == 3 else None), ex, bd)
        assert all(v <= 1.0 for v in rt.values()), (tag, m, r['branch'], rt)
        for k, v in rt.items():
            worst[k] = max(worst[k], v)
        if m >= 2:
            rd, _ = um.error_ratio(r['dstar'], Kinv, r['column'])
            assert rd <= 1.0, (tag, m, rd)
            worst['dstar'] = max(worst['dstar'], rd)
        seen['margin'] += 1
        if min(float(ex['margin']), 1.0 - float(ex['margin'])) > bd['f'] and abs(float(ex['slack'])) > bd['slack']:
            assert r['branch'] == ex['branch'], (tag, m, r['branch'], ex['branch'], float(ex['slack']), bd['slack'])
            seen['branch'] += 1
            if r['branch'] == 3 and bd['won_clear']:
                assert r['won'] == ex['won'], (tag, m, r['won'], ex['won'], ex['terms'])
                seen['won'] += 1
    print('%s: margin samples %d, branch decided clear of the bound %d, winning term %d; largest error / bound: f %.3g, d* %.3g, '
          'coefficients %.3g' % (tag, seen['margin'], seen['branch'], seen['won'], worst['f'], worst['dstar'], worst['coeff']))
    assert seen['branch'] > 0.9 * seen['margin'] and seen['won'] > 0


@pytest.fixture(scope='module')
def plus_inputs():
    """the inputs of tests/test_gpu_plus_chain.py, built without a device: dictionaries of the ladder's sizes grown in Projectron
    mode by the float64 restatement (tests/plus_mirror.py) on the two streams, one sample per case of the margin rule from
    update_mirror.PlusInputs, and the hand-built single-landmark points -> [(name, m, case or point, state, x, y)]"""
    import plus_mirror as pm
    from test_gpu_update_chain import _stream3
    out = []
    for name, (xs, ys), sizes in (('dims 10', _fast_growing_samples(4600), um.PLUS_LADDER10), ('dims 3', _stream3(3000), um.PLUS_LADDER3)):
        mir, i = pm.PlusMirror(gamma=GAMMA, eta=ETA, plus=False), 0
        for m in sizes:
            while mir.m < m:
                mir.predict(xs[i])
                mir.update(xs[i], int(ys[i]))
                i += 1
            assert mir.m == m
            state = (mir.P.copy(), mir.c.copy(), mir.L.copy())
            inp = um.PlusInputs(state[0], state[2], GAMMA, ETA, 200)
            found = []
            for case in um.CASES:      # one after the other on the same learner, as the device test takes them
                p = inp.pick(state[1], case)
                if p is not None:
                    found.append(case)
                    out.append((name, m, case, state, p[0], p[1]))
                    state = (state[0], um.step_plus(*state, p[0], p[1], GAMMA, ETA)['coeff'], state[2])
            assert set(um.cases_required(m)) <= set(found), (name, m, found, inp.counts(state[1]))
    b = um.one_landmark_inputs(GAMMA, ETA)
    x0 = b['x0']
    for point, near, x in b['points']:
        assert x is not None, point
        st = um.step_plus(np.ones((1, 1)), [1.0], x0[None], near, -1, GAMMA, ETA)
        out.append(('one landmark', 1, point, (st['kinv'], st['coeff'], st['landmarks']), x, 1))
    out.append(('one landmark', 1, 'x0', (np.ones((1, 1)), np.ones(1), x0[None]), x0, 1))
    return out


def test_the_mirror_names_the_case_the_float64_preselection_chose(plus_inputs):
    """the clearance of 1e-6 is far above the rounding of either: step_plus's branch and winning term are the wanted case; the
    single-landmark points meet all five cases, and both exact ties"""
    met = set()
    for name, m, case, state, x, y in plus_inputs:
        r = um.step_plus(*state, x, y, GAMMA, ETA)
        got = {0: 'branch0', 4: 'branch4', 3: r['won']}.get(r['branch'])
        if name == 'one landmark':
            met.add(got)
            if case == 'x0':
                assert r['margin'] == 1.0 and r['branch'] == 0
            if case == 'tie_alpha':
                assert r['terms'][0] == 1.0 and r['won'] == 'loss' and r['alpha'] == 1.0
            if case == 'tie_slack':
                assert r['slack'] == 0.0 and r['branch'] == 4
            if case not in ('x0', 'tie_slack'):
                assert 0 < r['coeff'][0] and r['coeff'][0] == np.float32(r['coeff'][0]) and r['loss'] == np.float32(r['loss'])
        else:
            assert got == case, (name, m, case, got)
    assert met == set(um.CASES), met


def test_inputs_show_every_contrast_switch_of_the_margin_rule(plus_inputs):
    """each deliberately wrong form of the rule changes at least one output (f, branch, winning term, delta or a coefficient, as
    bits) on these inputs -- a device test that compares them with step_plus on the same inputs would see such a fault.  What
    each can show at all: loss64 only while one landmark is held; alpha_order only the name of the winner on an exact tie of two
    terms (the minimum itself does not depend on the order) and slack_ge only slack == 0.0 exactly -- the two hand-built ties;
    fused_coeff and f_pairwise on the larger dictionaries."""
    shows = {k: 0 for k in um.PLUS_SWITCHES}
    view = lambda r: (np.float64(r['f']).tobytes(), r['branch'], r['won'], np.float64(r['delta']).tobytes(), r['coeff'].tobytes())
    for name, m, case, state, x, y in plus_inputs:
        base = view(um.step_plus(*state, x, y, GAMMA, ETA))
        for k in um.PLUS_SWITCHES:
            if (k == 'loss64') != (m == 1) and k not in ('alpha_order', 'slack_ge'):
                continue      # (loss64 is the m == 1 statement; the sums' switches cannot show on one landmark)
            shows[k] += view(um.step_plus(*state, x, y, GAMMA, ETA, **{k: True})) != base
    print('inputs on which each switch shows: %s of %d' % (shows, len(plus_inputs)))
    assert all(v > 0 for v in shows.values()), shows
