"""tests/scoring_mirror.py against exact arithmetic and the oracle, on the CPU: the documented order of the KBRL scoring chain
(bins in increasing j by segments, ONE fma chain over the grid indices, direct terms under the KB_E_TINY / KB_F_SETTLED rules),
fed with the oracle's exponentials, stays within the derived forward bound of sum_j coeff_j exp(-gamma |l_j - x_c|^2) in mpmath,
and decides every candidate as the oracle's predict does.  Each test prints its largest error / bound ratios (-s).
"""
import numpy as np
import pytest

import scoring_mirror as sm
from oracle import pyoracle as po

N_PRBS = 50
NARROW = [0.0]   # the largest mirror error / (p_max + KA + 5) u S seen by check_case so far
LADDER = [0, 1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 321, 513]


def grow_oracle(m, dims, n_prbs, seed, off_grid=()):
    """an oracle learner of exactly m landmarks: distinct random samples, alternating labels, until m have been inserted"""
    oa = po.OracleKBRL([dims], n_prbs, [0], [0], capacity=max(m, 2))
    oa.set_seed(seed)
    rng = np.random.default_rng(seed)
    X = sm.random_samples(rng, 3 * m + 60, dims, n_prbs)
    sm.grow(m, X, lambda x: oa.predict(0, x), lambda x, y: oa.update(0, x, y)[0], lambda: oa.m(0), set(off_grid), rng)
    return oa


def check_case(oa, state, n_prbs, gamma=1.0):
    """-> (worst mirror error / bound, worst oracle error / bound, candidates inside the bound)"""
    L, co = oa.landmarks(0), oa.coeff(0)
    m, d = oa.m(0), int(oa.dims[0]) + 1
    D0, E, idx, lam = sm.rows(L.reshape(m, d), state, n_prbs, gamma) if m else (np.zeros(0),) * 4
    out = sm.ordered_scores(E, idx, co, lam, D0, sm.gtable(gamma, n_prbs), n_prbs, gamma)
    fx, S, A = sm.exact_scores(L, co, state, n_prbs, gamma)
    tol = sm.tolerance_single(S) if m == 1 else sm.tolerance(out['p_max'], n_prbs, d, gamma, S, A, m, out['fdirect'] >> 8)
    err = sm.errors(out['F'], fx)
    of = np.zeros(n_prbs + 1)
    oy = np.zeros(n_prbs + 1, dtype=int)
    for c in range(n_prbs + 1):
        x = np.concatenate([np.asarray(state, dtype=np.float32).astype(np.float64), [c / n_prbs]])
        oy[c], of[c] = oa.predict(0, x)
    oerr = sm.errors(of, fx)
    assert (err <= tol).all(), (m, int(np.argmax(err / tol)), float((err / tol).max()))
    clear = np.array([abs(v) for v in fx], dtype=np.longdouble) > tol
    my = np.sign(out['F']).astype(int)
    if m:
        assert (my[clear] == oy[clear]).all(), (m, np.nonzero(my[clear] != oy[clear]))
        assert (np.sign(of)[clear] == my[clear]).all()
    inside = int((~clear).sum())
    if m >= 2:   # (printed only: against the constant that leaves out the exponentials' argument error)
        nar = np.longdouble(sm.issue_units(out['p_max'], n_prbs) * sm.U) * S + m * np.longdouble(sm.TINY)
        NARROW[0] = max(NARROW[0], float((err / np.where(nar > 0, nar, 1)).max()))
    tol = np.where(tol > 0, tol, 1)   # (an empty dictionary: no error and no bound)
    return float((err / tol).max()), float((oerr / tol).max()), inside, out


@pytest.mark.parametrize('m', LADDER)
def test_ordered_scores_within_the_bound_of_exact_and_signs_as_the_oracle(m):
    dims = 10 if LADDER.index(m) % 2 == 0 else 3
    oa = grow_oracle(m, dims, N_PRBS, 1000 + m)
    rng = np.random.default_rng(m)
    worst = [0.0, 0.0]
    for _ in range(2):
        state = rng.uniform(0.0, sm.SPREAD[dims], dims).astype(np.float32)
        if m == 1:   # (float32 arithmetic: a state near the landmark, or k is below the float32 range)
            state = (oa.landmarks(0)[0, :dims] + rng.uniform(-0.5, 0.5, dims)).astype(np.float32)
        r_m, r_o, inside, out = check_case(oa, state, N_PRBS)
        if m >= 1:
            assert inside <= (N_PRBS + 1) // 100, 'more than 1 %% of the candidates inside the bound: %d' % inside
        worst = [max(worst[0], r_m), max(worst[1], r_o)]
    print('m = %d, dims = %d: mirror error / bound %.3g, oracle error / bound %.3g; so far error / (p_max + KA + 5) u S %.3g'
          % (m, dims, worst[0], worst[1], NARROW[0]))


@pytest.mark.parametrize('n_off', [1, 47, 48, 49, 130])
def test_off_grid_landmarks_take_the_direct_terms(n_off):
    m = 150
    off = list(range(3, 3 + n_off))
    oa = grow_oracle(m, 10, N_PRBS, 2000 + n_off, off_grid=off)
    state = np.random.default_rng(n_off).uniform(0.0, 2.0, 10).astype(np.float32)
    r_m, r_o, inside, out = check_case(oa, state, N_PRBS)
    assert out['fdirect'] == (3 | (n_off << 8)) and out['open'].all()
    assert inside <= (N_PRBS + 1) // 100
    print('%d off the grid: mirror error / bound %.3g, oracle error / bound %.3g' % (n_off, r_m, r_o))


def band_state(oa, dims):
    return np.full(dims, sm.band_coordinate(oa.landmarks(0)[:, :dims]), dtype=np.float32)


@pytest.mark.parametrize('dims', [10, 3])
def test_band_state_takes_the_direct_terms_exactly(dims):
    """every E_j is below KB_E_TINY or zero: the binned sums are zero, every candidate is open and gets the exact exponentials
    of the landmarks in the band (subnormal values, a few quanta): within m quanta of exact, signs as the oracle's"""
    oa = grow_oracle(257, dims, N_PRBS, 3000 + dims)
    state = band_state(oa, dims)
    D0, E, idx, lam = sm.rows(oa.landmarks(0), state, N_PRBS, 1.0)
    band = (E > 0) & (E < sm.KB_E_TINY)
    assert band.any() and not (E >= sm.KB_E_TINY).any()
    r_m, r_o, inside, out = check_case(oa, state, N_PRBS)
    nb = int(band.sum())
    assert out['fdirect'] == (1 | (nb << 8)) and out['open'].all() and not out['W'].any()
    assert inside <= (N_PRBS + 1) // 100, inside
    # the scores are subnormal here, so the values are also held to the oracle's directly, in quanta: both sum the same nb
    # products coeff_j k_j(c), the oracle rounding each product and adding exactly, the mirror rounding each fused step -- half
    # a quantum per term each.
    q = sm.TINY
    of = np.array([oa.predict(0, np.append(state.astype(np.float64), c / N_PRBS))[1] for c in range(N_PRBS + 1)])
    assert out['F'].any() and (np.abs(out['F'] - of) <= nb * q).all(), np.abs(out['F'] - of).max() / q
    clear = np.abs(of) > nb * q
    assert (np.sign(out['F'])[clear] == np.sign(of)[clear]).all()
    print('band, dims %d: %d landmarks in the band, mirror error / bound %.3g, oracle %.3g, %d candidates inside the bound, '
          'mirror - oracle at most %g quanta, %d candidates beyond %d quanta'
          % (dims, nb, r_m, r_o, inside, np.abs(out['F'] - of).max() / q, clear.sum(), nb))


def test_settled_candidates_keep_their_binned_sum():
    """one binned landmark with E = 2e-240 at grid index 0 (G falls from 1 to 1 / e along the candidates: the binned sum crosses
    1e-240) and two band landmarks: candidates at or above KB_F_SETTLED keep the binned sum bit for bit, the others take the
    direct terms"""
    n = 255
    oa = po.OracleKBRL([3], n, [0], [0], capacity=8)
    oa.set_seed(1)
    near = np.array([0.5 + 23.493, 0.5, 0.5, 0.0])
    bandl = [np.array([26.8, 0.5, 0.5, 1.0]), np.array([0.5, 26.9, 0.5, 100.0 / 255.0])]
    for x in [near] + bandl:
        y, _ = oa.predict(0, x)
        assert oa.update(0, x, -y if y else 1)[0] == 2
    state = np.array([0.5, 0.5, 0.5], dtype=np.float32)
    D0, E, idx, lam = sm.rows(oa.landmarks(0), state, n, 1.0)
    assert 1e-240 < E[0] < 2.7e-240 and ((E[1:] > 0) & (E[1:] < sm.KB_E_TINY)).all()
    out = sm.ordered_scores(E, idx, oa.coeff(0), lam, D0, sm.gtable(1.0, n), n, 1.0)
    assert out['fdirect'] == (1 | (2 << 8))
    settled = np.abs(out['binned']) >= sm.KB_F_SETTLED
    assert settled.any() and (~settled).any()
    assert (out['F'][settled] == out['binned'][settled]).all() and (out['open'] == ~settled).all()
    r_m, r_o, inside, _ = check_case(oa, state, n)
    assert inside <= (n + 1) // 100, inside
    print('settled rule: mirror error / bound %.3g, oracle %.3g, %d candidates inside the bound' % (r_m, r_o, inside))


@pytest.mark.parametrize('m,dims', [(2, 10), (70, 3), (321, 10)])
def test_all_underflow_state_is_an_exact_tie_everywhere(m, dims):
    oa = grow_oracle(m, dims, N_PRBS, 4000 + m)
    state = sm.far_state(dims, 60.0)
    D0, E, idx, lam = sm.rows(oa.landmarks(0), state, N_PRBS, 1.0)
    assert not E.any()
    out = sm.ordered_scores(E, idx, oa.coeff(0), lam, D0, sm.gtable(1.0, N_PRBS), N_PRBS, 1.0)
    assert not out['F'].any() and out['fdirect'] == 0 and not np.signbit(out['F']).any()
    for c in range(N_PRBS + 1):
        y, f = oa.predict(0, np.concatenate([state.astype(np.float64), [c / N_PRBS]]))
        assert f == 0.0 and y in (-1, 1)
    # the oracle's select_action on that state, twice: each tie takes one draw of the learner's stream, the first +1 is accepted
    # (security factor 0: the action is the accepted candidate, n_prbs when none is), and the predictions made are counted
    ob = po.OracleKBRL([dims], N_PRBS, [0], [0], capacity=max(m, 2))
    X = sm.random_samples(np.random.default_rng(4000 + m), 3 * m + 60, dims, N_PRBS)
    sm.grow(m, X, lambda x: ob.predict(0, x), lambda x, y: ob.update(0, x, y)[0], lambda: ob.m(0))
    ob.set_seed(77)   # (after the growth, whose own ties draw too: the stream starts over)
    draws, ctr = [], 0
    for _ in range(2 * (N_PRBS + 1)):
        v, ctr = po.stream_probe('PM1', [[77, 0, 0, 0xffffffff, ctr]])[0]
        draws.append(int(v))
        ctr = int(ctr)
    n0, pos = ob.stats()[0], 0
    for _ in range(2):
        c, used = sm.first_accepted(out['F'], draws[pos:])
        act, adj = ob.select_action(state)
        assert int(act[0]) == (c if c >= 0 else N_PRBS) and adj == 0, (act, c, pos)
        pos += used
    assert ob.stats()[0] - n0 == pos, 'one prediction, and one draw, per candidate scanned'

def test_fraction_fma_is_the_oracles_fma():
    import primitives_util as pu
    from fractions import Fraction
    a, b, c = (v[:3000] for v in pu.fma_inputs())
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    a, b, c = a[fin], b[fin], c[fin]
    ref = po.detmath('FMA', a, np.concatenate([b, c]))
    ok = np.isfinite(ref)
    got = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a[ok].tolist(), b[ok].tolist(), c[ok].tolist())])
    nz = got != 0.0   # (an exact zero result: the Fraction has no sign)
    assert (got[nz].view(np.uint64) == ref[ok][nz].view(np.uint64)).all() and (ref[ok][~nz] == 0.0).all()
