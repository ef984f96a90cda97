"""A plain restatement of the KBRL scoring chain of kb_select_action / update_control (csrc/kb_kbrl.hip: bin_one_chunk, bin_pass /
select_bin_big_body, select_gemm_kernel / chain_scores, add_direct_terms, score_single), stage by stage, and the exact value
it approximates.  Used by tests/test_scoring_mirror.py (CPU); a device test feeds ordered_scores the rows that kb_dev_get_rows of
the test build returns.  Not a test module.

The chain, for a learner with landmarks l_j (last coordinate lam_j), coefficients coeff_j, the state x and candidates
x_c = (x, c / n_prbs), c = 0 .. n_prbs:

  rows      D0_j = sum over the state coordinates, in order from 0.0, of (l_jq - x_q)^2;  E_j = rs_exp_nonpos(-gamma D0_j);
            a_j = the integer with a_j / n_prbs == lam_j exactly, else -1 (off the candidate grid)
  direct    landmark j takes the direct evaluation when a_j < 0 or 0 < E_j < KB_E_TINY = 1e-300; E_j == 0 drops out
  W         W[a] = sum of coeff_j E_j (one rounding each) over the other landmarks with a_j = a whose product is not zero: in
            increasing j within a SEGMENT of KB_BIN_SEG x 64 = 256 landmarks, from 0.0; the segments' sums added in order from 0.0
  F         F(c) = ONE chain f <- fma(G[|a - c|], W[a], f) over a = 0 .. KA - 1 from 0.0, KA = (n_prbs + 4) & ~3,
            G[k] = rs_exp_nonpos(-gamma (k / n_prbs)^2)
  direct    a candidate is OPEN when some landmark is off the grid or its F(c) is not >= KB_F_SETTLED = 1e-240 in magnitude; open
            candidates then take f <- fma(coeff_j, rs_exp_nonpos(-gamma (D0_j + (lam_j - c / n_prbs)^2)), f) over the direct
            landmarks in increasing j (each operation rounded: the build has no contraction)
  m == 1    f(c) = float32(float32(rs_exp(-gamma (D0 + (lam - c / n_prbs)^2))) * float32(coeff)); m == 0: f = 0
"""
import math
from fractions import Fraction

import numpy as np

KB_E_TINY = 1e-300
KB_F_SETTLED = 1e-240
KB_CH = 64
KB_BIN_SEG = 4
U = 2.0 ** -53
TINY = 2.0 ** -1074


def fma(a, b, c):
    """the correctly rounded a * b + c of three doubles (the direct terms: math.fma where Python has it).  The Fraction form has
    no signed zero: an exactly cancelling sum gives +0.0, as round-to-nearest does, but a product that underflows to nothing
    added to -0.0 would too, where the hardware keeps -0.0.  No chain here starts from or reaches -0.0 other than through such an
    underflow, and the device comparison treats zeros of either sign as equal (tests/test_gpu_scoring.py: values_equal)."""
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _exp(op, x):
    from oracle import pyoracle as po   # rs_exp / rs_exp_nonpos: the bits tests/test_gpu_primitives.py pins the device to
    return po.detmath(op, np.ascontiguousarray(x, dtype=np.float64))


def gtable(gamma, n_prbs):
    """G[k], k = 0 .. 255 (kb_gtab_kernel)"""
    t = np.arange(256, dtype=np.float64) / float(n_prbs)
    return _exp('EXP_NONPOS', -gamma * (t * t))


def grid_index(lam, n_prbs):
    """a with float(a) / n_prbs == lam exactly, else -1 (grid_index)"""
    lam = np.asarray(lam, dtype=np.float64)
    r = np.rint(lam * float(n_prbs))
    ok = (r >= 0.0) & (r <= float(n_prbs))
    a = np.where(ok, r, 0.0).astype(np.int64)
    ok &= a.astype(np.float64) / float(n_prbs) == lam
    return np.where(ok, a, -1).astype(np.int32)


def rows(landmarks, state, n_prbs, gamma):
    """(D0, E, idx, lam) as the binning pass leaves them in the dictionary's rows; state: the float32 observation"""
    L = np.asarray(landmarks, dtype=np.float64)
    x = np.asarray(state, dtype=np.float32).astype(np.float64)
    d0 = np.zeros(len(L))
    for q in range(L.shape[1] - 1):
        t = L[:, q] - x[q]
        d0 = d0 + t * t
    return d0, _exp('EXP_NONPOS', -gamma * d0), grid_index(L[:, -1], n_prbs), L[:, -1].copy()


def direct_mask(E, idx):
    E, idx = np.asarray(E), np.asarray(idx)
    return (idx < 0) | (~(E >= KB_E_TINY) & (E > 0.0))


def bin_sums(E, idx, coeff):
    """W[256] and the largest number of landmarks one bin received"""
    E, idx, coeff = np.asarray(E, dtype=np.float64), np.asarray(idx), np.asarray(coeff, dtype=np.float64)
    m = len(E)
    binned = ~direct_mask(E, idx) & (idx >= 0)
    w = coeff * E
    W = np.zeros(256)
    count = np.zeros(256, dtype=np.int64)
    seg = KB_BIN_SEG * KB_CH
    for j0 in range(0, m, seg):
        Ws = np.zeros(256)
        for j in range(j0, min(j0 + seg, m)):
            if binned[j] and w[j] != 0.0:
                Ws[idx[j]] += w[j]
                count[idx[j]] += 1
        W = W + Ws
    return W, int(count.max()) if m else 0


def chain(W, G, n_prbs, ka=None):
    """F[c], c = 0 .. n_prbs: one fused multiply-add chain over a = 0 .. KA - 1 from 0.0 (a zero W[a] leaves f as it is).
    Always through Fraction (correctly rounded; see fma() for the one case it cannot express, a result of -0.0: a chain whose
    terms all underflow from below gives +0.0 here and may give -0.0 on the hardware -- equal as values, not as bits)."""
    KA = (n_prbs + 4) & ~3 if ka is None else ka
    nz = [a for a in range(KA) if W[a] != 0.0]
    Wf = {a: Fraction(float(W[a])) for a in nz}
    Gf = [Fraction(float(g)) for g in G[:256]]
    F = np.zeros(n_prbs + 1)
    for c in range(n_prbs + 1):
        f = 0.0
        for a in nz:
            f = float(Gf[abs(a - c)] * Wf[a] + Fraction(f))
        F[c] = f
    return F


def ordered_scores(E, idx, coeff, lam, D0, G, n_prbs, gamma=1.0):
    """The f64 bits the device should produce from its own E / idx / coeff / lam / D0 rows and G table.
    -> dict(W [256], F [n_prbs + 1], binned = F before the direct terms, fdirect = flags | count << 8 as bin_pass returns it,
            open = the candidates that took the direct terms, p_max)"""
    E, D0 = np.asarray(E, dtype=np.float64), np.asarray(D0, dtype=np.float64)
    coeff, lam, idx = np.asarray(coeff, dtype=np.float64), np.asarray(lam, dtype=np.float64), np.asarray(idx)
    m = len(E)
    cand = np.arange(n_prbs + 1)
    tc = cand.astype(np.float64) / float(n_prbs)
    if m == 0:
        return dict(W=np.zeros(256), F=np.zeros(n_prbs + 1), binned=np.zeros(n_prbs + 1), fdirect=0,
                    open=np.zeros(n_prbs + 1, dtype=bool), p_max=0)
    if m == 1:
        dl = lam[0] - tc
        k = _exp('EXP_INLINE', -gamma * (D0[0] + dl * dl))
        F = (k.astype(np.float32) * np.float32(coeff[0])).astype(np.float64)
        return dict(W=np.zeros(256), F=F, binned=F.copy(), fdirect=0, open=np.zeros(n_prbs + 1, dtype=bool), p_max=1)
    W, p_max = bin_sums(E, idx, coeff)
    binned = chain(W, G, n_prbs)
    direct = direct_mask(E, idx)
    ndir = int(direct.sum())
    flags = (1 if ndir else 0) | (2 if (idx < 0).any() else 0)
    F = binned.copy()
    is_open = np.zeros(n_prbs + 1, dtype=bool)
    if ndir:
        is_open = np.full(n_prbs + 1, bool(flags & 2)) | ~(np.abs(binned) >= KB_F_SETTLED)
        oc = cand[is_open]
        for j in np.nonzero(direct)[0]:
            dl = lam[j] - tc[oc]
            e = _exp('EXP_NONPOS', -gamma * (D0[j] + dl * dl))
            for i, c in enumerate(oc):
                F[c] = fma(float(coeff[j]), float(e[i]), float(F[c]))
    return dict(W=W, F=F, binned=binned, fdirect=flags | (ndir << 8), open=is_open, p_max=p_max)


def first_accepted(F, draws=None):
    """select_action's scan (kbrl_control.py:54-61): the first candidate with f > 0; an exact tie f == 0 takes the next of `draws`
    (+-1) and is accepted on +1.  -> (candidate or -1, draws used)"""
    used = 0
    for c, f in enumerate(F):
        if f > 0.0:
            return c, used
        if f == 0.0:
            assert draws is not None, 'an exact tie needs the tie-break stream'
            used += 1
            if draws[used - 1] == 1:
                return c, used
    return -1, used


# ------------------------------------------------------------------ the exact value and the scale of the forward error
def exact_scores(landmarks, coeff, state, n_prbs, gamma, prec=240):
    """f(c) = sum_j coeff_j exp(-gamma |l_j - x_c|^2) for x_c = (float32 state, the double c / n_prbs), c = 0 .. n_prbs, in mpmath
    at `prec` bits (its exponent is unbounded: terms far below 5e-324 keep their value), with
    S(c) = sum_j |coeff_j| k_j(c), the scale of the forward error, and A(c) = sum_j |coeff_j| k_j(c) gamma |l_j - x_c|^2 / S(c),
    the S-weighted mean argument of the exponential (its condition number; 0 where S is 0).
    -> (f: list of mpf, S: longdouble array, A: float array)"""
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = prec
    co = np.asarray(coeff, dtype=np.float64)
    x = np.asarray(state, dtype=np.float32).astype(np.float64)
    m, d = len(co), len(x) + 1
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    tc = [mp.mpf(float(c) / float(n_prbs)) for c in range(n_prbs + 1)]
    g = mp.mpf(gamma)
    f = [mp.mpf(0) for _ in tc]
    last = {}   # exp(-gamma (lam - c/n)^2) per distinct last coordinate: k_j(c) = exp(-gamma D0_j) exp(-gamma dl^2) exactly
    for j in range(m):
        d0 = mp.mpf(0)
        for q in range(d - 1):
            t = mp.mpf(float(L[j, q])) - mp.mpf(float(x[q]))
            d0 += t * t
        w = mp.mpf(float(co[j])) * mp.exp(-g * d0)
        lam = float(L[j, d - 1])
        if lam not in last:
            last[lam] = [mp.exp(-g * (mp.mpf(lam) - t) ** 2) for t in tc]
        e2 = last[lam]
        for c in range(n_prbs + 1):
            f[c] += w * e2[c]
    # the scale and the mean argument need a wide exponent, not precision: longdouble (to 1e-4950)
    ld = np.longdouble
    S = np.zeros(n_prbs + 1, dtype=ld)
    A = np.zeros(n_prbs + 1)
    if m:
        Ll, xl = L.astype(ld), x.astype(ld)
        d0 = ((Ll[:, :d - 1] - xl[None, :]) ** 2).sum(axis=1)
        tcl = np.arange(n_prbs + 1, dtype=np.float64) / float(n_prbs)
        arg = ld(gamma) * (d0[:, None] + (Ll[:, d - 1:d] - tcl[None, :].astype(ld)) ** 2)
        k = np.abs(co).astype(ld)[:, None] * np.exp(-arg)
        S = k.sum(axis=0)
        with np.errstate(invalid='ignore', divide='ignore'):
            A = np.where(S > 0, (k * arg).sum(axis=0) / np.where(S > 0, S, 1), 0).astype(np.float64)
    return f, S, A


def bound_units(p_max, n_prbs, d, gamma, A, m, n_direct=0):
    """The forward bound of the documented order on |F(c) - f(c)| in units of u S(c), u = 2^-53 (first order in u, then through
    gamma_n = n u / (1 - n u)):   p_max + KA + c,   c = nseg - 1 + n_direct + 5 + 4 gamma + (d + 3) A(c).

    Every term coeff_j E_j G[|a_j - c|] of F(c) carries, relative to its own magnitude |coeff_j| k_j(c):
      * the sums.  Inside its bin the term goes through at most p_max - 1 additions of a segment and one addition per segment
        (nseg = ceil(m / 256)), then through at most KA fused multiply-adds of the chain and one more per landmark that takes
        the direct evaluation (n_direct), one rounding each:  p_max - 1 + nseg + KA + n_direct.
      * the roundings of the term itself (the constant 5): rs_exp is within 1.0 ulp <= 2 u (tests/test_primitives.py: ULP_BOUND),
        once for E_j and once for the table entry G; the product coeff_j E_j rounds once; the product G W inside the fma is
        exact.  A direct term has one exponential and no table entry: less.
      * the last coordinates (4 gamma): the candidate's and the landmark's are the DOUBLES c / n and a_j / n, whose difference
        is within 2 u of the k / n the table was built from: at most 4 gamma |dl| u <= 4 gamma u on the argument.
      * the argument of the exponentials ((d + 3) A).  t = l - x rounds once, t t once more, the d - 1 squares are added in
        order from zero (at most d - 2 roundings each) and gamma D0 rounds once: gamma D0 is within (d + 2) u of exact,
        relatively; the table's gamma (k / n)^2 within 4 u; the direct form gamma (D0 + dl^2) within (d + 3) u.  exp turns a
        relative error eps of its argument z into a relative error |z| eps of its value, so the term carries at most
        (d + 3) gamma |l_j - x_c|^2 u, and summed with the weights |coeff_j| k_j(c) that is (d + 3) A(c) u S(c), with A the
        S-weighted mean argument exact_scores returns.
    Terms that underflow -- E_j rounds to zero, or a direct exponential lands on a subnormal -- are wrong by at most a quantum
    2^-1074 times |coeff_j| each: the absolute term m 2^-1074 of `tolerance`, for coefficients of magnitude one as every
    insertion leaves them.  A candidate that keeps its binned sum (|F| >= 1e-240) leaves out terms below 1e-280 |coeff_j|
    each: 1e-40 of it."""
    KA = (n_prbs + 4) & ~3
    nseg = max(1, -(-m // (KB_BIN_SEG * KB_CH)))
    n = p_max - 1 + nseg + KA + n_direct + 5 + 4.0 * gamma + (d + 3) * np.asarray(A, dtype=np.float64)
    return n / (1.0 - n * U)


def issue_units(p_max, n_prbs):
    """the narrower constant p_max + KA + 5 that counts the sums and the roundings of a term only (no argument error of the
    exponentials: not a bound, see bound_units).  The tests print the measured error against it next to the bound's ratio."""
    n = p_max + ((n_prbs + 4) & ~3) + 5
    return n / (1.0 - n * U)


def tolerance(p_max, n_prbs, d, gamma, S, A, m, n_direct=0):
    """|F(c) - f(c)| <= bound_units u S(c) + m 2^-1074, as a longdouble array over the candidates"""
    ld = np.longdouble
    return bound_units(p_max, n_prbs, d, gamma, A, m, n_direct).astype(ld) * ld(U) * np.asarray(S, dtype=ld) + ld(m) * ld(TINY)


def errors(F, f_exact):
    """|F(c) - f(c)| as longdouble (the difference is formed in mpmath)"""
    import mpmath
    out = np.zeros(len(f_exact), dtype=np.longdouble)
    for c, fx in enumerate(f_exact):
        e = abs(mpmath.mpf(float(F[c])) - fx)
        mant, ex = mpmath.frexp(e)
        out[c] = np.ldexp(np.longdouble(float(mant)), int(ex)) if e != 0 else 0
    return out


def tolerance_single(S):
    """m == 1: the kernel value and the product are rounded to float32 (numpy's first arrays are float32: kernel.py:16,
    projectron.py:9): rs_exp's 2 u, then 2^-24 each for k, coeff and their product, and a float32 quantum 2^-149"""
    ld = np.longdouble
    return (ld(3 * 2.0 ** -24) + ld(2 * U)) * np.asarray(S, dtype=ld) + ld(2.0 ** -149)


# ------------------------------------------------------------------ test dictionaries
SPREAD = {10: 2.0, 3: 15.0}   # side of the cube the landmarks of a learner of that many state variables are drawn from, and
MIN_D2 = {10: 0.0, 3: 1.0}    # the least squared distance between two of them: neighbours stay far enough apart (gamma = 1) for
                              # every mistaken sample to be inserted (delta > eta = 0.1), and gamma D0 stays below 3 x 15^2 = 675 for
                              # a state inside the cube: every E_j is a normal number there


def random_samples(rng, count, dims, n_prbs, f32=True):
    """`count` distinct samples x = (state coordinates in [0, SPREAD]^dims, a / n_prbs); f32: the state coordinates are float32
    values (as observations are)"""
    side, d2 = SPREAD.get(dims, 2.0), MIN_D2.get(dims, 0.0)
    X = np.zeros((count, dims + 1))
    n = 0
    while n < count:
        x = rng.uniform(0.0, side, dims)
        if f32:
            x = x.astype(np.float32).astype(np.float64)
        if d2 > 0.0 and n and ((X[:n, :dims] - x) ** 2).sum(axis=1).min() < d2:
            continue
        X[n, :dims] = x
        n += 1
    X[:, -1] = rng.integers(0, n_prbs + 1, count).astype(np.float64) / float(n_prbs)
    return X


def grow(m, X, predict, update, size, off_grid=(), rng=None):
    """Teacher-forced growth to exactly m landmarks: the samples X in order with alternating labels through predict(x) /
    update(x, y) -> branch, until size() == m.  A sample the learner already classifies as its label says changes nothing; every
    other one must be inserted (branch 2).  The landmarks whose index is in `off_grid` get a last coordinate off the candidate
    grid (a draw of `rng`)."""
    i = 0
    while size() < m:
        x = X[i].copy()
        if size() in off_grid:
            x[-1] = rng.uniform(0.0, 1.0)
        predict(x)
        br = update(x, 1 if i % 2 == 0 else -1)
        assert br in (0, 2), 'sample %d was projected (branch %d): the samples are too close for eta' % (i, br)
        i += 1


def far_state(dims, value):
    """a state every coordinate of which is `value`: 60 and beyond is where every E_j of SPREAD's landmarks underflows"""
    return np.full(dims, value, dtype=np.float32)


def band_coordinate(L, gamma=1.0, level=715.0):
    """v such that the state (v, ..., v), as float32, has gamma D0 >= `level` for every landmark (rows of L: the state
    coordinates) and below level + 3 for the nearest: that one -- and whoever else is below 744.4 -- has E_j between 1e-300 and
    5e-324, the middle of the band; everybody further away underflows to zero"""
    L = np.asarray(L, dtype=np.float64)
    for v in np.arange(float(L.max()), float(L.max()) + 80.0, 0.005):
        x = np.float64(np.float32(v))
        if gamma * ((L - x) ** 2).sum(axis=1).min() >= level:
            return float(np.float32(v))
    raise AssertionError('no band state')
