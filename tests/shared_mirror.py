"""A plain restatement of the shared-dictionary learning step as the device forms it (csrc/kb_kbrl.hip: shared_q_kernel,
shared_fgemm_kernel, shared_scan_kernel, shared_collect_kernel, shared_commit_kernel, shared_cols_kernel, shared_matvec_kernel /
shared_matvec_mfma_kernel, shared_gram_kernel, apply_full_batch, shared_apply_kernel), sum by sum in the order the kernels' code
states, and the exact values it approximates.  Used by tests/test_shared_mirror.py (CPU) and tests/test_gpu_shared_chain.py
(device).  Not a test module.  The fused multiply-add, rs_exp and rs_exp_nonpos come from the oracle's library
(oracle.pyoracle.detmath: the bits tests/test_gpu_primitives.py pins the device to); the helpers are those of
tests/scoring_mirror.py (sm) and tests/update_mirror.py (um).

THE SCORES OF A LARGE DICTIONARY (m >= KB_GEMM_M = 256, every landmark on the candidate grid), gemm_scores: for replica r with the
float32 state x_r, landmarks l_j (grid index a_j), coefficients coeff_j and candidates c = 0 .. n_prbs

  E         D0_rj = the squares (l_jq - x_rq)^2 of the state coordinates q = 0 .. d - 2 added in order from 0.0 (difference, product
            and sum each rounded); E_rj = rs_exp_nonpos(-gamma D0_rj)                                   [shared_fgemm_kernel]
  Q         Q[j][c] = coeff_j G[min(|a_j - c|, 255)], ONE rounded product, G = sm.gtable                [shared_q_kernel]
  parts     the landmarks in slabs of four, nk = ceil(m / 4) slabs, per = ceil(nk / 8) slabs a part: part kp = 0 .. 7 holds the
            slabs [kp per, min((kp + 1) per, nk)), that is the landmarks 4 kp per <= j < min(4 (kp + 1) per, 4 nk), j < m.  A part
            may be empty (m = 257: nk = 65, per = 9, part 7 starts at slab 63 and holds two; m = 260 .. 288: per = 9, part 7 is
            short or just full) and the last slab may be padded (m mod 4 != 0).
  partial   P_kp[r][c] = ONE chain acc <- fma(E_rj, Q[j][c], acc) from 0.0 over the part's landmarks in increasing j: what
            consecutive v_mfma_f64_16x16x4 on one accumulator form (tools/experiments/mfma_order.hip; sm.chain relies on the same).
            Padding landmarks (j >= m, and the second slab of a trip of two past the part's end) are fma(0.0, 0.0, acc): they can
            only turn an accumulator of -0.0 into +0.0, so zeros of either sign count as equal, as in tests/test_gpu_scoring.py.
  emax      emax_kp[r] = the largest E_rj of the part, from 0.0 (an empty part: 0.0)
  F         F[r][c] = ((P0 + P1) + (P2 + P3)) + ((P4 + P5) + (P6 + P7))                                 [shared_scan_kernel]
  fallback  a replica whose max_kp emax_kp < 1e-250 takes the streaming pass (the per-replica scoring chain, sm.ordered_scores);
            so does every replica of a dictionary below 256 landmarks or with a landmark off the grid.

THE SCAN, scan(): the augmentation range of the step is [a_i, n_prbs] after y = +1 and [0, a_i] after y = -1; round 0 starts at its
first candidate, a later round at the replica's cursor (a cursor outside [0, c_to]: nothing left, cstar = cursor = -1); cstar = the
first candidate of the range with f y <= 0, else -1, and the cursor STAYS on cstar until the commit.  Round 0 also says
hit = (y == sign f(a_i)) (an empty dictionary predicts 0: no hit; f(a_i) == 0.0 of a filled one draws, which the tests avoid).
collect(): per slice the proposers (cstar >= 0) in replica order, the first `budget` of them become the list, counts = ALL
proposers; the proposal is (global replica id, the word c 4 + (y == 1), the float32 state as doubles).  commit(): the first
`taken` proposers of the slice, in replica order, move their cursor to cstar + 1; the others keep it (and propose the same
candidate again).

THE APPLY OF A FULL DICTIONARY (m >= capacity, m >= 2), full_batch(): nothing but the coefficients changes, so for the whole list

  KF        KF[p] = um.column(landmarks, (x_p, c_p / n_prbs), gamma): kernel_column_full's arithmetic        [shared_cols_kernel]
  DS        DS[p] = um.dstar_col(Kinv, KF[p]): the column walk's eight chains and tree; shared_matvec_kernel forms them lane
            by lane, shared_matvec_mfma_kernel (capacities that are multiples of 64) on the matrix cores -- both claim these bits
  F0        F0[p] = um.dot(KF[p], coeff_0): 256 strided sums, butterfly, four totals                         [shared_gram_kernel]
  A         A[p][q] = k_p . d*_q as ONE chain acc <- fma(KF[p][k], DS[q][k], acc) from 0.0 in the order k0 = 0, 32, ..; h = 0, 1;
            u = 0 .. 3; kq = 0 .. 3 with k = k0 + 16 h + u + 4 kq (a lane keeps four consecutive doubles of a 16-landmark slab and
            MFMA step u contracts the lanes' u-th); k >= m: fma(0.0, 0.0, acc).  Only the 16 x 16 tiles t_j <= t_i of the lower
            block triangle are formed (p >> 4 >= q >> 4); the device stores A by column.                     [shared_gram_kernel]
  walk      g_p = 0.0; in list order: f_p = F0[p] + g_p (one rounded sum); applied iff f_p y_p <= 0; then for every LATER p' > p:
            g_p' <- fma(y_p, A[p'][p], g_p').  The saturation flag (error bit 8) is raised when an applied proposal has
            max(1 - A[p][p], 0) > eta.                                                                       [apply_full_batch]
  coeff     coeff_j <- coeff_j + y_q DS[q][j] over the applied q in list order (y_q = +-1: the product is exact; the sum rounds)

growing_apply(): a dictionary below its capacity takes the list one by one: f = um.score(um.column(..), coeff) (predict_column's
sum; 0.0 when empty, float32 while one landmark is held), and where f y <= 0 um.step(.., order='col'): Projectron.update with d* by
the column walk, which is what a handle that stores both triangles of Kinv runs.  A dictionary that reaches its capacity inside a
list goes on projecting through the same path.

BOUNDS, in units of u = 2^-53, for the inputs as the doubles they are, derived as sm.bound_units and um.bound_units are:

  bound_units (scores): every term coeff_j E_rj G[|a_j - c|] of F[r][c] carries, relative to its own magnitude,
      * the exponentials at the 1.0 ulp <= 2 u tests/test_primitives.py asserts, E and G:                          4
      * the product Q = coeff G:                                                                                   1
      * the chain of its part: at most 4 per fused multiply-adds, one rounding each (the product inside is exact)  4 per
      * the tree of eight partial sums, three additions deep:                                                      3
      * the last coordinates: the doubles c / n and a_j / n differ from the k / n of the table by 2 u at most:     4 gamma
      * the argument of E and of G, as in sm.bound_units:                                                          (d + 3) A(c)
    n = 4 per + 8 + 4 gamma + (d + 3) A(c), through gamma_n = n u / (1 - n u), times S(c) = sum_j |coeff_j| k_j(c), plus
    m 2^-1074 max(1, |coeff|_max) for the E_rj that underflow.
  gram_units (A): with B = um.bound_units(m, 'col') for DS, T_pq = sum_k |KF[p][k]| S_qk (S_qk = sum_j |Kinv_kj| |KF[q][j]| the
    scale of d*_qk): the chain has n_A = 32 ceil(m / 32) roundings and is formed of DS, not d*:
      |A^_pq - k_p . d*_q| <= (B + n_A (1 + B u)) u T_pq
  f_p: F0 within um.f_units(m) u sum_j |KF[p][j] coeff_0j|; g_p a chain of n_p fused multiply-adds over the n_p applied q < p:
      E_g = sum_q E_A(p, q) + n_p u sum_q (|A_pq| + E_A(p, q)), and the final sum rounds once:
      |f^_p - f_p| <= E_F0 + E_g + u (|f_p| + E_F0 + E_g)
  The exact companions of the apply (exact_full_batch) are in longdouble, as um.exact_step is: every bound takes
  um.exact_units(m) on top of B, n_A and F, and u (1 + 2^-10) for u.  The exact scores (exact_scores) are in mpmath at 240 bits.
"""
import numpy as np

import scoring_mirror as sm
import update_mirror as um

KB_GEMM_M = 256
KB_GEMM_KS = 8
KB_E_FALLBACK = 1e-250
U = 2.0 ** -53
TINY = 2.0 ** -1074


def _po():
    from oracle import pyoracle as po
    return po


def gemm_applies(m, idx):
    return m >= KB_GEMM_M and not (np.asarray(idx)[:m] < 0).any()


def part_ranges(m, ks=KB_GEMM_KS):
    """[(j_lo, j_hi)] of the ks parts: landmarks j_lo <= j < j_hi (j_hi may pass m by the last slab's padding)"""
    nk = (m + 3) >> 2
    per = (nk + ks - 1) // ks
    return [(4 * min(kp * per, nk), 4 * min((kp + 1) * per, nk)) for kp in range(ks)], per


def e_rows(landmarks, states, gamma):
    """E [N, m] = rs_exp_nonpos(-gamma D0), D0 in coordinate order (and D0 itself)"""
    L = np.asarray(landmarks, dtype=np.float64)
    X = np.atleast_2d(np.asarray(states, dtype=np.float32)).astype(np.float64)
    d0 = np.zeros((len(X), len(L)))
    for q in range(L.shape[1] - 1):
        t = L[None, :, q] - X[:, q, None]
        d0 = d0 + t * t
    E = _po().detmath('EXP_NONPOS', (-gamma * d0).ravel()).reshape(d0.shape)
    return E, d0


def q_table(coeff, idx, G, n_prbs):
    """Q [m, n_prbs + 1]"""
    a = np.asarray(idx, dtype=np.int64)
    o = np.minimum(np.abs(a[:, None] - np.arange(n_prbs + 1)[None, :]), 255)
    return np.asarray(coeff, dtype=np.float64)[:, None] * np.asarray(G, dtype=np.float64)[o]


def gemm_scores(landmarks, coeff, idx, state_f32, G, n_prbs, gamma, m=None, ks=KB_GEMM_KS, linear_tree=False):
    """-> dict(parts [ks, N, n_prbs + 1], F [N, n_prbs + 1], emax [ks, N], E [N, m]).  ks = 7 and linear_tree are deliberately WRONG
    orders for the tests of the tests (ks != 8: the tree is then a plain chain over the parts)"""
    m = len(coeff) if m is None else m
    L = np.asarray(landmarks, dtype=np.float64)[:m]
    E, _ = e_rows(L, state_f32, gamma)
    Q = q_table(np.asarray(coeff)[:m], np.asarray(idx)[:m], G, n_prbs)
    N, C = E.shape[0], n_prbs + 1
    ranges, per = part_ranges(m, ks)
    parts, emax = np.zeros((ks, N, C)), np.zeros((ks, N))
    for kp, (lo, hi) in enumerate(ranges):
        acc = np.zeros((N, C))
        for j in range(lo, min(hi, m)):
            acc = um.fma(E[:, j, None], Q[None, j, :], acc)
        parts[kp] = acc + 0.0      # (-0.0 -> +0.0: what a padding term does, and equal as a value anyway)
        if min(hi, m) > lo:
            emax[kp] = np.maximum(E[:, lo:min(hi, m)].max(axis=1), 0.0)
    F = um.tree8(parts, linear_tree) if ks == 8 else um.tree8(np.concatenate([parts, np.zeros((8 - ks, N, C))]), True)
    return dict(parts=parts, F=F, emax=emax, E=E, per=per)


def takes_product(emax):
    """per replica: the scan reads the product's scores (else the streaming pass)"""
    return np.asarray(emax).max(axis=0) >= KB_E_FALLBACK


# ------------------------------------------------------------------ scan, collect, commit
def scan(f, y, a_i, cursor, rnd, n_prbs, m=1):
    """f: the scores of candidates 0 .. n_prbs (any sequence of numbers: doubles, or exact values) -> dict(cstar, cursor, hit);
    hit is None past round 0"""
    c_to = n_prbs if y == 1 else a_i
    c_from = (a_i if y == 1 else 0) if rnd == 0 else cursor
    hit = None
    if rnd == 0:
        f0 = f[a_i] if m > 0 else 0
        assert m == 0 or f0 != 0, 'f(a_i) == 0 draws from the tie-break stream: not a case of these tests'
        hit = int(m > 0 and (1 if f0 > 0 else -1) == y)
    elif not (0 <= c_from <= c_to):
        return dict(cstar=-1, cursor=-1, hit=None)
    cstar = -1
    for c in range(c_from, c_to + 1):
        if f[c] * y <= 0:
            cstar = c
            break
    return dict(cstar=cstar, cursor=cstar if cstar >= 0 else -1, hit=hit)


def proposal_word(c, y):
    return float(c * 4 + (1 if y == 1 else 0))


def collect(cstar, budget, states=None, labels=None, first_env=0, offsets=None, dims=None):
    """cstar [N, S] -> (counts [S], lists: per slice the (replica, candidate) pairs of the first `budget` proposers in replica
    order); with states / labels / offsets / dims also props [S, budget, 18] as the device lays them out"""
    cstar = np.asarray(cstar)
    N, S = cstar.shape
    counts = np.array([int((cstar[:, s] >= 0).sum()) for s in range(S)], dtype=np.int32)
    lists = [[(e, int(cstar[e, s])) for e in range(N) if cstar[e, s] >= 0][:budget] for s in range(S)]
    if states is None:
        return counts, lists
    props = np.zeros((S, budget, 18))
    for s in range(S):
        for i, (e, c) in enumerate(lists[s]):
            props[s, i, 0] = first_env + e
            props[s, i, 1] = proposal_word(c, labels[e, s])
            props[s, i, 2:2 + dims[s]] = np.asarray(states, dtype=np.float32)[e, offsets[s]:offsets[s] + dims[s]]
    return counts, lists, props


def commit(cstar, taken, cursor):
    """the first taken[s] proposers of slice s, in replica order, move past their candidate -> the new cursors [N, S]"""
    cstar, cursor = np.asarray(cstar), np.array(cursor, copy=True)
    for s in range(cstar.shape[1]):
        left = int(taken[s])
        for e in range(cstar.shape[0]):
            if cstar[e, s] >= 0:
                if left > 0:
                    cursor[e, s] = cstar[e, s] + 1
                left -= 1
    return cursor


def unpack(props, count, d, n_prbs):
    """the first `count` proposals of one slice's list -> (X [count, d] = state and c / n_prbs, y [count], c [count], ids)"""
    P = np.asarray(props, dtype=np.float64)[:count]
    w = P[:, 1].astype(np.int64)
    c, y = w >> 2, np.where(w & 1, 1, -1)
    X = np.column_stack([P[:, 2:2 + d - 1], c.astype(np.float64) / float(n_prbs)]) if count else np.zeros((0, d))
    return X, y, c, P[:, 0].astype(np.int64)


# ------------------------------------------------------------------ the apply
def gram(KF, DS, m, plain_k=False):
    """A [np, np] = KF DS^T, every entry ONE chain in shared_gram_kernel's contraction order (plain_k: increasing k, a contrasting
    order).  All entries are formed; the device forms those with p >> 4 >= q >> 4 (lower_tiles)."""
    KF, DS = np.asarray(KF, dtype=np.float64), np.asarray(DS, dtype=np.float64)
    n = len(KF)
    mp = (m + 31) // 32 * 32
    a, b = np.zeros((n, mp)), np.zeros((n, mp))
    a[:, :m], b[:, :m] = KF[:, :m], DS[:, :m]
    if plain_k:
        order = list(range(mp))
    else:
        order = [k0 + 16 * h + u + 4 * kq for k0 in range(0, mp, 32) for h in range(2) for u in range(4) for kq in range(4)]
    acc = np.zeros((n, n))
    for k in order:
        acc = um.fma(a[:, k, None], b[None, :, k], acc)
    return acc + 0.0


def lower_tiles(n):
    p = np.arange(n)
    return (p[:, None] >> 4) >= (p[None, :] >> 4)


def full_batch(Kinv, coeff, landmarks, props, gamma, n_prbs, eta=0.1, count=None, plain_k=False, fresh_dot=False):
    """the list `props` ([np, 18] rows of one slice) applied to a dictionary at its capacity -> dict(KF, DS, F0, A, f [np] = the f_p
    the walk decided on, applied [np] bool, n_mist, sat, coeff).  plain_k / fresh_dot: deliberately OTHER orders for the tests of the
    tests (A summed in increasing k; the walk forming f_p = um.dot(KF[p], the coefficients as they stand) afresh)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    m = len(coeff)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, -1)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    n = len(props) if count is None else count
    X, y, _, _ = unpack(props, n, L.shape[1], n_prbs)
    KF = np.stack([um.column(L, x, gamma) for x in X]) if n else np.zeros((0, m))
    DS = np.stack([um.dstar_col(Kinv, k) for k in KF]) if n else np.zeros((0, m))
    F0 = np.array([um.dot(k, coeff) for k in KF])
    A = gram(KF, DS, m, plain_k) if n else np.zeros((0, 0))
    g, f = np.zeros(n), np.zeros(n)
    applied = np.zeros(n, dtype=bool)
    c = coeff.copy()
    sat = False
    for p in range(n):
        f[p] = um.dot(KF[p], c) if fresh_dot else F0[p] + g[p]
        if f[p] * y[p] <= 0.0:
            applied[p] = True
            delta = 1.0 - A[p, p]
            sat = sat or (delta if delta > 0.0 else 0.0) > eta
            if p + 1 < n:
                g[p + 1:] = um.fma(float(y[p]), A[p + 1:, p], g[p + 1:])
            c = c + float(y[p]) * DS[p]
    return dict(KF=KF, DS=DS, F0=F0, A=A, f=f, applied=applied, n_mist=int(applied.sum()), sat=bool(sat), coeff=c, y=y)


def growing_apply(Kinv, coeff, landmarks, props, gamma, n_prbs, d, eta=0.1, capacity=None, count=None):
    """the list applied one by one to a dictionary of samples of d coordinates that can still grow -> dict(f [np], applied [np],
    branch [np] (0: no mistake), kinv, coeff, landmarks, m)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    m = len(coeff)
    n = len(props) if count is None else count
    P = np.asarray(props, dtype=np.float64)
    f, applied, branch = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    for p in range(n):
        w = int(P[p, 1])
        y = 1 if w & 1 else -1
        x = np.append(P[p, 2:2 + d - 1], float(w >> 2) / float(n_prbs))
        f[p] = um.score(um.column(L, x, gamma), coeff) if len(coeff) else 0.0
        if f[p] * y <= 0.0:
            st = um.step(Kinv, coeff, L, x, y, gamma, eta, capacity, order='col')
            applied[p], branch[p] = True, st['branch']
            Kinv, coeff, L = st['kinv'], st['coeff'], st['landmarks']
    return dict(f=f, applied=applied, branch=branch, kinv=Kinv, coeff=coeff, landmarks=L, m=len(coeff))


# ------------------------------------------------------------------ exact companions and bounds
_pair_cache = {}


def _mp():
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = 240
    return mp


def _pair_table(n_prbs, gamma, bins):
    """exp(-gamma (lam - c / n)^2) of the DOUBLES lam and c / n as integers scaled by 2^300, per last coordinate lam of `bins`"""
    mp = _mp()
    tab = _pair_cache.setdefault((n_prbs, float(gamma)), {})
    tc = None
    for a in bins:
        if a not in tab:
            if tc is None:
                tc = [mp.mpf(float(c) / float(n_prbs)) for c in range(n_prbs + 1)]
            la = mp.mpf(float(a))
            g = mp.mpf(gamma)
            tab[a] = [int(mp.ldexp(mp.exp(-g * (la - t) ** 2), 300)) for t in tc]
    return tab


def exact_scores(landmarks, coeff, idx, state, n_prbs, gamma):
    """f(c), S(c), A(c) as sm.exact_scores returns them (f: list of mpf at 240 bits), for a dictionary on the candidate grid, in a
    form that costs m exponentials and one integer product sum per candidate: the exact D0_j from the coordinates as integers,
    w_j = coeff_j exp(-gamma D0_j) in mpmath, summed per grid index, scaled by the largest bin to integers of 300 bits and
    multiplied with the table exp(-gamma (lam - c / n)^2) of the doubles lam, c / n (300 bits).  Both truncations are 2^-300 of
    the largest bin, which is at most e^gamma S(c) away: f is exact to 2^-290 S(c).  The bins are the distinct last coordinates
    themselves (a landmark on the grid holds the double a / n), so a landmark off the grid is one more bin; idx is not used."""
    mp = _mp()
    co = np.asarray(coeff, dtype=np.float64)
    x = np.asarray(state, dtype=np.float32).astype(np.float64)
    m, d = len(co), len(x) + 1
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    # the coordinates as integers of one scale (they are float32 values, or doubles of a few bits: the scale is found, not assumed)
    vals = np.concatenate([L[:, :d - 1].ravel(), x])
    nz = vals[vals != 0]
    sh = 0 if nz.size == 0 else int(max(0, 53 - np.frexp(np.abs(nz))[1].min()))
    assert sh < 900
    toint = lambda v: int(np.ldexp(v, sh)) if sh < 1000 else 0
    Li = np.array([[toint(v) for v in row] for row in L[:, :d - 1]], dtype=object).reshape(m, d - 1)
    xi = np.array([toint(v) for v in x], dtype=object)
    assert all(float(np.ldexp(float(Li[j, q]), -sh)) == L[j, q] for j in range(min(m, 4)) for q in range(d - 1))
    d0i = ((Li - xi[None, :]) ** 2).sum(axis=1) if m else []
    g = mp.mpf(gamma)
    bins = {}
    for j in range(m):
        w = mp.mpf(float(co[j])) * mp.exp(-g * mp.ldexp(mp.mpf(int(d0i[j])), -2 * sh))
        a = float(L[j, d - 1])
        bins[a] = bins.get(a, mp.mpf(0)) + w
    f = [mp.mpf(0)] * (n_prbs + 1)
    big = max((abs(w) for w in bins.values()), default=mp.mpf(0))
    if big != 0:
        _, ex = mp.frexp(big)
        tab = _pair_table(n_prbs, gamma, sorted(bins))
        wi = {a: int(mp.ldexp(w, 300 - int(ex))) for a, w in bins.items()}
        for c in range(n_prbs + 1):
            f[c] = mp.ldexp(mp.mpf(sum(w * tab[a][c] for a, w in wi.items())), int(ex) - 600)
    ld = np.longdouble
    S, A = np.zeros(n_prbs + 1, dtype=ld), np.zeros(n_prbs + 1)
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


def bound_units(m, d, gamma, A):
    """the forward bound of gemm_scores' F in units of u S(c) (the module docstring derives it)"""
    _, per = part_ranges(m)
    n = 4 * per + 8 + 4.0 * gamma + (d + 3) * np.asarray(A, dtype=np.float64)
    return n / (1.0 - n * U)


def tolerance(m, d, gamma, S, A, coeff_max=1.0):
    ld = np.longdouble
    return bound_units(m, d, gamma, A).astype(ld) * ld(U) * np.asarray(S, dtype=ld) + ld(m) * ld(TINY) * ld(max(1.0, coeff_max))


def streaming_tolerance(landmarks, coeff, idx, state, n_prbs, gamma, S, A):
    """the bound of the per-replica scoring chain (sm.tolerance) for one replica that takes the streaming pass"""
    m = len(coeff)
    d0, E, _, _ = sm.rows(landmarks, state, n_prbs, gamma)
    _, p_max = sm.bin_sums(E, idx, coeff)
    nd = int(sm.direct_mask(E, idx).sum())
    d = np.asarray(landmarks).shape[1]
    cm = max(1.0, float(np.abs(coeff).max())) if m else 1.0
    return sm.tolerance(max(p_max, 1), n_prbs, d, gamma, S, A, m, nd) * np.longdouble(cm)


def open_candidates(f_exact, tol):
    """candidates whose exact |f| does not exceed the bound: the sign the device decides on is not determined"""
    return np.array([abs(f) <= t for f, t in zip(f_exact, (sm_float(t) for t in tol))])


def sm_float(t):
    import mpmath
    m, e = np.frexp(t)
    return mpmath.ldexp(mpmath.mpf(float(m)), int(e))


def gram_units(m):
    """(B, n_A): the units of d* (column walk) and the number of roundings of A's chain, exact_units included"""
    return um.bound_units(m, 'col') + um.exact_units(m), 32 * ((m + 31) // 32) + um.exact_units(m)


def exact_full_batch(Kinv, coeff, KF, y):
    """the list's walk of the SAME doubles (Kinv, the kernel columns KF, the coefficients, the labels) in longdouble -> dict(ds [np, m],
    S [np, m], A [np, np], EA [np, np] = the bound of the device's A, f [np], Ef [np] = the bound of the device's f_p, applied [np],
    coeff [m], open [np] = |f_p| <= Ef_p: from the first open proposal on the applied sets need not agree)"""
    ld = np.longdouble
    KF = np.asarray(KF, dtype=np.float64)
    n, m = KF.shape
    ue = ld(U * (1.0 + 2.0 ** -10))
    B, nA = gram_units(m)
    F = um.f_units(m) + um.exact_units(m)
    Kl = np.asarray(Kinv, dtype=np.float64).astype(ld)
    kl = KF.astype(ld)
    ds = np.stack([(Kl * kl[p][None, :]).sum(axis=1) for p in range(n)])
    S = np.stack([np.abs(Kl * kl[p][None, :]).sum(axis=1) for p in range(n)])
    A = kl @ ds.T                      # A[p][q] = k_p . d*_q
    T = np.abs(kl) @ S.T
    EA = (ld(B) + ld(nA) * (1 + ld(B) * ue)) * ue * T
    c0 = np.asarray(coeff, dtype=np.float64).astype(ld)
    f0 = kl @ c0
    E0 = ld(F) * ue * (np.abs(kl) @ np.abs(c0))
    f, Ef = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    applied, opened = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    c = c0.copy()
    for p in range(n):
        q = np.nonzero(applied[:p])[0]
        g = (np.asarray(y)[q].astype(ld) * A[p, q]).sum()
        Eg = EA[p, q].sum() + ld(len(q)) * ue * (np.abs(A[p, q]) + EA[p, q]).sum()
        f[p] = f0[p] + g
        Ef[p] = E0[p] + Eg + ue * (abs(f[p]) + E0[p] + Eg)
        opened[p] = abs(f[p]) <= Ef[p]
        if f[p] * ld(int(y[p])) <= 0:
            applied[p] = True
            c = c + ld(int(y[p])) * ds[p]
    return dict(ds=ds, S=S, A=A, EA=EA, f=f, Ef=Ef, applied=applied, coeff=c, open=opened)


# ------------------------------------------------------------------ the sequential oracle beside a step's rounds
def plain_scores(landmarks, coeff, state, n_prbs, gamma):
    """f(c) of candidates 0 .. n_prbs in plain float64 (numpy's exp and sums) and the scale sum_j |k_j(c) coeff_j|: decisions taken
    from it hold where |f| > 1e-9 (1 + scale), the teacher-forced tolerance of DESIGN.md section 2"""
    co = np.asarray(coeff, dtype=np.float64)
    m = len(co)
    if m == 0:
        return np.zeros(n_prbs + 1), np.zeros(n_prbs + 1)
    x = np.asarray(state, dtype=np.float32).astype(np.float64)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, len(x) + 1)
    d0 = ((L[:, :-1] - x[None, :]) ** 2).sum(axis=1)
    tc = np.arange(n_prbs + 1, dtype=np.float64) / float(n_prbs)
    k = np.exp(-gamma * (d0[:, None] + (L[:, -1:] - tc[None, :]) ** 2))
    return co @ k, np.abs(co) @ k


class OracleRounds:
    """ONE oracle learner per slice beside the rounds of a shared step: the scan is taken from the learners' dictionaries as they
    stand (plain_scores), the merged lists are fed in order through predict and, when mistaken, update -- what kb_kbrl.hip says
    the shared step is.  `open` counts the (replica, slice) pairs a scan left out because a candidate at or before the first
    mistake scored within 1e-9 (1 + scale) of zero (an empty dictionary scores exactly 0.0: every candidate is a mistake)."""

    def __init__(self, dims, n_prbs, n_envs, gamma, eta, capacity):
        po = _po()
        self.dims, self.n_prbs, self.N, self.gamma = list(dims), n_prbs, n_envs, gamma
        self.off = np.cumsum([0] + self.dims)[:-1]
        self.oa = [po.OracleKBRL([d], n_prbs, [0], [1], gamma=gamma, eta=eta, capacity=capacity) for d in dims]
        for o in self.oa:
            o.set_seed(0)
        self.open = 0
        self.pairs = 0

    def begin(self, states, actions, labels):
        self.states = np.asarray(states, dtype=np.float32)
        self.actions, self.labels = np.asarray(actions), np.asarray(labels)
        self.cursor = np.zeros((self.N, len(self.dims)), dtype=np.int64)
        self.round = 0

    def scan(self):
        """-> (cstar [N, S], hits [N, S] (round 0; else None), left_out [N, S] bool); self.n_pred = the predictions the scan makes as
        the device counts them: one for the hit of round 0 and one per candidate from the start to the proposal (or the range's end)"""
        self.n_pred = 0
        S = len(self.dims)
        cstar = np.full((self.N, S), -1, dtype=np.int64)
        hits = np.zeros((self.N, S), dtype=np.int64) if self.round == 0 else None
        out = np.zeros((self.N, S), dtype=bool)
        for s in range(S):
            o = self.oa[s]
            m = o.m(0)
            L, co = (o.landmarks(0), o.coeff(0)) if m else (np.zeros((0, self.dims[s] + 1)), np.zeros(0))
            for e in range(self.N):
                x = self.states[e, self.off[s]:self.off[s] + self.dims[s]]
                f, sc = plain_scores(L, co, x, self.n_prbs, self.gamma)
                y, a_i = int(self.labels[e, s]), int(self.actions[e, s])
                c_from = (a_i if y == 1 else 0) if self.round == 0 else int(self.cursor[e, s])
                r = scan(f, y, a_i, int(self.cursor[e, s]), self.round, self.n_prbs, m)
                cstar[e, s], self.cursor[e, s] = r['cstar'], r['cursor']
                c_to = self.n_prbs if y == 1 else a_i
                if 0 <= c_from <= c_to:
                    self.n_pred += (r['cstar'] if r['cstar'] >= 0 else c_to) - c_from + 1
                if self.round == 0:
                    hits[e, s] = r['hit']
                    self.n_pred += 1
                if m and (self.round == 0 or 0 <= c_from <= (self.n_prbs if y == 1 else a_i)):
                    near =np.abs(f) <= 1e-9 * (1.0 + sc)
                    last = r['cstar'] if r['cstar'] >= 0 else (self.n_prbs if y == 1 else a_i)
                    out[e, s] = bool(near[max(c_from, 0):last + 1].any()) or (self.round == 0 and bool(near[a_i]))
                self.pairs += 1
        self.open += int(out.sum())
        self.cstar = cstar
        return cstar, hits, out

    def apply(self, lists):
        """lists: per slice [(replica, candidate)] in order -> per slice [(f, applied, branch)]"""
        res = []
        for s, lst in enumerate(lists):
            o, rows = self.oa[s], []
            for e, c in lst:
                x = np.append(self.states[e, self.off[s]:self.off[s] + self.dims[s]].astype(np.float64), float(c) / float(self.n_prbs))
                y = int(self.labels[e, s])
                f = o.predict(0, x)[1]       # (the empty dictionary answers 0.0; update takes the column predict left)
                br = o.update(0, x, y)[0] if f * y <= 0 else 0
                rows.append((f, f * y <= 0, br))
            res.append(rows)
        return res

    def commit(self, taken):
        self.cursor = commit(self.cstar, taken, self.cursor)
        self.round += 1


# ------------------------------------------------------------------ the inputs of the tests (CPU and device use the same)
GEMM_SIZES = [255, 256, 257, 259, 260, 288, 320, 513]
FULL_CASES = [    # (capacity, proposals, kind): the column walk at 2, 63, 65; the matrix cores from 64 on, nine blocks at 576
    (2, 1, 'none'), (63, 15, 'stop'), (65, 17, 'none'), (64, 16, 'stop'), (128, 64, 'none'), (256, 256, 'stop'), (320, 65, 'stop'),
    (576, 17, 'none')]


def stream(dims, n_prbs, count, seed):
    """ONE sample stream per (dims, n_prbs): sm.random_samples, float32 states, allocations on the grid; sm.grow's alternating labels"""
    X = sm.random_samples(np.random.default_rng(seed), count, dims, n_prbs)
    return X, np.where(np.arange(count) % 2 == 0, 1, -1)


def oracle_trace(dims, n_prbs, count, seed, capacity, gamma=1.0, eta=0.1, off_grid=None):
    """ONE oracle learner teacher-forced along stream() -> (the learner, X, Y, m_after [count] = its size after every sample,
    branch [count]).  off_grid: from this sample on, the first one the learner gets wrong has its allocation moved off the candidate
    grid (X holds it)."""
    po = _po()
    X, Y = stream(dims, n_prbs, count, seed)
    oa = po.OracleKBRL([dims], n_prbs, [0], [1], gamma=gamma, eta=eta, capacity=capacity)
    oa.set_seed(0)
    m_after, branch = np.zeros(count, dtype=np.int64), np.zeros(count, dtype=np.int64)
    for i in range(count):
        if off_grid is not None and i >= off_grid:       # the first sample from there on that the learner gets wrong
            xt = X[i].copy()
            xt[-1] = 0.4321
            if oa.predict(0, xt)[1] * Y[i] <= 0:
                X[i], off_grid = xt, None
        if oa.predict(0, X[i])[1] * Y[i] <= 0:
            branch[i] = oa.update(0, X[i], int(Y[i]))[0]
        m_after[i] = oa.m(0)
        if m_after[i] >= capacity:
            m_after[i + 1:], count = m_after[i], i + 1
            break
    return oa, X, Y, m_after, branch


def prefix_for(m_after, m):
    """samples of the stream after which the dictionary first holds m landmarks"""
    at = np.nonzero(np.asarray(m_after) == m)[0]
    assert at.size, 'the stream never holds %d landmarks' % m
    return int(at[0]) + 1


def oracle_grown(dims, n_prbs, sizes, seed, gamma=1.0, eta=0.1):
    """{m: (Kinv, coeff, landmarks)} of ONE oracle learner teacher-forced along stream(): every sample it gets wrong is inserted
    (sm.SPREAD keeps the samples apart), so the dictionary passes every size; -> (dict, samples used per size)"""
    po = _po()
    X, Y = stream(dims, n_prbs, 2 * max(sizes) + 64, seed)
    oa = po.OracleKBRL([dims], n_prbs, [0], [1], gamma=gamma, eta=eta, capacity=max(sizes) + 8)
    oa.set_seed(0)
    out, used, i = {}, {}, 0
    for m in sorted(sizes):
        while oa.m(0) < m:
            f = oa.predict(0, X[i])[1]
            if f * Y[i] <= 0:
                assert oa.update(0, X[i], int(Y[i]))[0] == 2, 'sample %d was projected' % i
            i += 1
        out[m], used[m] = (oa.kinv(0), oa.coeff(0), oa.landmarks(0)), i
    return out, used


def replica_states(landmarks, n, seed, far=None):
    """n float32 states: landmarks' own states moved by up to 0.05 a coordinate (even replicas) and draws from the cube (odd
    ones); replica `far`, if given, lies where gamma D0 is 600 .. 603 for the nearest landmark (sm.band_coordinate): every E_j is
    below 1e-250 there, and still a normal number for the nearest ones"""
    rng = np.random.default_rng(seed)
    L = np.asarray(landmarks)
    dims = L.shape[1] - 1
    X = np.zeros((n, dims), dtype=np.float32)
    for e in range(n):
        if e % 2 == 0:
            X[e] = (L[rng.integers(len(L)), :dims] + rng.uniform(-0.05, 0.05, dims)).astype(np.float32)
        else:
            X[e] = rng.uniform(0.0, sm.SPREAD.get(dims, 2.0), dims).astype(np.float32)
    if far is not None and far < n:
        X[far] = sm.far_state(dims, sm.band_coordinate(L[:, :dims], level=600.0))
    return X


def apply_list(landmarks, coeff, n_prbs, n, seed, kind, gamma=1.0):
    """a merged list of n proposals [n, 18] against a dictionary: near-duplicates of its landmarks (the state moved by up to 0.02 a
    coordinate, the allocation by up to three grid steps) with the label the dictionary does NOT predict: every one is a mistake
    against the dictionary as it stands.  kind 'stop': every proposal is followed by its copy, which stops being a mistake once
    the first is applied; 'none': distinct landmarks."""
    rng = np.random.default_rng(seed)
    L, co = np.asarray(landmarks, dtype=np.float64), np.asarray(coeff, dtype=np.float64)
    m, d = L.shape
    props = np.zeros((n, 18))
    picks = rng.permutation(m)
    i = 0
    while i < n:
        j = int(picks[i % m]) if kind == 'none' else int(rng.integers(m))
        st = (L[j, :d - 1] + rng.uniform(-0.02, 0.02, d - 1)).astype(np.float32)
        c = int(np.clip(int(round(L[j, d - 1] * n_prbs)) + rng.integers(-3, 4), 0, n_prbs))
        f = plain_scores(L, co, st, n_prbs, gamma)[0][c]
        y = -1 if f > 0 else 1
        for _ in range(2 if kind == 'stop' else 1):
            if i < n:
                props[i, 0], props[i, 1] = 7 * i + 3, proposal_word(c, y)
                props[i, 2:2 + d - 1] = st
                i += 1
    return props


def round_inputs(n_envs, dims, n_prbs, steps, seed):
    """[(states [N, nv] float32, actions [N, S], labels [N, S])]: a slice is satisfied when its allocation exceeds a demand that
    grows with the first state variable of its learner"""
    rng = np.random.default_rng(seed)
    nv, S = int(sum(dims)), len(dims)
    lead = np.cumsum([0] + list(dims))[:-1]
    out = []
    for _ in range(steps):
        states = (rng.random((n_envs, nv)) * 0.5).astype(np.float32)
        actions = rng.integers(2, n_prbs - 1, size=(n_envs, S)).astype(np.int32)
        demand = (states[:, lead] * 2 * (n_prbs - 10)).astype(np.int32) + 4
        out.append((states, actions, np.where(actions >= demand, 1, -1).astype(np.int32)))
    return out


def select(found, security, n_prbs):
    """select_kernel's and adjust_kernel's rule for one replica: found [S] = the first candidate with f > 0 (or -1), security [S]
    -> (actions [S], margins [S], adjusted)"""
    act, mar = [], []
    for fd, off in zip(found, security):
        a = min(n_prbs, fd + int(off)) if fd >= 0 else n_prbs
        act.append(a)
        mar.append(a - fd if fd >= 0 else 0)
    total = sum(act)
    if total <= n_prbs:
        return act, mar, 0
    na = [int(np.floor(float(n_prbs) * (float(a) / float(total)))) for a in act]
    return na, [m - (a - n) for m, a, n in zip(mar, act, na)], 1
