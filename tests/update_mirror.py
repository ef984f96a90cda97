"""A plain restatement of ONE Projectron.update as the device forms it (csrc/kb_kbrl.hip: predict_column / kernel_column_from_d0,
matvec_tri_tiles / matvec_tri_tiles_lds, matvec_tri_combine / matvec_tri_combine_wide, matvec_colsum, wave_dot256_rows,
residual_delta, finish_update, rank1_units), sum by sum in the order the kernels' comments state, and the exact value it
approximates; below it the same for ONE ProjectronPlus.update (apply_update_plus, margin_update: score, step_plus, exact_plus,
plus_bounds) and the inputs its tests are run on.  Used by tests/test_update_mirror.py (CPU), tests/test_gpu_update_chain.py and
tests/test_gpu_plus_chain.py (device).  Not a test module.

The input is what the device holds BEFORE the step: Kinv [m, m] (symmetric), the coefficients [m], the landmarks [m, d], the
sample x [d] and its label y.  The fused multiply-add, the division and rs_exp come from the oracle's library
(oracle.pyoracle.detmath: the bits tests/test_gpu_primitives.py pins the device to).

  column     K_f[j] = rs_exp(-gamma (D0_j + dl_j^2)), D0_j the squares (l_jq - x_q)^2 of the state coordinates added in
             coordinate order from 0.0, dl_j = l_j[d-1] - x[d-1] (the last coordinate last); float32 when m == 1
  dstar_tri  d* = Kinv K_f from the lower block triangle of 64 x 64 tiles (b_i, b_j), b_j <= b_i.  Per tile T:
               dpart[c] = sum_r T[r][c] K_f[64 b_i + r]: eight chains acc[u] <- fma(T[8 x + u][c], K_f[64 b_i + 8 x + u], acc[u]),
                          x = 0 .. 7 from 0.0 (the row classes r mod 8), then ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7));
               tpart[r] = sum_c T[r][c] K_f[64 b_j + c] (off-diagonal tiles): eight chains over the column classes c mod 8,
                          p[s] <- fma(T[r][s + 8 k], K_f[64 b_j + s + 8 k], p[s]), k = 0 .. 7 from 0.0, then the same tree;
             rows past m contribute zeros.  Output i = 64 b + c:  dsum = dpart(b, b)[c], then + dpart(b_r, b)[c] for
             b_r = b + 1 .. n_b - 1;  tsum = 0.0, then + tpart(b, b_r)[c] for b_r = 0 .. b - 1;  d*_i = dsum + tsum.
  dstar_col  the full-storage order of the shared handles (matvec_colsum): eight chains over the row classes j mod 8 down
             the WHOLE column i (increasing j, fused multiply-adds, from 0.0), then the tree.
  dot        sum_j d*_j K_f[j] (wave_dot256_rows): 256 strided sums part[t] += d*_j K_f[j], j = t, t + 256, ... (a multiply and
             an add, each rounded: the build has no contraction), from 0.0; within each group of 64 the xor butterfly
             32, 16, .. 1; the four group totals added in order from 0.0.
  delta      max(1 - dot, 0);  m <= 1: d* = float32(1.0f * float32 K_f) (0 when m == 0), dot = float32(d* K_f) in float32.
  branch     1 (projection) when delta <= eta or the dictionary is at its capacity, else 2 (insertion).
  project    coeff_j + y d*_j (y = +-1: the product is exact); float32 when m == 1.
  insert     d*_m = -1; every entry old + (d_i d_j) / delta (the product rounded, a true division, the sum rounded), the new
             row and column starting from 0.0; the new coefficient is y; m == 0: Kinv = [[1.0]].
"""
import numpy as np

U = 2.0 ** -53
KB_CH = 64


def _po():
    from oracle import pyoracle as po
    return po


def fma(a, b, c):
    """the correctly rounded a * b + c, element by element (broadcast)"""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.float64))
    out = _po().detmath('FMA', a.ravel(), np.concatenate([b.ravel(), c.ravel()]))
    return out.reshape(a.shape)


def div(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))
    return _po().detmath('DIV', a.ravel(), b.ravel()).reshape(a.shape)


def tree8(p, linear=False):
    """((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)) over the first axis (length 8); linear: ((((p0+p1)+p2)+p3)+ ... a contrasting order"""
    if linear:
        t = p[0]
        for k in range(1, 8):
            t = t + p[k]
        return t
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))


def column(landmarks, x, gamma):
    L = np.asarray(landmarks, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    m, d = L.shape
    d0 = np.zeros(m)
    for q in range(d - 1):
        t = L[:, q] - x[q]
        d0 = d0 + t * t
    dl = L[:, d - 1] - x[d - 1]
    k = _po().detmath('EXP_INLINE', -gamma * (d0 + dl * dl))
    return k.astype(np.float32).astype(np.float64) if m == 1 else k


def _padded(Kinv, kf):
    m = len(kf)
    nb = (m + 63) >> 6
    Kp = np.zeros((64 * nb, 64 * nb))
    Kp[:m, :m] = Kinv
    kp = np.zeros(64 * nb)
    kp[:m] = kf
    return Kp, kp, nb


def tri_tiles(Kinv, kf, classes=8, linear_tree=False):
    """the partial sums of every stored tile (matvec_tri_tiles) -> (dpart, tpart): dicts (b_i, b_j) -> 64 doubles; tpart holds the
    off-diagonal tiles only.  classes = 4 is a deliberately WRONG order (chains over index mod 4) for the tests of the tests."""
    Kp, kp, nb = _padded(Kinv, kf)
    tiles = [(bi, bj) for bi in range(nb) for bj in range(bi + 1)]
    T = np.stack([Kp[64 * bi:64 * bi + 64, 64 * bj:64 * bj + 64] for bi, bj in tiles])      # [nt, r, c]
    kr = np.stack([kp[64 * bi:64 * bi + 64] for bi, bj in tiles])
    kc = np.stack([kp[64 * bj:64 * bj + 64] for bi, bj in tiles])
    g, n = classes, 64 // classes
    acc = np.zeros((len(tiles), g, 64))      # [tile, row class u, column]
    for x in range(n):
        acc = fma(T[:, g * x:g * x + g, :], kr[:, g * x:g * x + g, None], acc)
    p = np.zeros((len(tiles), 64, g))        # [tile, row, column class s]
    for k in range(n):
        p = fma(T[:, :, g * k:g * k + g], kc[:, None, g * k:g * k + g], p)
    if g == 8:
        dp = tree8(np.moveaxis(acc, 1, 0), linear_tree)
        tp = tree8(np.moveaxis(p, 2, 0), linear_tree)
    else:
        dp = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
        tp = (p[:, :, 0] + p[:, :, 1]) + (p[:, :, 2] + p[:, :, 3])
    dpart = {t: dp[i] for i, t in enumerate(tiles)}
    tpart = {t: tp[i] for i, t in enumerate(tiles) if t[0] != t[1]}
    return dpart, tpart


def tri_combine(dpart, tpart, m, rows_first=False):
    """matvec_tri_combine.  rows_first: ONE chain over the row parts (increasing b_j) and then the column parts (increasing b_i) --
    a contrasting order, not the device's"""
    nb = (m + 63) >> 6
    out = np.zeros(64 * nb)
    for b in range(nb):
        if rows_first:
            s = np.zeros(64)
            for br in range(b):
                s = s + tpart[(b, br)]
            for br in range(b, nb):
                s = s + dpart[(br, b)]
        else:
            dsum = dpart[(b, b)].copy()
            for br in range(b + 1, nb):
                dsum = dsum + dpart[(br, b)]
            tsum = np.zeros(64)
            for br in range(b):
                tsum = tsum + tpart[(b, br)]
            s = dsum + tsum
        out[64 * b:64 * b + 64] = s
    return out[:m]


def dstar_tri(Kinv, kf, classes=8, linear_tree=False, rows_first=False):
    """-> (d* [m], dpart, tpart)"""
    dpart, tpart = tri_tiles(Kinv, kf, classes, linear_tree)
    return tri_combine(dpart, tpart, len(kf), rows_first), dpart, tpart


def dstar_col(Kinv, kf):
    """matvec_colsum: the column walk of the handles that store both triangles"""
    Kp, kp, nb = _padded(Kinv, kf)
    acc = np.zeros((8, 64 * nb))
    for t in range(8 * nb):
        acc = fma(Kp[8 * t:8 * t + 8, :], kp[8 * t:8 * t + 8, None], acc)
    return tree8(acc)[:len(kf)]


def dstar_rows(Kinv, kf):
    """the oracle's order (oracle/kb_oracle.c: kbo_update): row i in increasing j, a multiply and an add each rounded"""
    Kinv, kf = np.asarray(Kinv, dtype=np.float64), np.asarray(kf, dtype=np.float64)
    acc = np.zeros(len(kf))
    for j in range(len(kf)):
        acc = acc + Kinv[:, j] * kf[j]
    return acc


def dot(a, b):
    """wave_dot256_rows"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    m = len(a)
    n = (m + 255) // 256 * 256
    pa, pb = np.zeros(n), np.zeros(n)
    pa[:m], pb[:m] = a, b
    part = np.zeros(256)
    for j0 in range(0, n, 256):
        live = np.arange(j0, j0 + 256) < m       # (a lane past the end adds nothing; adding +0.0 to a sum from 0.0 is the same)
        part = np.where(live, part + pa[j0:j0 + 256] * pb[j0:j0 + 256], part)
    part = part.reshape(4, 64)
    lane = np.arange(64)
    for dd in (32, 16, 8, 4, 2, 1):
        part = part + part[:, lane ^ dd]
    t = 0.0
    for v in range(4):
        t = t + part[v, 0]
    return float(t)


def step(Kinv, coeff, landmarks, x, y, gamma=1.0, eta=0.1, capacity=None, **order):
    """one Projectron.update of a sample the learner misclassified -> dict(column, dstar, dpart, tpart, dot, delta, branch,
    m, coeff, kinv): the state after the step, every stage in the device's order (`order`: dstar_tri's contrasting switches;
    order='col': d* by dstar_col, the column walk of the handles that store both triangles -- the shared ones)"""
    col = order.pop('order', 'tri') == 'col'
    x = np.asarray(x, dtype=np.float64)
    m = len(coeff)
    d = len(x)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    coeff = np.asarray(coeff, dtype=np.float64)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    kf = column(L, x, gamma) if m else np.zeros(0)
    dpart, tpart = {}, {}
    if m == 0:
        ds, dt = np.zeros(0), 0.0
    elif m == 1:
        ds = np.array([float(np.float32(1.0) * np.float32(kf[0]))])
        dt = float(np.float32(ds[0]) * np.float32(kf[0]))
    elif col:
        ds = dstar_col(Kinv, kf)
        dt = dot(ds, kf)
    else:
        ds, dpart, tpart = dstar_tri(Kinv, kf, **order)
        dt = dot(ds, kf)
    delta = 1.0 - dt
    delta = delta if delta > 0.0 else 0.0
    full = capacity is not None and m >= capacity
    out = dict(column=kf, dstar=ds, dpart=dpart, tpart=tpart, dot=dt, delta=delta)
    if delta <= eta or full:
        nc = coeff + float(y) * ds
        if m == 1:
            nc = nc.astype(np.float32).astype(np.float64)
        out.update(branch=1, m=m, coeff=nc, kinv=Kinv.copy(), landmarks=L.copy())
        return out
    d1 = np.append(ds, -1.0)
    old = np.zeros((m + 1, m + 1))
    old[:m, :m] = Kinv
    if m == 0:
        new = np.ones((1, 1))
    else:
        new = old + div(d1[:, None] * d1[None, :], delta)
    out.update(branch=2, m=m + 1, coeff=np.append(coeff, float(y)), kinv=new, landmarks=np.vstack([L, x[None]]))
    return out


# ------------------------------------------------------------------ the exact value and the forward bound
def exact_step(Kinv, kf):
    """d* = Kinv K_f of the SAME doubles and the scale S_i = sum_j |Kinv_ij| |K_f_j| of its forward error, with delta =
    max(1 - K_f . d*, 0), in longdouble (64-bit significand, pairwise sums).  Its own error is at most exact_units(m) u S_i:
    one rounding of each product and fewer than m of the sum, 2^-64 each.  -> (d* [m], S [m], delta) as longdouble"""
    ld = np.longdouble
    assert np.finfo(ld).nmant >= 63, 'exact_step needs an extended long double'
    # (a Kinv handed over as longdouble is the caller's conversion of the same doubles, made once for many steps)
    K = Kinv if getattr(Kinv, 'dtype', None) == ld else np.asarray(Kinv, dtype=np.float64).astype(ld)
    k = np.asarray(kf, dtype=np.float64).astype(ld)
    P = K * k[None, :]
    ds = P.sum(axis=1)
    S = np.abs(P).sum(axis=1)
    delta = ld(1) - (ds * k).sum()
    return ds, S, (delta if delta > 0 else ld(0))


def exact_units(m):
    """the error of exact_step's d* in units of u S_i: (m + 1) roundings of 2^-64 = 2^-11 u"""
    return (m + 1) * 2.0 ** -11


def bound_units(m, order='tri'):
    """The forward bound of |d*_i - (Kinv K_f)_i| in units of u S_i, u = 2^-53, S_i = sum_j |Kinv_ij| |K_f_j|, for the inputs as
    the doubles they are (first order n u, then through gamma_n = n u / (1 - n u)).

    Every product Kinv_ij K_f_j is exact inside its fused multiply-add and is then carried through n roundings, each of which
    scales the running sum by (1 + e), |e| <= u, so it ends up within gamma_n of itself and d*_i within gamma_n S_i.  Counting n
    for the stated order ('tri'), n_b = ceil(m / 64) blocks:
      * the chain of its class inside the tile: eight fused multiply-adds, one rounding each, the first product going through
        all of them:                                                                                   8
      * the tree ((p0+p1)+(p2+p3))+((p4+p5)+(p6+p7)): three additions deep:                            3
      * the combine.  A column part dpart(b_r, b) enters a chain of n_b - b parts, at most n_b - 1 additions (block 0); a row
        part tpart(b, b_r) a chain of b parts from 0.0 -- the first addition 0.0 + t is exact -- at most n_b - 2 additions:
                                                                                                       n_b - 1
      * the final dsum + tsum, where there is a row part at all (n_b > 1):                             1
    so n = 11 for one block and n_b + 11 beyond.  m == 1: d* = float32(1.0f * K_f) of a float32 K_f is K_f itself: 0.
    'col' (matvec_colsum): one chain of 8 n_b fused multiply-adds down the whole column and the tree: n = 8 n_b + 3.
    'rows' (the oracle's row walk): the product rounds once and goes through at most m - 1 rounded additions (the first,
    0.0 + p, is exact): n = m."""
    if m <= 1:
        return 0.0
    nb = (m + 63) >> 6
    n = {'tri': 11 + (nb if nb > 1 else 0), 'col': 8 * nb + 3, 'rows': m}[order]
    return n / (1.0 - n * U)


def error_ratio(ds, Kinv, kf, order='tri'):
    """-> (max_i |ds_i - exact_i| / ((bound_units + exact_units) u S_i), max_i |ds_i - exact_i| / (u S_i)): the first is at most 1
    when the order keeps its bound (outputs whose scale S_i is zero must be exact)"""
    ld = np.longdouble
    m = len(kf)
    ex, S, _ = exact_step(Kinv, kf)
    err = np.abs(np.asarray(ds, dtype=np.float64).astype(ld) - ex)
    if m <= 1:
        return (0.0, 0.0) if (err == 0).all() else (np.inf, np.inf)
    assert (err[S == 0] == 0).all()
    if not (S > 0).any():
        return 0.0, 0.0
    units = float((err[S > 0] / (ld(U) * S[S > 0])).max())
    return units / (bound_units(m, order) + exact_units(m)), units


# ------------------------------------------------------------------ Projectron++: the margin step (apply_update_plus, margin_update)
U32 = 2.0 ** -24
PLUS_SWITCHES = ('loss64', 'alpha_order', 'fused_coeff', 'slack_ge', 'f_pairwise')
TERMS = ('loss', 'one', 'slack')     # the three terms of alpha: loss / norm, 1.0, (2 slack) / norm


def score(kf, coeff, pairwise=False):
    """predict_column's f = K_f . coeff: the order dot() states -- 256 strided sums part[t] += K_f[j] coeff[j], j = t, t + 256, ...
    (a product and an add, each rounded) from 0.0, the xor butterfly 32, 16, .. 1 within each group of 64, the four group totals
    added in order from 0.0 (block_sum of a 256-thread block).  0.0 for the empty dictionary; float32(float32 K_f * float32 coeff)
    while one landmark is held.  pairwise: numpy's pairwise sum of the rounded products -- a contrasting order, not the device's"""
    kf, coeff = np.asarray(kf, dtype=np.float64), np.asarray(coeff, dtype=np.float64)
    m = len(kf)
    if m == 0:
        return 0.0
    if m == 1:
        return float(np.float32(kf[0]) * np.float32(coeff[0]))
    if pairwise:
        return float(_po().pairwise_sum(kf * coeff))
    return dot(kf, coeff)


def step_plus(Kinv, coeff, landmarks, x, y, gamma=1.0, eta=0.1, capacity=None, **contrast):
    """one ProjectronPlus.update as the device forms it (predict_column, then apply_update_plus and margin_update, statement for
    statement) -> dict of every stage and of the state after.

      column   as in step(); f = score(column, coeff); margin = y f (y = +-1: exact).
      branch 0 margin >= 1.0: nothing is formed and nothing written; delta is returned as 0.0.
      mistake  margin <= 0.0: step() -- Projectron's update, branches 1 and 2 (the empty dictionary has f = 0.0 and comes here).
      margin   otherwise.  d* and dot as in step() (m == 1: d* = float32(1.0f * float32 K_f), dot = float32(d* K_f));
               delta = max(1.0 - dot, 0.0);  norm = max(1.0 - delta, 0.0);  loss = 1.0 - margin, while one landmark is held
               float32(1.0f - float32(margin));  slack = loss - delta / eta (a true division, the difference rounded).
      branch 4 not (slack > 0.0): nothing is written.
      branch 3 alpha = loss / norm (div(); +inf when norm == 0.0), then 1.0 where 1.0 < alpha, then (2.0 slack) / norm (2 slack is
               exact; div()) where that is < alpha: `won` names the term that stands ('loss', 'one', 'slack'; on a tie the
               earlier one).  coeff_j <- coeff_j + (alpha y) d*_j: alpha y exact, the product rounded, the sum rounded; stored as
               float32 while one landmark is held.  Kinv and the landmarks stay.

    contrast: the switches of dstar_tri, and deliberately WRONG forms of the margin rule for the tests of the tests --
    loss64 (the float64 loss while one landmark is held), alpha_order (the three terms compared from 1.0: 1.0, then 2 slack / norm,
    then loss / norm), fused_coeff (ONE fused multiply-add forms the new coefficient), slack_ge (slack >= 0.0 opens branch 3),
    f_pairwise (score(pairwise=True)).  The minimum of three numbers does not depend on the order they are compared in, so
    alpha_order can only show in `won`, and only on an exact tie of two terms; slack_ge only on slack == 0.0 exactly.

    keys: column, f, margin, dstar, dpart, tpart, dot, delta, norm, loss, slack, branch, terms (loss / norm, 1.0, 2 slack / norm),
    won, alpha, m, coeff, kinv, landmarks; what a branch does not form is NaN (None for terms and won)."""
    sw = {k: bool(contrast.pop(k, False)) for k in PLUS_SWITCHES}
    x = np.asarray(x, dtype=np.float64)
    m = len(coeff)
    d = len(x)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    coeff = np.asarray(coeff, dtype=np.float64)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    kf = column(L, x, gamma) if m else np.zeros(0)
    f = score(kf, coeff, sw['f_pairwise'])
    margin = float(y) * f
    nan = float('nan')
    out = dict(column=kf, f=f, margin=margin, dstar=np.zeros(0), dpart={}, tpart={}, dot=nan, delta=0.0, norm=nan, loss=nan,
               slack=nan, terms=None, won=None, alpha=nan)
    if margin >= 1.0:
        out.update(branch=0, m=m, coeff=coeff.copy(), kinv=Kinv.copy(), landmarks=L.copy())
        return out
    if margin <= 0.0:
        out.update(step(Kinv, coeff, L, x, y, gamma, eta, capacity, **contrast))
        return out
    if m == 1:
        ds = np.array([float(np.float32(1.0) * np.float32(kf[0]))])
        dt = float(np.float32(ds[0]) * np.float32(kf[0]))
    else:
        ds, dpart, tpart = dstar_tri(Kinv, kf, **contrast)
        dt = dot(ds, kf)
        out.update(dpart=dpart, tpart=tpart)
    delta = 1.0 - dt
    delta = delta if delta > 0.0 else 0.0
    norm = 1.0 - delta
    norm = norm if norm > 0.0 else 0.0
    loss = float(np.float32(1.0) - np.float32(margin)) if m == 1 and not sw['loss64'] else 1.0 - margin
    slack = loss - delta / eta
    out.update(dstar=ds, dot=dt, delta=delta, norm=norm, loss=loss, slack=slack, m=m, kinv=Kinv.copy(), landmarks=L.copy())
    if not (slack >= 0.0 if sw['slack_ge'] else slack > 0.0):
        out.update(branch=4, coeff=coeff.copy())
        return out
    with np.errstate(divide='ignore', invalid='ignore'):
        by_loss, by_slack = float(div(loss, norm)), float(div(2.0 * slack, norm))
    if sw['alpha_order']:
        alpha, won = 1.0, 'one'
        if by_slack < alpha:
            alpha, won = by_slack, 'slack'
        if by_loss < alpha:
            alpha, won = by_loss, 'loss'
    else:
        alpha, won = by_loss, 'loss'
        if 1.0 < alpha:
            alpha, won = 1.0, 'one'
        if by_slack < alpha:
            alpha, won = by_slack, 'slack'
    ay = alpha * float(y)
    nc = fma(ds, ay, coeff) if sw['fused_coeff'] else coeff + ay * ds
    if m == 1:
        nc = nc.astype(np.float32).astype(np.float64)
    out.update(branch=3, terms=(by_loss, 1.0, by_slack), won=won, alpha=alpha, coeff=nc)
    return out


def f_units(m):
    """The forward bound of |f - K_f . coeff| in units of u Sf, Sf = sum_j |K_f_j coeff_j|, and of |dot - d* . K_f| in units of
    u sum_j |d*_j K_f_j| (wave_dot256_rows is the same order), for the inputs as the doubles they are.  A product is rounded once
    and then carried through the additions behind it, each of which scales the running sum by (1 + e), |e| <= u:
      * its strided chain of n_c = ceil(m / 256) terms: the first addition 0.0 + p is exact, so at most n_c - 1 additions; with the
        product's own rounding:                                                                      n_c
      * the butterfly 32, 16, .. 1:                                                                  6
      * the four group totals in order from 0.0, the first addition exact:                           3
    n = n_c + 9, through gamma_n = n u / (1 - n u).  m == 1: ONE float32 product, 2^-24 = 2^29 u."""
    if m <= 0:
        return 0.0
    if m == 1:
        return U32 / U
    n = (m + 255) // 256 + 9
    return n / (1.0 - n * U)


def exact_plus(Kinv, kf, coeff, y, eta):
    """the margin step of the SAME doubles (Kinv, the kernel column K_f, the coefficients, eta) in longdouble, beside exact_step ->
    dict: f = K_f . coeff and its scale Sf = sum |K_f_j coeff_j|; dstar and S (exact_step); dot = d* . K_f and its scale
    T = sum_j S_j |K_f_j|; margin, delta, norm, loss, slack, terms (loss / norm, 1, 2 slack / norm), alpha, won, coeff (the
    coefficients after a margin update), branch (0, 3, 4; -1 for a mistake, which exact_step covers).  Its own error: every
    operation rounds to 2^-64 = 2^-11 u; plus_bounds allows for it."""
    ld = np.longdouble
    ds, S, delta = exact_step(Kinv, kf)
    k, c = np.asarray(kf, dtype=np.float64).astype(ld), np.asarray(coeff, dtype=np.float64).astype(ld)
    f, Sf = (k * c).sum(), np.abs(k * c).sum()
    dt, T = (ds * k).sum(), (S * np.abs(k)).sum()
    margin = ld(int(y)) * f
    norm = ld(1) - delta
    norm = norm if norm > 0 else ld(0)
    loss = ld(1) - margin
    slack = loss - delta / ld(eta)
    inf = ld(np.inf)
    terms = (loss / norm if norm > 0 else inf, ld(1), 2 * slack / norm if norm > 0 else (inf if slack > 0 else -inf))
    won = int(np.argmin([float(t) for t in terms])) if terms[0] != terms[1] and terms[1] != terms[2] and terms[0] != terms[2] else None
    alpha = min(terms)
    branch = 0 if margin >= 1 else -1 if margin <= 0 else 3 if slack > 0 else 4
    return dict(f=f, Sf=Sf, dstar=ds, S=S, dot=dt, T=T, margin=margin, delta=delta, norm=norm, loss=loss, slack=slack, terms=terms,
                won=None if won is None else TERMS[won], alpha=alpha, coeff=c + alpha * ld(int(y)) * ds, branch=branch)


def plus_bounds(ex, m, eta):
    """The forward bounds of the margin step's scalar chain against exact_plus (`ex`), from the bounds of its two sums: B = bound_units(m)
    for d* (|d^_i - d*_i| <= B u S_i; a hat marks the device's value) and F = f_units(m) for f and dot.  Every later operation is
    ONE rounding: fl(v) is within u |v| of v, and |v| is at most its exact value plus the error already carried.

      f        E_f = F u Sf;  margin = y f^ is exact:  E_margin = E_f
      dot      the sum is formed of d^, not d*:  |sum d^_j k_j - sum d*_j k_j| <= B u T, T = sum_j S_j |k_j|, and its own rounding is
               F u sum |d^_j k_j| <= F u (1 + B u) T (|d*_j| <= S_j):            E_dot = (B + F (1 + B u)) u T
      delta    fl(1 - dot^), and max(., 0) moves no two values apart:            E_delta = E_dot + u (|1 - dot| + E_dot)
      norm     the same once more:                                               E_norm = E_delta + u (|1 - delta| + E_delta)
      loss     fl(1 - margin^):                                                  E_loss = E_f + v (|loss| + E_f)
               v = u; while one landmark is held f^ is a float32, so float32(margin^) is exact and the difference rounds to
               v = 2^-24
      slack    q = delta / eta:  E_q = E_delta / eta + u (|q| + E_delta / eta) -- the error of dot enters divided by eta --
               then fl(loss^ - q^):                                              E_slack = E_loss + E_q + u (|slack| + E_loss + E_q)
      terms    a^/n^ - a/n = (a^ - a)/n^ + (a/n)(n - n^)/n^ with n^ >= norm - E_norm (which must be positive, else no bound):
               R_loss = (E_loss + |loss / norm| E_norm) / (norm - E_norm),  R_slack = (2 E_slack + |2 slack / norm| E_norm) / (norm - E_norm)
               -- the error of dot enters divided by norm -- and the division's rounding:  E_t = R_t + u (|t| + R_t);  E_one = 0
      alpha    where the exact winner is clear of both others by more than their errors added, the device's alpha is the same
               term: E_alpha = E_won; otherwise min() moves no two triples apart: E_alpha = max(E_loss_term, E_slack_term)
      coeff_i  alpha^ d^_i against alpha d*_i:  P_i = E_alpha (|d*_i| + B u S_i) + alpha B u S_i;  the product's rounding:
               Q_i = P_i + u (|alpha d*_i| + P_i);  the sum's:  E_c_i = Q_i + u (|c'_i| + Q_i), c' the exact new coefficient;  while
               one landmark is held the float32 store:  + 2^-24 (|c'_i| + E_c_i).

    exact_plus's own roundings (2^-11 u each, one or two where the device has one): B and F take exact_units(m), every u above is
    taken as u (1 + 2^-10).  -> dict(f, dot, delta, norm, loss, slack, terms (3), alpha, coeff [m]) as float64"""
    fl = lambda v: np.asarray(v, dtype=np.float64)
    ue = U * (1.0 + 2.0 ** -10)
    v = U32 * (1.0 + 2.0 ** -10) if m == 1 else ue
    B = (bound_units(m) + exact_units(m)) if m > 1 else 0.0
    F = f_units(m) + exact_units(m)
    Sf, T, S, ds = float(ex['Sf']), float(ex['T']), fl(ex['S']), np.abs(fl(ex['dstar']))
    dt, delta, norm, loss, slack = (float(ex[k]) for k in ('dot', 'delta', 'norm', 'loss', 'slack'))
    t_loss, _, t_slack = (float(t) for t in ex['terms'])
    alpha = float(ex['alpha'])
    E_f = F * U * Sf
    E_dot = (B + F * (1.0 + B * U)) * U * T
    E_delta = E_dot + ue * (abs(1.0 - dt) + E_dot)
    E_norm = E_delta + ue * (abs(1.0 - delta) + E_delta)
    E_loss = E_f + v * (abs(loss) + E_f)
    E_q = E_delta / eta
    E_q = E_q + ue * (abs(delta / eta) + E_q)
    E_slack = E_loss + E_q
    E_slack = E_slack + ue * (abs(slack) + E_slack)
    den = norm - E_norm
    if den > 0.0 and np.isfinite(t_loss) and np.isfinite(t_slack):
        R = (E_loss + abs(t_loss) * E_norm) / den
        E1 = R + ue * (abs(t_loss) + R)
        R = (2.0 * E_slack + abs(t_slack) * E_norm) / den
        E3 = R + ue * (abs(t_slack) + R)
    else:
        E1 = E3 = np.inf
    Et = (E1, 0.0, E3)
    tv = (t_loss, 1.0, t_slack)
    w = ex['won']
    clear = w is not None and all(tv[i] - tv[TERMS.index(w)] > Et[i] + Et[TERMS.index(w)] for i in range(3) if TERMS[i] != w)
    E_alpha = Et[TERMS.index(w)] if clear else max(E1, E3)
    P = E_alpha * (ds + B * U * S) + abs(alpha) * B * U * S
    Q = P + ue * (abs(alpha) * ds + P)
    cn = np.abs(fl(ex['coeff']))
    E_c = Q + ue * (cn + Q)
    if m == 1:
        E_c = E_c + v * (cn + E_c)
    return dict(f=E_f, dot=E_dot, delta=E_delta, norm=E_norm, loss=E_loss, slack=E_slack, terms=Et, alpha=E_alpha, coeff=E_c,
                won_clear=clear)


def plus_ratios(mir, ex, bd):
    """-> dict(f, coeff, dstar): error / bound of the mirror's or the device's stage output `mir` (keys f, and optionally coeff
    after a margin update and dstar) against exact_plus; a zero bound demands equality"""
    ld = np.longdouble

    def ratio(err, bound):
        err, bound = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(bound, dtype=np.float64))
        if (err[bound == 0] != 0).any():
            return np.inf
        return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    out = dict(f=ratio(abs(ld(mir['f']) - ex['f']), bd['f']))
    if mir.get('dstar') is not None and len(ex['S']) >= 2:      # (error_ratio's figure, from the exact step already formed)
        m = len(ex['S'])
        out['dstar'] = ratio(np.abs(np.asarray(mir['dstar'], dtype=np.float64).astype(ld) - ex['dstar']),
                             (bound_units(m) + exact_units(m)) * U * np.asarray(ex['S'], dtype=np.float64))
    if 'coeff' in mir and mir['coeff'] is not None:
        out['coeff'] = ratio(np.abs(np.asarray(mir['coeff'], dtype=np.float64).astype(ld) - ex['coeff']), bd['coeff'])
    return out


# ------------------------------------------------------------------ the inputs of the Projectron++ tests
CASES = ('branch0', 'branch4', 'slack', 'loss', 'one')    # branch 3 by the term of alpha that wins; in the order a learner takes
                                                          # them one after the other: the smaller steps of its coefficients first
PLUS_LADDER10 = [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 575, 576, 577, 640, 641]
PLUS_LADDER3 = [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193]


def cases_required(m):
    """the cases a ladder learner of m landmarks must supply (one landmark with a coefficient of +-1 has slack < 0 throughout:
    one_landmark_inputs covers that size)"""
    return CASES if m >= 63 else ('branch4', 'loss', 'slack') if m >= 2 else ()
SHIFTS = (0, .002, .005, .01, .02, .03, .04, .05, .07, .1, .2, .4)
MOVES = (0, 1, 5, 20, -20)
CLEARANCE = 1e-6


class PlusInputs:
    """The candidates of one learner for the cases of the margin rule, preselected in plain float64 (NumPy's sums and exp, no
    device order): the first `tries` landmarks of the dictionary, each with its state shifted by t of SHIFTS on every state
    coordinate (rounded to float32) and its allocation moved by g of MOVES grid steps (kept inside 0 .. n_prbs), labelled
    y = sign(f).  A candidate is of a case only when its margin, its slack and the gaps between the terms of alpha are at
    least CLEARANCE from their thresholds.  Kinv and the landmarks do not change under the margin rule, so the kernel columns K of
    the candidates and their delta = 1 - K . Kinv K are formed once -- in batches of BATCH landmarks and only as far as the search
    gets, delta only where the margin leaves the case open; pick(coeff, case) classifies under the coefficients the learner holds
    now and returns the first candidate of the case."""
    BATCH = 4

    def __init__(self, Kinv, landmarks, gamma, eta, n_prbs, tries=48):
        self.L = np.asarray(landmarks, dtype=np.float64)
        self.m, self.d = self.L.shape
        self.Kinv = np.asarray(Kinv, dtype=np.float64).reshape(self.m, self.m)
        self.gamma, self.eta, self.n_prbs, self.n = gamma, eta, n_prbs, min(self.m, tries)
        self.l2 = (self.L ** 2).sum(axis=1)
        self.batches = []

    def _batch(self, b):
        while len(self.batches) <= b:
            L, d, X = self.L, self.d, []
            for j in range(self.BATCH * len(self.batches), min(self.BATCH * (len(self.batches) + 1), self.n)):
                for t in SHIFTS:
                    for g in MOVES:
                        a = int(round(L[j, d - 1] * self.n_prbs)) + g
                        if 0 <= a <= self.n_prbs:
                            X.append(np.append((L[j, :d - 1] + t).astype(np.float32).astype(np.float64), a / float(self.n_prbs)))
            X = np.asarray(X)
            K = np.exp(-self.gamma * np.maximum(self.l2[:, None] + (X ** 2).sum(axis=1)[None, :] - 2.0 * (L @ X.T), 0.0))    # [m, n]
            if self.m == 1:
                K = K.astype(np.float32).astype(np.float64)
            self.batches.append(dict(X=X, K=K, delta=np.full(len(X), np.nan)))
        return self.batches[b]

    def _classify(self, bt, coeff, cases):
        """-> (case index into CASES or -1 [n], y [n]) of one batch; only the cases of `cases` are looked for"""
        K, c = bt['K'], CLEARANCE
        f = np.asarray(coeff, dtype=np.float64) @ K
        y = np.where(f > 0, 1, -1)
        margin = np.abs(f)
        case = np.full(len(f), -1)
        case[margin >= 1.0 + c] = 0
        inside = (margin >= c) & (margin <= 1.0 - c)
        if set(cases) <= {'branch0'}:
            return case, y
        if set(cases) <= {'branch0', 'one'}:
            # alpha = 1 needs loss >= norm and 2 slack >= norm, that is margin <= delta <= (1 - 2 margin) / (2 / eta - 1): no
            # delta can do both unless margin (2 / eta - 1) <= 1 - 2 margin
            inside &= margin * (2.0 / self.eta + 1.0) <= 1.0
        need = inside & np.isnan(bt['delta'])
        if need.any():
            Kn = K[:, need]
            bt['delta'][need] = np.maximum(1.0 - (Kn * (self.Kinv @ Kn)).sum(axis=0), 0.0)
        delta = np.where(inside, bt['delta'], 0.0)
        norm = np.maximum(1.0 - delta, 0.0)
        loss = 1.0 - margin
        slack = loss - delta / self.eta
        with np.errstate(divide='ignore', invalid='ignore'):
            t = np.stack([loss / norm, np.ones_like(loss), 2.0 * slack / norm])
        case[inside & (slack <= -c)] = 1
        for w in range(3):
            others = [i for i in range(3) if i != w]
            wins = (t[others[0]] - t[w] >= c) & (t[others[1]] - t[w] >= c)
            case[inside & (slack >= c) & (norm >= c) & wins] = CASES.index(TERMS[w])
        return case, y

    def pick(self, coeff, case):
        """-> (x, y) of the first candidate of `case` under `coeff`, or None"""
        for b in range((self.n + self.BATCH - 1) // self.BATCH):
            bt = self._batch(b)
            cs, y = self._classify(bt, coeff, (case,))
            at = np.nonzero(cs == CASES.index(case))[0]
            if at.size:
                return bt['X'][at[0]].copy(), int(y[at[0]])
        return None

    def counts(self, coeff):
        """the candidates of every case among all of them (the whole search: for a test's report, not for its run)"""
        tot = np.zeros(len(CASES), dtype=np.int64)
        for b in range((self.n + self.BATCH - 1) // self.BATCH):
            cs, _ = self._classify(self._batch(b), coeff, CASES)
            tot += np.bincount(cs[cs >= 0], minlength=len(CASES))
        return {c: int(tot[i]) for i, c in enumerate(CASES)}


def one_landmark_inputs(gamma=1.0, eta=0.1, seed=11):
    """The hand-built inputs of the float32 regime (one landmark of ten state variables, a coefficient other than +-1):
    -> dict(x0, points = [(name, near, x)]): one learner per point inserts x0 with y = +1, projects `near` with y = -1 (x0 + 0.05
    on every state coordinate: delta 0.049, a coefficient of about 0.025 as float32) and is taught x with y = +1 -- x0 shifted on
    its first coordinate to kernel values of about 1, 0.98, 0.955 and 0.94, and two exact ties found by a search over the float32
    kernel values in the mirror's own arithmetic (x is None where the search finds none): 'tie_alpha' with loss == norm, so
    loss / norm == 1.0 exactly, and 'tie_slack' with loss == delta / eta, slack == 0.0 exactly -- what the switches alpha_order
    and slack_ge need to show; a tie's `near` lies 0.05 .. 0.07 away, whichever coefficient first admits one"""
    rng = np.random.default_rng(seed)
    x0 = np.append((rng.random(10) * 1.6).astype(np.float32).astype(np.float64), 0.5)
    one = np.ones((1, 1))

    def projected(shift):
        near = x0.copy()
        near[:10] = (near[:10] + shift).astype(np.float32)
        st = step_plus(one, [1.0], x0[None], near, -1, gamma, eta)
        assert st['branch'] == 1 and len(st['coeff']) == 1
        return near, np.float32(st['coeff'][0])
    near, _ = projected(0.05)
    points = []
    for name, k in (('k1.0', 0.999999), ('k0.98', 0.98), ('k0.955', 0.955), ('k0.94', 0.94)):
        x = x0.copy()
        x[0] += np.sqrt(-np.log(k) / gamma)
        points.append((name, near, x))
    # The ties.  With the coefficient c: loss = 1 - c k, norm = k^2, delta / eta = (1 - k^2) / eta, so loss == norm where
    # k^2 + c k = 1 and slack == 0 where (1 - k^2) / eta = 1 - c k.  The kernel value is monotone in the shift: a fine ladder of
    # shifts around the crossing visits every float32 there.  Whether one of them is an exact tie depends on c, so the projected
    # point moves (0.05, 0.0502, ...: delta stays below eta) until one is.
    for name in ('tie_alpha', 'tie_slack'):
        found = (name, None, None)
        for shift in 0.05 + 0.0002 * np.arange(100):
            near_t, c = projected(shift)
            cf = float(c)
            k_mid = (-cf + np.sqrt(cf * cf + 4.0)) / 2.0 if name == 'tie_alpha' else \
                (cf * eta + np.sqrt((cf * eta) ** 2 + 4.0 * (1.0 - eta))) / 2.0
            s = np.sqrt(-np.log(k_mid) / gamma) + np.arange(-4000, 4001) * 2e-8
            P = np.tile(x0, (len(s), 1))
            P[:, 0] += s
            k = column(P, x0, gamma).astype(np.float32)      # (the squares do not see which of the two points is the sample)
            delta = np.maximum(1.0 - (k * k).astype(np.float64), 0.0)
            norm = np.maximum(1.0 - delta, 0.0)
            loss = (np.float32(1.0) - k * c).astype(np.float64)
            at = np.nonzero((loss == norm) if name == 'tie_alpha' else (loss - delta / eta == 0.0))[0]
            if at.size:
                found = (name, near_t, P[at[0]].copy())
                break
        points.append(found)
    return dict(x0=x0, points=points)
