"""A plain restatement of ONE Projectron.update as the device forms it (csrc/kb_kbrl.hip: predict_column / kernel_column_from_d0,
matvec_tri_tiles / matvec_tri_tiles_lds, matvec_tri_combine / matvec_tri_combine_wide, matvec_colsum, wave_dot256_rows,
residual_delta, finish_update, rank1_units), sum by sum in the order the kernels' comments state, and the exact value it
approximates.  Used by tests/test_update_mirror.py (CPU) and tests/test_gpu_update_chain.py (device).  Not a test module.

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
    m, coeff, kinv): the state after the step, every stage in the device's order (`order`: dstar_tri's contrasting switches)"""
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
    K, k = np.asarray(Kinv, dtype=np.float64).astype(ld), np.asarray(kf, dtype=np.float64).astype(ld)
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
