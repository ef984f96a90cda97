"""Shared by tests/test_primitives.py (CPU) and tests/test_gpu_primitives.py (device): the input sets of the deterministic
elementary functions, an integer restatement of Philox4x32-10 and of the stream draws, and the ulp measure against mpmath.
Not a test module."""
import functools
import math

import numpy as np

M32 = 0xffffffff
EXP_HI, EXP_LO = 709.782712893384, -745.2  # rs_exp's two cut-offs (include/rs_detmath.h)
LN2 = 0.6931471805599453
DBL_MAX = 1.7976931348623157e308
NAN, INF = float('nan'), float('inf')


# ------------------------------------------------------------------ Philox4x32-10 and the draws, in Python integers
def philox4x32_10(c, k):
    """Random123's Philox4x32-10: counter words c[0..3], key words k[0..1] -> the four output words"""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0 = 0xD2511F53 * c0
        p1 = 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + 0x9E3779B9) & M32
        k1 = (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def py_block(row):
    """first two words for a probe row (c0, c1, c2, c3, k0, k1)"""
    r = [int(v) for v in row]
    return philox4x32_10(r[:4], r[4:])[:2]


def py_uniform(st):
    """st = [key0, key1, slice, serial, ctr] (Python ints, advanced in place): rs_stream_uniform"""
    a, b = philox4x32_10((st[4], 0, st[3], st[2]), (st[0], st[1]))[:2]
    st[4] = (st[4] + 1) & M32
    return float(((a << 32) | b) >> 11) * 2.0 ** -53


def py_integers(st, n):
    v = int(py_uniform(st) * float(n))
    return v if v < n else n - 1


def py_walker(row, T):
    """row = (key0, key1, slice, serial, now, attempt): rs_walker_redraw"""
    r = [int(v) for v in row]
    a, b = philox4x32_10((r[4], (1 + r[5]) & M32, r[3], r[2]), (r[0], r[1]))[:2]
    return (a * T) >> 32, (1 if b >> 31 else -1)


def random_streams(rng, n):
    """n stream rows (key0, key1, slice, serial, ctr): random words, small and extreme field values, counters about to wrap"""
    st = rng.integers(0, 1 << 32, size=(n, 5), dtype=np.uint64).astype(np.uint32)
    st[: n // 4, 2] = rng.integers(0, 8, n // 4)          # slice ids and serials as the simulator has them
    st[: n // 4, 3] = rng.integers(0, 200, n // 4)
    st[: n // 2, 4] = rng.integers(0, 5000, n // 2)
    edge = rng.integers(0, n, 64)
    st[edge[:32], 4] = M32 - rng.integers(0, 3, 32)       # ctr wraps within the draw
    st[edge[32:48], rng.integers(0, 5, 16)] = M32
    st[edge[48:], rng.integers(0, 5, 16)] = 0
    return st


# ------------------------------------------------------------------ input sets (tests/test_primitives.py states what each holds)
def _around(x, k):
    """the 2 k + 1 doubles around x"""
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = math.nextafter(lo, -INF), math.nextafter(hi, INF)
        out += [lo, hi]
    return out


def _shuffled(parts, seed):
    v = np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in parts])
    return np.random.default_rng(seed).permutation(v)


@functools.lru_cache(None)
def exp_inputs():
    rng = np.random.default_rng(101)
    k = np.arange(-1075, 1025, dtype=np.float64)
    return _shuffled([
        rng.uniform(-40, 40, 14000), rng.uniform(-745.2, 709.78, 14000), rng.uniform(-1e-3, 1e-3, 6000),
        10.0 ** rng.uniform(-300, -3, 1500) * rng.choice([-1.0, 1.0], 1500),
        k * LN2, (k + 0.5) * LN2, rng.uniform(-745.2, -708.0, 3000),   # (the last: subnormal results)
        _around(EXP_HI, 8), _around(EXP_LO, 8), _around(-745.1332191019412, 4), _around(-708.3964185322641, 4),
        [0.0, -0.0, NAN, INF, -INF, 5e-324, -5e-324, 1.0, -1.0, 710.0, 1000.0, -746.0, -1000.0, 1e308, -1e308],
    ], 1)


@functools.lru_cache(None)
def log_inputs():
    rng = np.random.default_rng(102)
    sub = (rng.integers(1, 1 << 52, 2000, dtype=np.uint64)).view(np.float64)
    return _shuffled([
        10.0 ** rng.uniform(-307, 308, 15000), rng.uniform(0.5, 2.0, 15000),
        1.0 + rng.uniform(0, 1e-6, 4000), 1.0 - rng.uniform(0, 1e-6, 4000),
        _around(math.sqrt(2.0), 50), _around(math.sqrt(0.5), 50), _around(math.sqrt(2.0) * 2.0 ** -1040, 50),
        _around(math.sqrt(2.0) * 2.0 ** 700, 20), _around(2.2250738585072014e-308, 8),
        sub, 2.0 ** rng.integers(-1074, 1024, 1000).astype(np.float64),
        [5e-324, 1e-323, DBL_MAX, math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 2.0, 0.5, 10.0,
         0.0, -0.0, -5e-324, -1.0, -INF, NAN, INF],
    ], 2)


@functools.lru_cache(None)
def acos_inputs():
    rng = np.random.default_rng(103)
    t = 10.0 ** rng.uniform(-16, -1, 6000)
    return _shuffled([
        rng.uniform(-1, 1, 24000), 0.5 + rng.uniform(-1e-9, 1e-9, 1500), -0.5 + rng.uniform(-1e-9, 1e-9, 1500),
        _around(0.5, 10), _around(-0.5, 10), [0.5 + 1e-9, 0.5 - 1e-9, -0.5 + 1e-9, -0.5 - 1e-9],
        1.0 - t, -(1.0 - t), 10.0 ** rng.uniform(-300, -1, 1000) * rng.choice([-1.0, 1.0], 1000),
        _around(1.0, 6), _around(-1.0, 6), [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, INF, -INF, NAN, 5e-324, -5e-324],
    ], 3)


def sigmoid_inputs(x0):
    """SINR arguments of the MI curve with midpoint x0: ordinary, dense at the midpoint, into both saturations, specials"""
    rng = np.random.default_rng(104)
    return _shuffled([rng.uniform(-60, 60, 12000), x0 + rng.uniform(-1e-3, 1e-3, 2000), rng.uniform(-5000, 5000, 4000),
                      _around(x0, 4), [0.0, -0.0, 1e308, -1e308, INF, -INF, NAN]], 4)


def inv_sigmoid_inputs():
    """MI averages y: ordinary, at 1/2 (the logarithm's zero), towards 1 (the cancellation in 1/y - 1) and towards 0"""
    rng = np.random.default_rng(105)
    return _shuffled([rng.uniform(1e-6, 1 - 1e-6, 12000), 0.5 + rng.uniform(-1e-6, 1e-6, 2000),
                      1.0 - 10.0 ** rng.uniform(-12, -1, 3000), 10.0 ** rng.uniform(-300, -1, 3000), _around(0.5, 4)], 5)


def _wide(rng, n, lo=-600, hi=600):
    return rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(lo, hi, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)


@functools.lru_cache(None)
def div_inputs():
    """(a, b): 2^18 random pairs, subnormal operands and quotients, quotients next to a rounding boundary, specials"""
    rng = np.random.default_rng(106)
    n = 1 << 18
    a, b = _wide(rng, n), _wide(rng, n, -400, 400)
    a[:8000] = rng.integers(1, 1 << 52, 8000, dtype=np.uint64).view(np.float64)         # subnormal dividends
    b[8000:16000] = rng.integers(1, 1 << 52, 8000, dtype=np.uint64).view(np.float64)    # subnormal divisors
    a[16000:24000] = _wide(rng, 8000, -1000, -600)                                       # subnormal quotients
    b[16000:24000] = _wide(rng, 8000, 20, 70)
    i, j = np.meshgrid(np.arange(200.0), np.arange(200.0))                               # (1 + i ulp) / (1 + j ulp): within an ulp
    a[24000:64000] = 1.0 + i.ravel() * 2.0 ** -52                                        # of a rounding boundary, (1+2^-52)/(1+2^-51) among them
    b[24000:64000] = 1.0 + j.ravel() * 2.0 ** -52
    sp = np.array([0.0, -0.0, 1.0, -1.0, INF, -INF, NAN, 5e-324, DBL_MAX, 2.2250738585072014e-308])
    sa, sb = np.meshgrid(sp, sp)
    a[64000:64100], b[64000:64100] = sa.ravel(), sb.ravel()
    p = np.random.default_rng(6).permutation(n)
    return a[p], b[p]


@functools.lru_cache(None)
def sqrt_inputs():
    rng = np.random.default_rng(107)
    r = np.abs(_wide(rng, 1 << 18, -1022, 1023))
    r[:8000] = rng.integers(1, 1 << 52, 8000, dtype=np.uint64).view(np.float64)          # subnormal arguments
    sq = rng.integers(1, 1 << 26, 8000).astype(np.float64) ** 2                          # perfect squares and their neighbours
    r[8000:16000], r[16000:24000], r[24000:32000] = sq, np.nextafter(sq, 0.0), np.nextafter(sq, INF)
    r[32000:32100] = 1.0 + np.arange(100.0) * 2.0 ** -52
    r[32100:32112] = [0.0, -0.0, -1.0, -5e-324, INF, -INF, NAN, 5e-324, DBL_MAX, 2.2250738585072014e-308, 2.0, 4.0]
    return np.random.default_rng(7).permutation(r)


@functools.lru_cache(None)
def rint_inputs():
    rng = np.random.default_rng(108)
    r = rng.uniform(-2000, 2000, 1 << 16)
    r[:4000] = rng.integers(-3000, 3000, 4000) + 0.5                                      # ties, to even
    r[4000:6000] = _wide(rng, 2000, 40, 70)
    r[6000:8000] = np.nextafter(rng.integers(-3000, 3000, 2000) + 0.5, rng.choice([-INF, INF], 2000))
    r[8000:8012] = [0.0, -0.0, -0.3, 0.3, 0.5, -0.5, INF, -INF, NAN, 4503599627370495.5, -4503599627370495.5, 5e-324]
    return np.random.default_rng(8).permutation(r)


@functools.lru_cache(None)
def fma_inputs():
    """(a, b, c): random triples; c = -RN(a b) (the result is the product's rounding error); subnormal results; specials"""
    rng = np.random.default_rng(109)
    n = 1 << 18
    a, b, c = _wide(rng, n, -300, 300), _wide(rng, n, -300, 300), _wide(rng, n, -600, 600)
    c[:60000] = -(a[:60000] * b[:60000])
    c[60000:90000] = -(a[60000:90000] * b[60000:90000]) * (1.0 + rng.integers(-4, 5, 30000) * 2.0 ** -52)
    a[90000:98000], b[90000:98000], c[90000:98000] = _wide(rng, 8000, -600, -500), _wide(rng, 8000, -560, -500), _wide(rng, 8000, -1074, -1040)
    sp = np.array([0.0, -0.0, 1.0, INF, -INF, NAN, 5e-324, DBL_MAX])
    sa, sb, sc = np.meshgrid(sp, sp, sp)
    a[98000:98512], b[98000:98512], c[98000:98512] = sa.ravel(), sb.ravel(), sc.ravel()
    p = np.random.default_rng(9).permutation(n)
    return a[p], b[p], c[p]


# ------------------------------------------------------------------ error in ulps against mpmath
def ulp_errors(got, xs, f, prec=220):
    """|got - f(x)| in ulps of the correctly rounded f(x) (the subnormal spacing below 2.2e-308), f evaluated by mpmath at `prec`
    bits; an overflowed `got` counts as 2^1024.  Every x must give a finite real f(x).  Returns the array of errors."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = prec
    fn = getattr(mp, f) if isinstance(f, str) else (lambda x: f(mp, x))
    top = mp.mpf(2) ** 1024
    err = np.zeros(len(xs))
    for i, (g, x) in enumerate(zip(got.tolist(), xs.tolist())):
        exact = fn(mp.mpf(x))
        cr = float(exact) if abs(exact) < top else math.copysign(INF, exact)
        ulp = math.ulp(min(abs(cr), DBL_MAX))
        assert g == g, (x, g)
        gm = mp.mpf(g) if abs(g) != INF else (top if g > 0 else -top)
        err[i] = float(abs(gm - exact) / ulp)
    return err


def same_bits(a, b):
    """f64 arrays equal bit for bit; a NaN matches a NaN of the same class (quiet / signalling), whatever sign and payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    ua, ub = a.view(np.uint64), b.view(np.uint64)
    nan = np.isnan(a)
    quiet = np.uint64(1 << 51)
    ok = np.where(nan, np.isnan(b) & ((ua & quiet) == (ub & quiet)), ua == ub)
    return ok
