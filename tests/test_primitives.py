"""The arithmetic primitives of the parity argument, on the CPU: include/rs_philox.h against the Random123 known answers and
an integer restatement, the stream draws against their formulas, include/rs_detmath.h against mpmath at 220 bits with the error
measured in ulps of the correctly rounded result.  tests/test_gpu_primitives.py compares the device with the same oracle entry
points bit for bit, on the same input sets (tests/primitives_util.py).

Measured worst errors (ulps; the argument in brackets), printed by the tests with -s:
    rs_exp 0.837 (-509.81)   rs_log 1.889 (1.06328)   rs_acos 1.090 (-0.53495)   rs_log10 3.892 (1 + 1.3e-7: the rounding of
    log times log10(e) on top of rs_log's own error)
"""
import math

import numpy as np
import pytest

import primitives_util as pu
from oracle import pyoracle as po
from ranslice.config import make_config

# the bounds: the worsts first measured on 45,000 arguments per function (0.84 / 1.85 / 1.13 / 3.96) plus a quarter to half an ulp
ULP_BOUND = {'exp': 1.0, 'log': 2.0, 'acos': 1.5, 'log10': 4.5}


# ------------------------------------------------------------------ Philox
KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, first two output words
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb)),
]


def test_philox_known_answers():
    for c, k, want in KAT:
        assert pu.philox4x32_10(c, k)[:2] == want
        assert tuple(int(v) for v in po.philox_block([c + k])[0]) == want


def test_philox_block_matches_integer_restatement():
    rng = np.random.default_rng(11)
    rows = rng.integers(0, 1 << 32, size=(2000, 6), dtype=np.uint64).astype(np.uint32)
    edges = []
    for w in range(6):  # 0 and 0xffffffff in each word, the others random / all at the same end
        for v in (0, pu.M32):
            r = rng.integers(0, 1 << 32, size=6, dtype=np.uint64)
            r[w] = v
            edges += [r, np.where(np.arange(6) == w, v, pu.M32 - v)]
    rows = np.concatenate([rows, np.array(edges, dtype=np.uint64).astype(np.uint32)])
    got = po.philox_block(rows)
    for r, g in zip(rows, got):
        assert pu.py_block(r) == (int(g[0]), int(g[1])), r


# ------------------------------------------------------------------ stream draws
N_DRAWS = 10000


def _streams():
    return pu.random_streams(np.random.default_rng(12), N_DRAWS)


def test_stream_uniform_and_pm1():
    st = _streams()
    uni, pm = po.stream_probe('UNIFORM', st), po.stream_probe('PM1', st)
    for row, (u, c), (s, c2) in zip(st, uni, pm):
        w = [int(v) for v in row]
        want = pu.py_uniform(w)
        assert u == want and 0.0 <= u < 1.0
        assert s == (-1.0 if want < 0.5 else 1.0)
        assert c == c2 == w[4] == (int(row[4]) + 1) & pu.M32   # one uniform consumed


@pytest.mark.parametrize('n', [1, 2, 3, 2 ** 31 - 1, 2 ** 40])
def test_stream_integers(n):
    st = _streams()
    got = po.stream_probe('INTEGERS', st, [float(n)])
    for row, (v, c) in zip(st, got):
        w = [int(x) for x in row]
        assert v == pu.py_integers(w, n) and 0 <= v < n
        assert c == w[4]


@pytest.mark.parametrize('T', [1, 2, 1000, 2 ** 31 - 1])
def test_walker_redraw(T):
    rows = np.random.default_rng(13).integers(0, 1 << 32, size=(N_DRAWS, 6), dtype=np.uint64).astype(np.uint32)
    rows[:200, 5] = pu.M32 - np.arange(200) % 2   # 1 + attempt wraps
    got = po.walker_redraw(rows, T)
    for r, (fi, fs) in zip(rows, got):
        a, b = pu.philox4x32_10((int(r[4]), (1 + int(r[5])) & pu.M32, int(r[3]), int(r[2])), (int(r[0]), int(r[1])))[:2]
        assert 0 <= fi < T and fi == (a * T) >> 32
        assert fs == (1 if b & 0x80000000 else -1)
        assert (fi, fs) == pu.py_walker(r, T)


def test_stream_exponential():
    st = _streams()
    scale = 37.5
    got = po.stream_probe('EXPONENTIAL', st, [scale])
    u = po.stream_probe('UNIFORM', st)[:, 0]
    want = (-po.detmath('LOG_INLINE', 1.0 - u)) * scale
    assert pu.same_bits(got[:, 0], want).all()
    assert (got[:, 1] == ((st[:, 4].astype(np.int64) + 1) & pu.M32)).all()


def test_stream_normal():
    st = _streams()
    loc, scale = 0.25, 10.0
    got = po.stream_probe('NORMAL', st, [loc, scale])
    v1s, r2s, ctrs = [], [], []
    for row in st:   # Marsaglia's polar method on the restated uniforms
        w = [int(x) for x in row]
        while True:
            v1 = 2.0 * pu.py_uniform(w) - 1.0
            v2 = 2.0 * pu.py_uniform(w) - 1.0
            r2 = v1 * v1 + v2 * v2
            if not (r2 >= 1.0 or r2 == 0.0):
                break
        v1s.append(v1), r2s.append(r2), ctrs.append(w[4])
    v1s, r2s = np.array(v1s), np.array(r2s)
    z = v1s * po.detmath('SQRT', po.detmath('DIV', -2.0 * po.detmath('LOG_INLINE', r2s), r2s))
    assert pu.same_bits(got[:, 0], loc + scale * z).all()
    assert (got[:, 1] == np.array(ctrs)).all()                      # two uniforms per attempt
    assert ((np.array(ctrs) - st[:, 4].astype(np.int64)) & pu.M32).max() > 2  # (some stream did reject a pair)


def test_macro_cell_stream_matches_the_tape_entry_point():
    """rso_macro_cell_stream against rso_macro_cell (pinned to the reference by fixture G6) fed with the restated draws: the
    point's uniforms, then the shadowing normal by Marsaglia's method as in test_stream_normal"""
    cfg = make_config(0)
    rng = np.random.default_rng(14)
    cases = [(123456789123, 1, 7, 0), (2 ** 64 - 1, 5, 0, 0xfffffffe)]
    cases += [(int(rng.integers(0, 1 << 63)), int(rng.integers(0, 6)), int(rng.integers(0, 300)), int(c))
              for c in list(rng.integers(0, 5000, 300)) + [0xfffffff0] * 50 + [0xfffffffd] * 50]
    most = 0
    for key, sl, serial, ctr in cases:
        v, after = po.macro_cell_stream(cfg, key, sl, serial, ctr)
        st = [key & pu.M32, key >> 32, sl, serial, ctr]
        uv = []
        while True:   # generate_xy: pairs until one lies in the cell (rso_macro_cell takes the first such pair itself)
            uv += [pu.py_uniform(st), pu.py_uniform(st)]
            if _in_cell(*uv[-2:]):
                break
        while True:
            v1 = 2.0 * pu.py_uniform(st) - 1.0
            v2 = 2.0 * pu.py_uniform(st) - 1.0
            r2 = v1 * v1 + v2 * v2
            if not (r2 >= 1.0 or r2 == 0.0):
                break
        one = lambda op, x, b=None: float(po.detmath(op, [x], b)[0])
        z = v1 * one('SQRT', one('DIV', -2.0 * one('LOG_INLINE', r2), [r2]))
        want, used = po.macro_cell(cfg, np.array(uv), 0.0 + 10.0 * z)
        assert used == len(uv)
        assert np.float64(v).tobytes() == np.float64(want).tobytes(), (key, sl, serial, ctr, v, want)
        assert after == st[4]               # the counter advanced by exactly the uniforms consumed
        most = max(most, (after - ctr) & pu.M32)
    assert most >= 8                        # (rejections occurred)


def _in_cell(x, y):
    """generate_xy's hexagonal cell (channel_models.py:50-76)"""
    def line(x1, y1, x2, y2):
        m = (y2 - y1) / (x2 - x1)
        return m * x + (-m * x1 + y1)
    return y > line(0, 0.5, 0.25, 0) and y > line(0.75, 0, 1, 0.5) and y < line(0, 0.5, 0.25, 1) and y < line(0.75, 1, 1, .5)


# ------------------------------------------------------------------ rs_detmath.h against mpmath
def _finite_case(f, x):
    if f == 'exp':
        return pu.EXP_LO <= x <= pu.EXP_HI
    if f in ('log', 'log10'):
        return 0.0 < x < pu.INF
    return -1.0 < x < 1.0


def _measure(f, op, xs):
    got = po.detmath(op, xs)
    sel = np.array([_finite_case(f, x) for x in xs.tolist()])
    err = pu.ulp_errors(got[sel], xs[sel], f)
    w = int(np.argmax(err))
    print('rs_%s: worst error %.3f ulp at x = %r over %d arguments' % (f, err[w], float(xs[sel][w]), int(sel.sum())))
    return got, err, float(xs[sel][w])


def test_exp_against_mpmath():
    xs = pu.exp_inputs()
    got, err, at = _measure('exp', 'EXP_INLINE', xs)
    assert err.max() <= ULP_BOUND['exp'], (err.max(), at)
    for x, g in zip(xs.tolist(), got.tolist()):
        if x != x:
            assert g != g
        elif x > pu.EXP_HI:
            assert g == pu.INF, x
        elif x < pu.EXP_LO:
            assert g == 0.0 and math.copysign(1.0, g) == 1.0, x
    assert po.detmath('EXP_INLINE', [0.0, -0.0]).tolist() == [1.0, 1.0]


def test_exp_nonpos_is_exp():
    xs = pu.exp_inputs()
    xs = np.concatenate([xs[xs <= 0.0], [-745.2, math.nextafter(-745.2, -pu.INF), -745.3, -800.0, -1e300, -pu.INF]])
    assert len(xs) > 20000 and (xs < -745.2).sum() >= 5
    assert po.detmath('EXP_NONPOS', xs).tobytes() == po.detmath('EXP_INLINE', xs).tobytes()


@pytest.mark.parametrize('f,op', [('log', 'LOG_INLINE'), ('log10', 'LOG10')])
def test_log_against_mpmath(f, op):
    xs = pu.log_inputs()
    got, err, at = _measure(f, op, xs)
    assert err.max() <= ULP_BOUND[f], (err.max(), at)
    for x, g in zip(xs.tolist(), got.tolist()):
        if x != x or x < 0.0:
            assert g != g, x
        elif x == 0.0:
            assert g == -pu.INF
        elif x == pu.INF:
            assert g == pu.INF
    assert po.detmath(op, [1.0]).tobytes() == np.array([0.0]).tobytes()


def test_acos_against_mpmath():
    xs = pu.acos_inputs()
    got, err, at = _measure('acos', 'ACOS', xs)
    assert err.max() <= ULP_BOUND['acos'], (err.max(), at)
    for x, g in zip(xs.tolist(), got.tolist()):
        if x != x or abs(x) > 1.0:
            assert g != g, x
    assert po.detmath('ACOS', [1.0, -1.0, 0.0]).tolist() == [0.0, math.pi, math.pi / 2]


def test_scalar_entry_points_agree_with_the_batched_one():
    L = po.lib()
    for name, op, xs in (('rso_exp', 'EXP_INLINE', pu.exp_inputs()), ('rso_log', 'LOG_INLINE', pu.log_inputs()),
                         ('rso_acos', 'ACOS', pu.acos_inputs())):
        xs = xs[:2000]
        one = np.array([getattr(L, name)(float(x)) for x in xs])
        assert pu.same_bits(one, po.detmath(op, xs)).all()
    for op in ('EXP_OOL', 'EXP2_OOL'):
        assert po.detmath(op, pu.exp_inputs()[:500]).tobytes() == po.detmath('EXP_INLINE', pu.exp_inputs()[:500]).tobytes()


# rs_sigmoid: y = 1 / (1 + exp(t)), t = (-k) (x - x0).  Against the real value of the same formula at the same doubles, absolute:
#   t carries two roundings (2^-52 relative), which sigma turns into |t| sigma (1 - sigma) 2^-52 <= 0.224 x 2.2e-16 = 5.0e-17;
#   rs_exp is within 1 ulp (above): sigma (1 - sigma) 2^-52 <= 5.6e-17;  the rounding of 1 + e: sigma 2^-53 <= 1.1e-16;
#   the divide: half an ulp of y < 1, <= 5.6e-17.  Sum 2.8e-16.
SIGMOID_ABS = 2.8e-16


@pytest.mark.parametrize('mod', [0, 1, 2])
def test_sigmoid_against_mpmath(mod):
    import mpmath
    cfg = make_config(0)
    x0, k = cfg.mi_x0[mod], cfg.mi_k[mod]
    xs = pu.sigmoid_inputs(x0)
    got = po.detmath('SIGMOID', xs, params=[x0, k])
    mp = mpmath.mp.clone()
    mp.prec = 220
    worst = 0.0
    for x, g in zip(xs.tolist(), got.tolist()):
        if x != x:
            assert g != g
            continue
        if abs(x) == pu.INF:
            assert g == (1.0 if x > 0 else 0.0)
            continue
        exact = 1 / (1 + mp.exp(-mp.mpf(k) * (mp.mpf(x) - mp.mpf(x0))))
        worst = max(worst, float(abs(mp.mpf(g) - exact)))
        assert 0.0 <= g <= 1.0
    print('rs_sigmoid (x0 = %g, k = %g): worst absolute error %.3g' % (x0, k, worst))
    assert worst <= SIGMOID_ABS, worst


# rs_inv_sigmoid: x = -(1/k) L + x0, L = log(w), w = 1/y - 1.  The problem is ill-conditioned where y -> 1 (w cancels) and the
# bound follows the condition number: 1/y is rounded (2^-53 / y absolute), the subtraction rounds again (2^-53 w), so
# dw / w <= 2^-53 (1 + 1 / (1 - y)); rs_log adds 2 ulp of L (above) = 2^-51 |L|; 1/k and the product round once each
# (2^-52 |L| / k together); the final sum rounds to half an ulp of x (2^-53 |x|).  First order, so 2 % is added:
#   |x - exact| <= 1.02 x [ (2^-53 (1 + 1 / (1 - y)) + (2^-51 + 2^-52) |L|) / k + 2^-53 |x| ]
@pytest.mark.parametrize('mod', [0, 1, 2])
def test_inv_sigmoid_against_mpmath(mod):
    import mpmath
    cfg = make_config(0)
    x0, k = cfg.mi_x0[mod], cfg.mi_k[mod]
    ys = pu.inv_sigmoid_inputs()
    got = po.detmath('INV_SIGMOID', ys, params=[x0, k])
    mp = mpmath.mp.clone()
    mp.prec = 220
    worst = 0.0
    for y, g in zip(ys.tolist(), got.tolist()):
        L = mp.log(1 / mp.mpf(y) - 1)
        exact = -(1 / mp.mpf(k)) * L + mp.mpf(x0)
        bound = 1.02 * ((2.0 ** -53 * (1 + 1 / (1 - y)) + (2.0 ** -51 + 2.0 ** -52) * abs(float(L))) / k + 2.0 ** -53 * abs(float(exact)))
        e = float(abs(mp.mpf(g) - exact))
        worst = max(worst, e / bound)
        assert e <= bound, (y, g, e, bound)
    print('rs_inv_sigmoid (x0 = %g, k = %g): worst error %.3f of its condition-number bound' % (x0, k, worst))
