"""The arithmetic primitives of the parity argument ON THE DEVICE, one by one: rs_dev_probe of the test build
(csrc/rs_probe.hip) evaluates a production device function per element, and every f64 value must equal the oracle's bit for bit
on the input sets of tests/test_primitives.py, shuffled so that special, seam and ordinary arguments share a wave.  The float32
chains of the reception test are held to the budgets rx_fast_setup (csrc/rs_api.hip) derives its guard bands from;
each of those two tests prints its measured worst error (-s) and quotes it when it fails.

Measured on an MI355X (the table in DESIGN.md §4): fast_sigmoid's worst absolute error 1.07e-7 .. 1.15e-7 over the three
modulations and four nominal SINRs (budget 4e-7); the s* chain 9.9e-7 / A at u = 1.8e-4 (budget 6.2e-6 / A).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import primitives_util as pu
from oracle import pyoracle as po
from ranslice.config import make_config

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 65, 4097, None]   # None: the whole set


def probe(op, inp, out_dtype, out_shape, params=()):
    from ranslice import _lib
    L = _lib.load(dev=True)
    inp = np.ascontiguousarray(inp)
    out = np.zeros(out_shape, dtype=out_dtype)
    n = out_shape[0] if op != 'TEAM_PAIRWISE' else out_shape[0] * 8
    p = np.zeros(4, dtype=np.float64)
    p[:len(params)] = params
    rc = L.rs_dev_probe(0, po.OP[op], inp.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), int(n),
                        p.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0, 'rs_dev_probe(%s) returned %d' % (op, rc)
    return out


def unary(op, xs, params=()):
    return probe(op, xs, np.float64, (len(xs),), params)


def assert_bits(dev, ref, xs, what):
    ok = pu.same_bits(dev, ref)
    if not ok.all():
        i = int(np.argmin(ok))
        raise AssertionError('%s: %d of %d differ; first at %d: x = %r device %r (%#x) oracle %r (%#x)' % (
            what, int((~ok).sum()), len(ok), i, np.asarray(xs).ravel()[i] if xs is not None else None,
            dev[i], int(np.asarray(dev[i:i + 1]).view(np.uint64)[0]), ref[i], int(np.asarray(ref[i:i + 1]).view(np.uint64)[0])))


def _head(a, n):
    return a if n is None else a[:n]


@functools.lru_cache(None)
def _ref(op, which):
    """the oracle's values on a whole input set, computed once"""
    cfg = make_config(0)
    if which.startswith('sig'):
        mod = int(which[-1])
        x0, k = cfg.mi_x0[mod], cfg.mi_k[mod]
        xs = pu.sigmoid_inputs(x0) if which.startswith('sigm') else pu.inv_sigmoid_inputs()
        return xs, po.detmath(op, xs, params=[x0, k]), (x0, k)
    xs = {'exp': pu.exp_inputs, 'log': pu.log_inputs, 'acos': pu.acos_inputs, 'sqrt': pu.sqrt_inputs, 'rint': pu.rint_inputs}[which]()
    if op == 'EXP_NONPOS':
        xs = xs[(xs <= 0.0)]
    return xs, po.detmath(op, xs), ()


# ------------------------------------------------------------------ the elementary functions, every code shape
@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('op,which', [
    ('EXP_OOL', 'exp'), ('EXP_INLINE', 'exp'), ('EXP_NONPOS', 'exp'), ('LOG_OOL', 'log'), ('LOG_INLINE', 'log'), ('LOG10', 'log'),
    ('ACOS', 'acos'), ('SQRT', 'sqrt'), ('RINT', 'rint'),
    ('SIGMOID', 'sigm0'), ('SIGMOID', 'sigm1'), ('SIGMOID', 'sigm2'), ('INV_SIGMOID', 'sigi0'), ('INV_SIGMOID', 'sigi1'),
    ('INV_SIGMOID', 'sigi2')])
def test_unary_matches_oracle(op, which, n):
    xs, ref, params = _ref(op, which)
    xs, ref = _head(xs, n), _head(ref, n)
    assert_bits(unary(op, xs, params), ref, xs, op)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('op,which', [('EXP2_OOL', 'exp'), ('SIGMOID2', 'sigm0'), ('SIGMOID2', 'sigm1'), ('SIGMOID2', 'sigm2')])
def test_two_argument_forms_match_oracle(op, which, n):
    """element i rides in the first slot of thread i and in the second slot of thread n-1-i, beside another argument each time"""
    xs, ref, params = _ref(op, which)
    xs, ref = _head(xs, n), _head(ref, n)
    out = probe(op, xs, np.float64, (len(xs), 2), params)
    assert_bits(out[:, 0], ref, xs, op + ' first slot')
    assert_bits(out[::-1, 1], ref, xs, op + ' second slot')


@pytest.mark.parametrize('n', SIZES)
def test_divide_matches_oracle(n):
    a, b = pu.div_inputs()
    a, b = _head(a, n), _head(b, n)
    assert_bits(probe('DIV', np.concatenate([a, b]), np.float64, (len(a),)), po.detmath('DIV', a, b), a, 'a / b')


@pytest.mark.parametrize('n', SIZES)
def test_fma_matches_oracle(n):
    a, b, c = (_head(v, n) for v in pu.fma_inputs())
    assert_bits(probe('FMA', np.concatenate([a, b, c]), np.float64, (len(a),)), po.detmath('FMA', a, np.concatenate([b, c])), a, 'fma')


# ------------------------------------------------------------------ Philox and the draws
def test_philox_known_answers_and_restatement():
    rng = np.random.default_rng(21)
    rows = rng.integers(0, 1 << 32, size=(1 << 16, 6), dtype=np.uint64).astype(np.uint32)
    kat = [((0, 0, 0, 0, 0, 0), (0x6627e8d5, 0xe169c58d)), ((pu.M32,) * 6, (0x408f276d, 0x41c83b0e)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb))]
    for i, (r, _) in enumerate(kat):
        rows[1000 * i + 7] = r
    got = probe('PHILOX', rows, np.uint32, (len(rows), 2))
    for i, (_, want) in enumerate(kat):
        assert tuple(int(v) for v in got[1000 * i + 7]) == want
    want = np.array([pu.py_block(r) for r in rows.tolist()], dtype=np.uint32)
    assert (got == want).all(), np.argwhere(got != want)[:4]


@pytest.mark.parametrize('kind,params', [('UNIFORM', ()), ('PM1', ()), ('EXPONENTIAL', (37.5,)), ('NORMAL', (0.25, 10.0)),
                                         ('INTEGERS', (1,)), ('INTEGERS', (2,)), ('INTEGERS', (3,)), ('INTEGERS', (2 ** 31 - 1,)),
                                         ('INTEGERS', (2 ** 40,))])
def test_stream_draws_match_oracle(kind, params):
    st = pu.random_streams(np.random.default_rng(22), 10000 + 37)
    dev = probe(kind, st, np.float64, (len(st), 2), params)
    ref = po.stream_probe(kind, st, params)
    assert_bits(dev[:, 0], ref[:, 0], st[:, 4], kind)
    assert (dev[:, 1] == ref[:, 1]).all(), 'ctr after ' + kind


@pytest.mark.parametrize('T', [1, 2, 1000, 2 ** 31 - 1])
def test_walker_redraw_matches_oracle(T):
    rows = np.random.default_rng(23).integers(0, 1 << 32, size=(10000 + 37, 6), dtype=np.uint64).astype(np.uint32)
    rows[:200, 5] = pu.M32 - np.arange(200) % 2
    dev = probe('WALKER', rows, np.int32, (len(rows), 2), (T,))
    assert (dev == po.walker_redraw(rows, T)).all()
    assert (dev[:, 0] >= 0).all() and (dev[:, 0] < T).all()


def test_macro_cell_draw_matches_oracle():
    """macro_cell_draw spells the shadowing normal out with the in-line logarithm; the oracle calls rs_stream_normal"""
    cfg = make_config(0)
    rng = np.random.default_rng(24)
    n = 20000
    st = rng.integers(0, 1 << 32, size=(n, 5), dtype=np.uint64).astype(np.uint32)
    st[:, 2] = rng.integers(0, 6, n)
    st[: n // 2, 3] = rng.integers(1, 300, n // 2)
    st[:, 4] = np.where(np.arange(n) % 2 == 0, 0, 0xfffffff0)
    st[::10, 4] = 0xfffffffd   # (the counter wraps inside every one of these)
    dev = probe('MACRO_CELL', st, np.float64, (n, 2), (cfg.prop_A, cfg.prop_B))
    ref = np.array([po.macro_cell_stream(cfg, int(r[0]) | (int(r[1]) << 32), r[2], r[3], r[4]) for r in st.tolist()])
    assert_bits(dev[:, 0], ref[:, 0], st[:, 4], 'macro_cell_draw')
    assert (dev[:, 1] == ref[:, 1]).all()
    assert (ref[::10, 1] < 100).all()   # those counters did wrap


# ------------------------------------------------------------------ numpy's pairwise order across lanes and teams
SPECIAL_LEN = [0, 1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 200, 249, 250, 255, 256]


@functools.lru_cache(None)
def _ill_conditioned():
    """2^16 values of both signs over sixteen decades: another order of summation changes the low bits of nearly every sum"""
    rng = np.random.default_rng(25)
    return 10.0 ** rng.uniform(-8, 8, 1 << 16) * rng.choice([-1.0, 1.0], 1 << 16)


# team_pairwise has eight teams to a wave, so the special lengths cannot all share one: the first waves are built by hand to put
# the neighbours of each split (8, 16, 128, 136, 256) and idle teams side by side, the others take four specials each in rotation
HAND_TEAM_WAVES = [[127, 128, 129, 0, 135, 136, 137, 0], [7, 8, 9, 0, 15, 16, 17, 1], [249, 250, 0, 255, 256, 200, 128, 129],
                   [256, 0, 1, 136, 0, 8, 137, 127]]


def _lengths(rng, rows, per_wave):
    """`rows` lengths, `per_wave` of them to a wavefront (64 lanes, or 8 teams).  Lanes: every wave holds all the special lengths.
    Teams: HAND_TEAM_WAVES first, then four specials per wave in rotation.  Every length 1..256 occurs somewhere; the rest are
    random in 0..256."""
    lens = rng.integers(0, 257, rows)
    every = list(range(1, 257))
    for w in range((rows + per_wave - 1) // per_wave):
        lo, hi = w * per_wave, min(rows, (w + 1) * per_wave)
        if per_wave == 8 and w < len(HAND_TEAM_WAVES):
            lens[lo:hi] = HAND_TEAM_WAVES[w]
            continue
        pos = lo + rng.permutation(hi - lo)
        k = min(len(SPECIAL_LEN), (hi - lo) // 2) if per_wave >= 2 * len(SPECIAL_LEN) else max(1, (hi - lo) // 2)
        sp = [SPECIAL_LEN[(w * k + i) % len(SPECIAL_LEN)] for i in range(k)]
        lens[pos[:k]] = sp
        for p in pos[k:k + max(3, per_wave // 8)]:
            if every:
                lens[p] = every.pop()
        if per_wave == 8 and w % 2 == 0:
            lens[pos[-1]] = 0   # an idle team between busy ones
    assert not every and set(range(1, 257)) <= set(lens.tolist())
    return lens.astype(np.int32)


def _pairwise_case(rows, per_wave, seed):
    vec = _ill_conditioned()
    rng = np.random.default_rng(seed)
    lens = _lengths(rng, rows, per_wave)
    offs = (rng.integers(0, 1 << 62, rows) % (len(vec) - lens + 1)).astype(np.int32)
    offs[:8] = len(vec) - lens[:8]   # spans that end with the vector
    ref = np.array([po.pairwise_sum(vec[o:o + n]) for o, n in zip(offs.tolist(), lens.tolist())])
    inp = np.concatenate([np.stack([lens, offs], axis=1).ravel().view(np.uint8), vec.view(np.uint8)])
    return vec, lens, ref, inp


def test_lane_pairwise_matches_oracle():
    rows = 64 * 64 + 37   # 64 full waves and a partial one; every wave holds all the special lengths next to random ones
    vec, lens, ref, inp = _pairwise_case(rows, 64, 26)
    dev = probe('LANE_PAIRWISE', inp, np.float64, (rows,), (len(vec),))
    assert_bits(dev, ref, lens, 'lane_pairwise (x = length)')
    # the order matters on this vector: a plain left-to-right sum differs for most spans
    naive = np.array([np.cumsum(vec[:n])[-1] if n else 0.0 for n in lens.tolist()[:200]])
    assert (naive != np.array([po.pairwise_sum(vec[:n]) for n in lens.tolist()[:200]])).mean() > 0.5


def test_team_pairwise_matches_oracle():
    teams = 2048 + 3      # 8 teams to a wave: busy teams of every length next to idle ones (length 0), the last wave partial
    vec, lens, ref, inp = _pairwise_case(teams, 8, 27)
    assert 50 < (lens == 0).sum() < teams // 4
    dev = probe('TEAM_PAIRWISE', inp, np.float64, (teams,), (len(vec),))
    assert_bits(dev, ref, lens, 'team_pairwise (x = length)')


# ------------------------------------------------------------------ the float32 chains of the reception test
# The budgets are the project's own (csrc/rs_api.hip, above rx_fast_setup): 4e-7 absolute per sigmoid, 6.2e-6 / A for s*.
FAST_SIGMOID_BUDGET = 4.0e-7
RX_DQ_BUDGET = 6.2e-6   # over A
LOG2E = 1.4426950408889634


@pytest.mark.parametrize('nominal', [-30.0, 0.0, 17.3, 60.0])
@pytest.mark.parametrize('mod', [0, 1, 2])
def test_fast_sigmoid_within_its_budget(mod, nominal):
    cfg = make_config(0)
    x0, k = cfg.mi_x0[mod], cfg.mi_k[mod]
    rng = np.random.default_rng(28 + mod)
    n = 1 << 20
    c = x0 - nominal   # the sample at which the curve is at its midpoint
    v = np.concatenate([c + rng.uniform(-40, 40, n // 2), c + rng.normal(0, 3, n // 4), rng.uniform(-1000, 1000, n // 4 - 8),
                        [c, -1000.0, 1000.0, 0.0, -0.0, c + 300, c - 300, c + 0.001]])
    v = np.clip(v, -1000.0, 1000.0).astype(np.float32)
    v = rng.permutation(v)
    got = probe('FAST_SIGMOID', v, np.float32, (n,), (x0, k, nominal))
    assert not np.isnan(got).any()
    z = k * (v.astype(np.float64) + nominal - x0)
    with np.errstate(over='ignore'):
        exact = 1.0 / (1.0 + np.exp(-z))
    err = np.abs(got.astype(np.float64) - exact)
    w = int(np.argmax(err))
    # v_exp_f32 overflows above 2^128 and 1 + e is 1 below 2^-24: at |z| log2(e) >= 160 the limits must come out exactly
    sat = np.abs(z) * LOG2E >= 160.0
    assert sat.sum() > 1000 and (z[sat] > 0).any() and (z[sat] < 0).any()
    print('fast_sigmoid mod %d nominal %g: worst |error| %.3g at v = %r' % (mod, nominal, err[w], float(v[w])))
    assert (got[sat] == np.where(z[sat] > 0, np.float32(1.0), np.float32(0.0))).all(), 'saturated arguments'
    assert err[w] <= FAST_SIGMOID_BUDGET, 'worst |fast_sigmoid - sigmoid| = %.3g at v = %r (budget %.1g)' % (
        err[w], float(v[w]), FAST_SIGMOID_BUDGET)


def test_rx_threshold_chain_within_its_budget():
    A, B = po.mcs_factors()
    rng = np.random.default_rng(31)
    n = 1 << 18
    d = 10.0 ** rng.uniform(-9, -2, n // 4)
    u = np.concatenate([rng.uniform(1e-4, 1 - 1e-4, n - 2 * len(d) - 2), [1e-4, 1 - 1e-4], 0.5 + d, 0.5 - d])
    u = rng.permutation(u)
    got = probe('RX_DQ', u, np.float32, (n,), (A, B))
    exact = (B - np.log((1.0 - u) / u)) / A
    err = np.abs(got.astype(np.float64) - exact)
    w = int(np.argmax(err))
    print('s* chain: worst |dq - exact| = %.3g = %.3g / A at u = %r' % (err[w], err[w] * A, float(u[w])))
    assert err[w] <= RX_DQ_BUDGET / A, 'worst |dq - exact| = %.3g / A at u = %r (budget %.2g / A)' % (err[w] * A, float(u[w]), RX_DQ_BUDGET)


def test_probe_rejects_bad_calls():
    from ranslice import _lib
    L = _lib.load(dev=True)
    x = np.zeros(8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.rs_dev_probe(0, 999, vp(x), vp(x), 8, None) == _lib.RS_EINVAL
    assert L.rs_dev_probe(0, -1, vp(x), vp(x), 8, None) == _lib.RS_EINVAL
    assert L.rs_dev_probe(0, 0, vp(x), vp(x), 0, None) == _lib.RS_EINVAL
    assert L.rs_dev_probe(0, 0, vp(x), vp(x), (1 << 22) + 1, None) == _lib.RS_EINVAL
    bad = np.array([257, 0, 4, 6], dtype=np.int32)   # a length above 256; a span past the end of an 8-element vector
    p = np.array([8.0, 0, 0, 0])
    assert L.rs_dev_probe(0, po.OP['LANE_PAIRWISE'], vp(bad), vp(x), 1, p.ctypes.data_as(C.POINTER(C.c_double))) == _lib.RS_EINVAL
    assert L.rs_dev_probe(0, po.OP['LANE_PAIRWISE'], vp(bad[2:]), vp(x), 1, p.ctypes.data_as(C.POINTER(C.c_double))) == _lib.RS_EINVAL
