"""Adversarial fading tables for the channel estimate by guard band, and its arithmetic restated in numpy.

The step kernel (rs_embb.hip, the est_fast block) decides round(mean SINR over the slice's RBs) from two entries of a per-column
prefix-sum table, (PS[lo + n] - PS[lo]) / n + nominal, unless that mean lies within est_band = 1e-9 of a half-integer or is 3e4 or
more in magnitude; then numpy's pairwise sum of the samples decides, as in the oracle and the reference (slice_ran.py:43-45).  The
table and the band come from upload_fading (rs_api.hip).  The decision can only go wrong where a mean sits at a half-integer, so the
two families below put nearly all of their columns there:

  family A   100 PRB rows (a 200-PRB carrier wraps them, channel_models.py:144-148), 256 time columns.  Column t holds
             c_t + 0.5 + sigma_t U(-1, 1) with an integer c_t in [-60, -41]; a UE whose path loss is clamped has the nominal SINR
             61.0 exactly (30 - 70 + 110 - 9), so its means sit at half-integers between 1.5 and 20.5, across the MCS thresholds.
  family B   256 PRB rows, the build's maximum.  Rows 0..239 hold U(990, 1000) -- a prefix of 2.4e5 in front of the slice, the
             worst case of the band's budget (2^-52 P smax) --, rows 240..255 the half-integer columns, c_t in [-65, -41].  In the
             odd columns the prefix ends just above 2^17 instead (_binade_prefix): there the fast mean lands on the WRONG SIDE
             of the half, not merely on it.

The kind of a column goes by its index t (COLUMN KINDS below): sigma = 0 (exact ties), a constant offset just outside the band,
plainly random samples, and for the rest sigma log-uniform -- in the even columns over the whole range (1e-16..1e-7 in A, 1e-14..1e-8
in B), in the odd ones over the decades of the arithmetic's own error (1e-15..1e-12, 1e-13..3e-11).  Family B also
carries one sample of exactly 1000.0 and one of exactly -1000.0: upload_fading keeps the short paths for smax <= 1e3.  No sample
exceeds 1e3 in magnitude.

Everything is a pure function of the seed; the tables are made at test time and need no fixture.
"""
from collections import namedtuple

import numpy as np

from ranslice.config import make_config

N_COLS = 256
EST_BAND = 1.0e-9        # rs_api.hip: upload_fading (d.est_band)
MEAN_BOUND = 3.0e4       # rs_embb.hip: est_fast block
SMAX = 1.0e3             # rs_api.hip: upload_fading (the short paths are kept for smax <= 1e3)
NOMINAL = 61.0           # macro_cell with the path loss clamped at the MCL: 30 - 70 - (-110) - 9
OFFSETS = (1.5e-9, -1.5e-9, 3e-9, -3e-9, 1e-8, -1e-8, 1e-7, -1e-7)   # constant distances from the half, just outside the band

SCRIPT_A = ((40, 40, 40, 40, 40), (200, 0, 0, 0, 0), (1, 2, 3, 5, 8), (13, 7, 1, 0, 179), (129, 0, 71, 0, 0), (33, 33, 33, 33, 33),
            (64, 64, 64, 8, 0))
SCRIPT_B = ((240, 1, 2, 3, 10), (240, 4, 6, 3, 3), (224, 16, 8, 4, 4), (250, 1, 1, 1, 3))
B_PREFIX_ROWS = 240

Census = namedtuple('Census', 'spans in_band ties differ differ_off_tie differ_outside near worst reach')


# ---- COLUMN KINDS -----------------------------------------------------------------------------------------------------------------
def _kind(t):
    if t % 16 == 0:
        return 'tie'                 # 16 columns: sigma = 0, every mean an exact tie
    if t % 32 == 5:
        return 'offset'              # 8 columns, one per entry of OFFSETS
    if t % 64 == 9:
        return 'random'              # 4 columns
    return 'noisy'


def _half_integer_rows(rng, rows, c_lo, c_hi, sig_wide, sig_sharp):
    """[rows][N_COLS]: the half-integer columns of either family"""
    out = np.empty((rows, N_COLS))
    for t in range(N_COLS):
        c = float(rng.integers(c_lo, c_hi + 1))
        u = rng.uniform(-1.0, 1.0, size=rows)
        # odd columns: sigma in the decades of the arithmetic's own error, where the roundings disagree; even ones: the wide range
        lo, hi = sig_sharp if t % 2 else sig_wide
        sigma = 10.0 ** rng.uniform(np.log10(lo), np.log10(hi))
        kind = _kind(t)
        if kind == 'tie':
            out[:, t] = c + 0.5
        elif kind == 'offset':
            out[:, t] = c + 0.5 + OFFSETS[t // 32]
        elif kind == 'random':
            out[:, t] = rng.uniform(-70.0, -30.0, size=rows)
        else:
            out[:, t] = c + 0.5 + sigma * u
    return out


def family_a(seed=20261021):
    """three tables [100 PRB rows][256 time columns]"""
    return [_half_integer_rows(np.random.default_rng([seed, f]), 100, -60, -41, (1e-16, 1e-7), (1e-15, 1e-12)) for f in range(3)]


def _binade_prefix(rng, col):
    """A prefix that ends just above 2^17: the slice's samples (about -50 each) take the running sum back below it, so PS[lo] and
    PS[hi] are rounded on different grids (2^-35 and 2^-36).  Where both lie in one binade the rounding is monotone -- PS[hi] - PS[lo]
    never has the wrong sign, it can only be a false tie, which the kernel hands to the pairwise sum whatever the band -- so these
    are the columns where the fast mean lands on the wrong side of the half, by up to 2.2e-11.  53 of rows 0..237 change sign
    (sum about 131,340); the last two rows make up the rest, well inside the 1e3 limit."""
    neg = rng.choice(B_PREFIX_ROWS - 2, size=53, replace=False)
    col[neg] = -col[neg]
    target = 131072.0 + rng.uniform(5.0, 600.0)
    col[-2:] = (target - float(np.sum(col[:-2]))) / 2.0


def family_b(seed=20261022):
    """three tables [256 PRB rows][256 time columns]: a large prefix, a narrow band of half-integer rows behind it"""
    tabs = []
    for f in range(3):
        rng = np.random.default_rng([seed, f])
        tab = np.empty((256, N_COLS))
        tab[:B_PREFIX_ROWS] = rng.uniform(990.0, 1000.0, size=(B_PREFIX_ROWS, N_COLS))
        tab[B_PREFIX_ROWS:] = _half_integer_rows(rng, 256 - B_PREFIX_ROWS, -65, -41, (1e-14, 1e-8), (1e-13, 3e-11))
        for t in range(1, N_COLS, 2):
            _binade_prefix(rng, tab[:B_PREFIX_ROWS, t])
        tabs.append(tab)
    tabs[0][17, 40] = 1000.0        # smax == 1e3 exactly: the short paths stay on
    tabs[1][101, 77] = -1000.0
    return tabs


# ---- the arithmetic, restated -----------------------------------------------------------------------------------------------------
def carrier(table, n_prbs):
    """[time][PRB] with the reference's row wrap, as rs_load_fading stores a trace"""
    table = np.asarray(table, dtype=np.float64)
    P = max(n_prbs, table.shape[0])
    assert P <= 2 * table.shape[0]
    return np.ascontiguousarray(table[np.arange(P) % table.shape[0]].T)


def prefix_table(cols):
    """[time][P + 1]: per column the prefix sums of its samples, accumulated in long double and rounded once (upload_fading)"""
    ps = np.zeros((cols.shape[0], cols.shape[1] + 1))
    ps[:, 1:] = np.cumsum(cols.astype(np.longdouble), axis=1).astype(np.float64)
    return ps


def fast_mean(ps, lo, n, nom):
    """the kernel's mean of every column over [lo, lo + n)"""
    return (ps[:, lo + n] - ps[:, lo]) / float(n) + nom


def exact_mean(cols, lo, n, nom):
    """numpy's own mean of samples + nominal, column by column: the pairwise sum of a contiguous vector"""
    blk = np.ascontiguousarray(cols[:, lo:lo + n] + nom)
    return np.array([np.sum(blk[t]) for t in range(blk.shape[0])]) / float(n)


def half_distance(mean):
    """distance of a mean from the nearest half-integer"""
    return 0.5 - np.abs(mean - np.rint(mean))


def in_band(mean):
    """the kernel's `!sure`: the pairwise sum decides"""
    return ~((np.abs(mean - np.rint(mean)) < 0.5 - EST_BAND) & (np.abs(mean) < MEAN_BOUND))


def spans_of(script):
    """the distinct (first PRB, width) of the slices of every action row"""
    out = []
    for row in script:
        lo = 0
        for n in row:
            if n > 0 and (lo, n) not in out:
                out.append((lo, n))
            lo += n
    return out


def census(tables, script, nom):
    """every (trace, column, span of the script) -> Census:
         spans           how many there are
         in_band         ... whose fast mean the kernel would not trust
         ties            ... whose fast mean is a half-integer exactly
         differ          ... with rint(fast) != rint(exact)
         differ_off_tie  ... of those, how many where the fast mean is no exact tie: only the band sends these to the pairwise sum
         differ_outside  ... of those, how many the kernel would have trusted: the property is that there are none
         near            ... whose fast mean lies between 1e-9 and 1e-7 from a half-integer (fast path, just outside the band)
         worst           max |fast - exact|
         reach           the largest distance from the half at which the two roundings differ"""
    n_prbs = max(sum(r) for r in script)      # the carrier: 200 PRBs for SCRIPT_A, 256 for SCRIPT_B
    tot = dict(spans=0, in_band=0, ties=0, differ=0, differ_off_tie=0, differ_outside=0, near=0)
    worst = reach = 0.0
    for tab in tables:
        cols = carrier(tab, n_prbs)
        assert np.max(np.abs(cols)) <= SMAX
        ps = prefix_table(cols)
        for lo, n in spans_of(script):
            fast, exact = fast_mean(ps, lo, n, nom), exact_mean(cols, lo, n, nom)
            d = half_distance(fast)
            band = in_band(fast)
            differ = np.rint(fast) != np.rint(exact)
            tot['spans'] += fast.size
            tot['in_band'] += int(band.sum())
            tot['ties'] += int((d == 0.0).sum())
            tot['differ'] += int(differ.sum())
            tot['differ_off_tie'] += int((differ & (d != 0.0)).sum())
            tot['differ_outside'] += int((differ & ~band).sum())
            tot['near'] += int(((d > 1e-9) & (d < 1e-7)).sum())
            worst = max(worst, float(np.max(np.abs(fast - exact))))
            if differ.any():
                reach = max(reach, float(np.max(d[differ])))
    return Census(worst=worst, reach=reach, **tot)


def rotation(script, n_envs, step):
    """[n_envs][slices] int32: the script's rows in rotation over replicas and steps"""
    return np.array([script[(r + step) % len(script)] for r in range(n_envs)], dtype=np.int32)


# ---- the configuration in which a tenth of the UEs carry the clamped nominal ------------------------------------------------------
def churn(cfg):
    """arrivals, departures and bursts within a few steps (tests/test_gpu_edges.py: _churn)"""
    cfg.cbr_lambda, cfg.cbr_t_mean = 2.0 / 1.2, 0.6
    cfg.vbr_lambda, cfg.vbr_t_mean = 5.0 / 1.2, 0.6
    cfg.vbr_b_size, cfg.vbr_b_rate = 40, 12
    return cfg


def floor_config(scenario=0, n_envs=1, **shape):
    """prop_A = prop_B = 0: the path loss is the FSPL floor, and macro_cell clamps it at the MCL for the nearer UEs"""
    cfg = churn(make_config(scenario, n_envs=n_envs, **shape))
    cfg.prop_A = cfg.prop_B = 0.0
    return cfg
