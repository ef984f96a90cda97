"""The KBRL scoring chain ON THE DEVICE, stage by stage: what kb_select_action leaves in K.Wg / K.F / K.fdirect and in the
dictionaries' D0 / E / index rows (kb_dev_get_scores / kb_dev_get_rows of the test build, csrc/kb_probe.hip) against
tests/scoring_mirror.py and exact arithmetic.  Dictionaries are grown teacher-forced through kb_predict / kb_update with an
oracle agent in lock-step (equal branch codes at every sample).  Every case asserts

  (a) bits       W and F equal ordered_scores fed with the device's own E / D0 / index rows and G table, value for value (the
                 mirror's Fraction chain cannot produce -0.0, so a zero compares equal to a zero of either sign; everything
                 else is bit equality); fdirect equals the mirror's flags and count; E equals rs_exp_nonpos(-gamma D0) as the
                 oracle computes it; D0 is within the (d - 2) roundings of its sum of the mirror's;
  (b) accuracy   |F - exact| <= bound_units u S(c) + m 2^-1074 with exact_scores in mpmath, for every learner and candidate;
  (c) decisions  actions and `adjusted` equal the oracle's select_action under the same tie-break seeds.

Each test prints its largest device error / bound and oracle error / bound (-s); DESIGN.md §2 quotes them.
"""
import ctypes as C

import numpy as np
import pytest

import primitives_util as pu
import scoring_mirror as sm
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

GAMMA = 1.0


def _bind(L):
    """the two accessors of the test build (not part of ranslice._lib's product surface)"""
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    L.kb_dev_get_scores.argtypes = [vp, dp, dp, ip]
    L.kb_dev_get_scores.restype = C.c_int
    L.kb_dev_get_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int32, ip, dp, dp, ip, dp, dp, dp]
    L.kb_dev_get_rows.restype = C.c_int


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def values_equal(a, b):
    """bit equality, a zero matching a zero of either sign"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return pu.same_bits(a, b) | ((a == 0.0) & (b == 0.0))


class Pair:
    """a device agent (test build) and one oracle agent per replica, kept in lock-step"""

    def __init__(self, n_envs, dims, n_prbs, capacity=256, seed0=11):
        from ranslice.kbrl_dev import VecKBRL
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv('RANSLICE_DEV_BUILD', '1')
            self.ag = VecKBRL(n_envs, dims, n_prbs, capacity=capacity, gamma=GAMMA)
        _bind(self.ag.L)
        self.N, self.dims, self.S, self.n, self.cap = n_envs, list(dims), len(dims), n_prbs, capacity
        self.T = n_envs * self.S
        self.off = np.concatenate([[0], np.cumsum(dims)]).astype(int)
        zero = np.zeros((n_envs, self.S), dtype=np.int32)
        self.ag.reset(zero, zero, seeds=np.arange(n_envs, dtype=np.uint64) + seed0)
        self.oa = []
        for e in range(n_envs):
            a = po.OracleKBRL(dims, n_prbs, zero[e], zero[e], gamma=GAMMA, capacity=capacity)
            a.set_seed(seed0 + e)
            self.oa.append(a)

    def close(self):
        self.ag.close()

    def grow(self, e, s, m, seed, off_grid=()):
        rng = np.random.default_rng(seed)
        X = sm.random_samples(rng, 3 * m + 60, self.dims[s], self.n)
        oa, ag = self.oa[e], self.ag

        def predict(x):
            ag.predict(e, s, x)
            oa.predict(s, x)

        def update(x, y):
            br, obr = ag.update(e, s, x, y)[0], oa.update(s, x, y)[0]
            assert br == obr, (e, s, oa.m(s), br, obr)
            return br
        sm.grow(m, X, predict, update, lambda: oa.m(s), set(off_grid), rng)
        assert self.ag.dictionary_sizes()[e, s] == m

    def state_of(self, states, e, s):
        return states[e, self.off[s]:self.off[s + 1]]

    def select(self, states):
        """select_action on both sides: actions and adjusted must agree -> (actions, adjusted)"""
        act, adj = self.ag.select_action(states)
        for e in range(self.N):
            oact, oadj = self.oa[e].select_action(states[e])
            self.oa[e].adjusted = oadj
            assert (act[e] == oact).all() and adj[e] == oadj, (e, act[e], oact, adj[e], oadj)
        assert (act >= 0).all() and (act <= self.n).all()
        return act, adj

    def scores(self):
        F, W = np.zeros((self.T, 256)), np.zeros((self.T, 256))
        fd = np.zeros(self.T, dtype=np.int32)
        rc = self.ag.L.kb_dev_get_scores(self.ag.h, _p(F, C.c_double), _p(W, C.c_double), _p(fd, C.c_int32))
        assert rc == 0, rc
        return F, W, fd

    def rows(self, e, s):
        cap = self.cap
        D0, E, co, lam, G = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(256)
        idx = np.zeros(cap, dtype=np.int32)
        m = C.c_int32(-1)
        rc = self.ag.L.kb_dev_get_rows(self.ag.h, e, s, cap, C.byref(m), _p(D0, C.c_double), _p(E, C.c_double), _p(idx, C.c_int32),
                                       _p(co, C.c_double), _p(lam, C.c_double), _p(G, C.c_double))
        assert rc == 0, rc
        m = m.value
        return dict(m=m, D0=D0[:m], E=E[:m], idx=idx[:m], coeff=co[:m], lam=lam[:m], G=G)

    def check(self, states, scores, learners=None, accuracy=True):
        """(a) and (b) for the given learners [(e, s)] (default: all) -> (worst device error / bound, worst oracle error / bound,
        {(e, s): the mirror's output})"""
        F, W, fd = scores
        n, worst, outs = self.n, [0.0, 0.0], {}
        assert pu.same_bits(self.rows(0, 0)['G'], sm.gtable(GAMMA, n)).all(), 'the G table'
        for e, s in learners if learners is not None else [(e, s) for e in range(self.N) for s in range(self.S)]:
            t, d = e * self.S + s, self.dims[s] + 1
            x = self.state_of(states, e, s)
            r = self.rows(e, s)
            m = r['m']
            assert m == self.oa[e].m(s)
            Lm = self.ag.learner(e, s)
            if m:
                D0m, _, idxm, lamm = sm.rows(Lm['landmarks'], x, n, GAMMA)
                assert pu.same_bits(r['coeff'], Lm['coeff']).all() and pu.same_bits(r['lam'], lamm).all(), (e, s)
                assert (np.abs(r['D0'] - D0m) <= 2 * max(d - 2, 0) * sm.U * D0m).all(), (e, s, 'D0')
                assert pu.same_bits(r['E'], po.detmath('EXP_NONPOS', -GAMMA * r['D0'])).all(), (e, s, 'E')
                if m >= 2:
                    assert (r['idx'] == idxm).all(), (e, s, 'grid indices')
                k = min(m, 32)
                assert pu.ulp_errors(r['E'][:k], -GAMMA * r['D0'][:k], 'exp').max() <= 1.0
            out = sm.ordered_scores(r['E'], r['idx'], r['coeff'], r['lam'], r['D0'], r['G'], n, GAMMA)
            outs[(e, s)] = out
            assert fd[t] == out['fdirect'], (e, s, m, hex(fd[t]), hex(out['fdirect']))
            if m >= 2:
                ok = values_equal(W[t], out['W'])
                assert ok.all(), ('W', e, s, m, np.nonzero(~ok)[0][:8], W[t][~ok][:4], out['W'][~ok][:4])
            ok = values_equal(F[t, :n + 1], out['F'])
            assert ok.all(), ('F', e, s, m, np.nonzero(~ok)[0][:8], F[t, :n + 1][~ok][:4], out['F'][~ok][:4])
            if not accuracy:
                continue
            fx, S, A = sm.exact_scores(Lm['landmarks'], Lm['coeff'], x, n, GAMMA)
            tol = sm.tolerance_single(S) if m == 1 else sm.tolerance(out['p_max'], n, d, GAMMA, S, A, m, out['fdirect'] >> 8)
            err = sm.errors(F[t, :n + 1], fx)
            assert (err <= tol).all(), ('accuracy', e, s, m, int(np.argmax(err - tol)))
            of = np.array([self.oa[e].predict(s, np.append(x.astype(np.float64), c / n))[1] for c in range(n + 1)])
            tol1 = np.where(tol > 0, tol, 1)
            worst = [max(worst[0], float((err / tol1).max())), max(worst[1], float((sm.errors(of, fx) / tol1).max()))]
            if m >= 2:   # (printed only: against the constant that leaves out the exponentials' argument error)
                nar = np.longdouble(sm.issue_units(out['p_max'], n) * sm.U) * S + m * np.longdouble(sm.TINY)
                self.narrow = max(getattr(self, 'narrow', 0.0), float((err / np.where(nar > 0, nar, 1)).max()))
        return worst[0], worst[1], outs


def random_states(pair, rng):
    st = np.zeros((pair.N, pair.off[-1]), dtype=np.float32)
    for s, dm in enumerate(pair.dims):
        st[:, pair.off[s]:pair.off[s + 1]] = rng.uniform(0.0, sm.SPREAD[dm], (pair.N, dm))
    return st


def report(what, r_dev, r_or, pair=None):
    print('%s: device error / bound %.3g, oracle error / bound %.3g' % (what, r_dev, r_or)
          + (', device error / (p_max + KA + 5) u S %.3g' % pair.narrow if hasattr(pair, 'narrow') else ''))


# ------------------------------------------------------------------ the size ladder
LADDER = [0, 1, 2, 63, 64, 65, 127, 128, 191, 192, 255, 256, 257, 319, 320, 321, 513, 70]


def test_size_ladder_one_wave_and_four_waves_give_the_mirrors_bits():
    """eighteen learners (9 replicas x dims 10 and 3) at every size of the ladder in ONE handle, two workgroups of
    select_gemm_kernel.  The first select_action bins the 320+ learners on one wave and writes their list, the second walks them
    with four waves: F, W and fdirect must be identical, and equal the mirror's"""
    n = 70   # two groups of 64 candidates, five tiles of 16, KA = 72
    P = Pair(9, [10, 3], n, capacity=640)
    try:
        for i, m in enumerate(LADDER):
            P.grow(i // 2, i % 2, m, 500 + i)
        st = random_states(P, np.random.default_rng(1))
        # (a single landmark is scored in float32: a state near it, or k is below the float32 range)
        st[0, 10:13] = (P.oa[0].landmarks(1)[0, :3] + 0.25).astype(np.float32)
        a1 = P.select(st)
        s1 = P.scores()
        a2 = P.select(st)
        s2 = P.scores()
        assert (a1[0] == a2[0]).all() and (a1[1] == a2[1]).all()
        # (F beyond candidate n_prbs is whatever the workgroup's LDS held: never stored by a tile, never read by anybody)
        for u, v, what in zip((s1[0][:, :n + 1],) + s1[1:], (s2[0][:, :n + 1],) + s2[1:], 'FWd'):
            assert u.tobytes() == v.tobytes(), 'one wave and four waves differ in ' + what
        r_dev, r_or, _ = P.check(st, s2)
        report('size ladder', r_dev, r_or, P)
        assert (s2[0][0] == 0.0).all(), 'an empty dictionary scores zero everywhere'
    finally:
        P.close()


# ------------------------------------------------------------------ the candidate grid's edges
@pytest.mark.parametrize('n_prbs', [1, 3, 15, 16, 17, 63, 64, 65, 200, 255])
def test_candidate_grid_edges(n_prbs):
    """tile (n / 16 + 1) and group (64 g <= n) edges of select_gemm_kernel, every candidate 0 .. n_prbs"""
    P = Pair(1, [10, 3], n_prbs, capacity=128)
    try:
        P.grow(0, 0, 70, 600 + n_prbs)
        P.grow(0, 1, 67, 900 + n_prbs)
        rng = np.random.default_rng(n_prbs)
        worst = [0.0, 0.0]
        for _ in range(2 if n_prbs < 100 else 1):
            st = random_states(P, rng)
            P.select(st)
            r_dev, r_or, _ = P.check(st, P.scores())
            worst = [max(worst[0], r_dev), max(worst[1], r_or)]
        report('n_prbs = %d' % n_prbs, worst[0], worst[1], P)
    finally:
        P.close()


# ------------------------------------------------------------------ workgroups of sixteen learners
@pytest.mark.parametrize('n_envs,dims', [(1, [10]), (5, [10, 3, 10]), (8, [3, 10]), (17, [10]), (11, [3, 10, 3])])
def test_workgroup_packing(n_envs, dims):
    """T = 1, 15, 16, 17, 33 learners: full and partial workgroups of select_gemm_kernel, with empty dictionaries and
    single-landmark ones (zero columns of W^T) between the others"""
    n = 50
    sizes = [0, 1, 5, 20, 2, 0, 33]
    P = Pair(n_envs, dims, n, capacity=64)
    try:
        for t in range(P.T):
            P.grow(t // P.S, t % P.S, sizes[t % len(sizes)], 700 + t)
        st = random_states(P, np.random.default_rng(P.T))
        P.select(st)
        sc = P.scores()
        r_dev, r_or, _ = P.check(st, sc, accuracy=False)
        some = sorted({0, P.T - 1, min(15, P.T - 1), min(16, P.T - 1), min(4, P.T - 1)})
        r_dev, r_or, _ = P.check(st, sc, learners=[(t // P.S, t % P.S) for t in some])
        report('T = %d' % P.T, r_dev, r_or, P)
    finally:
        P.close()


# ------------------------------------------------------------------ direct terms
def test_off_grid_counts_across_the_list_of_48():
    """0, 1, 47, 48, 49 and 130 landmarks off the candidate grid (the list holds 48; 130 span three chunks): every candidate takes
    the direct terms in increasing j"""
    n, m, counts = 50, 150, [0, 1, 47, 48, 49, 130]
    P = Pair(len(counts), [10], n, capacity=192)
    try:
        for e, k in enumerate(counts):
            P.grow(e, 0, m, 2000 + k, off_grid=range(3, 3 + k))
        st = random_states(P, np.random.default_rng(3))
        P.select(st)
        sc = P.scores()
        r_dev, r_or, outs = P.check(st, sc)
        for e, k in enumerate(counts):
            assert sc[2][e] == ((3 | (k << 8)) if k else 0), (k, hex(sc[2][e]))
            assert outs[(e, 0)]['open'].all() == bool(k)
        report('off the grid', r_dev, r_or, P)
    finally:
        P.close()


def test_band_state_and_the_settled_rule():
    """a state that leaves a few E_j in (5e-324, 1e-300) and the rest at zero: binned sums of zero, every candidate takes the
    exact exponentials; and three crafted landmarks whose binned sum crosses 1e-240 along the candidates: those at or above it
    keep the binned sum, the others take the direct terms"""
    n = 255
    P = Pair(2, [10, 3], n, capacity=320)
    try:
        P.grow(0, 0, 257, 3010)
        P.grow(0, 1, 257, 3003)
        P.grow(1, 0, 40, 3011)
        near = np.array([0.5 + 23.493, 0.5, 0.5, 0.0])
        for x in [near, np.array([26.8, 0.5, 0.5, 1.0]), np.array([0.5, 26.9, 0.5, 100.0 / 255.0])]:
            y, _ = P.oa[1].predict(1, x)
            P.ag.predict(1, 1, x)
            y = -y if y else 1
            assert P.ag.update(1, 1, x, y)[0] == P.oa[1].update(1, x, y)[0] == 2
        st = np.zeros((2, 13), dtype=np.float32)
        st[0, :10] = sm.band_coordinate(P.oa[0].landmarks(0)[:, :10])
        st[0, 10:] = sm.band_coordinate(P.oa[0].landmarks(1)[:, :3])
        st[1, :10] = 1.0
        st[1, 10:] = 0.5
        P.select(st)
        sc = P.scores()
        r_dev, r_or, outs = P.check(st, sc)
        for s in (0, 1):
            o, r = outs[(0, s)], P.rows(0, s)
            band = (r['E'] > 0) & (r['E'] < sm.KB_E_TINY)
            assert band.any() and not (r['E'] >= sm.KB_E_TINY).any()
            assert sc[2][s] == (1 | (int(band.sum()) << 8)) and o['open'].all() and not sc[1][s].any()
            assert sc[0][s, :n + 1].any(), 'the band terms are not zero'
        o = outs[(1, 1)]
        settled = np.abs(o['binned']) >= sm.KB_F_SETTLED
        assert sc[2][3] == (1 | (2 << 8)) and settled.any() and (~settled).any()
        assert values_equal(sc[0][3, :n + 1][settled], o['binned'][settled]).all()
        assert (o['open'] == ~settled).all()   # (their direct terms, 1e-300 and below, are far under an ulp of 1e-241: same bits)
        report('band and settled', r_dev, r_or, P)
    finally:
        P.close()


# ------------------------------------------------------------------ exact ties and the scores' reuse
def test_all_underflow_state_ties_draw_as_the_oracle():
    """a state so far away that every E_j is zero: every candidate of every learner is an exact tie, decided by the learner's
    Philox stream.  Actions and adjusted equal the oracle's, the predictions' count too, and an update_control + select_action
    that follow still agree: the streams stand at the same position"""
    n = 50
    P = Pair(2, [10, 3], n, capacity=384)
    try:
        for t, m in enumerate([2, 70, 321, 5]):
            P.grow(t // 2, t % 2, m, 4000 + t)
        st = np.full((2, 13), 60.0, dtype=np.float32)
        dev0, orc0 = np.array(P.ag.stats()[:2], dtype=np.int64), np.sum([a.stats() for a in P.oa], axis=0)
        for _ in range(2):
            act, adj = P.select(st)
            F, W, fd = P.scores()
            assert not F.any() and not W.any() and not fd.any()
        dev, orc = np.array(P.ag.stats()[:2], dtype=np.int64) - dev0, np.sum([a.stats() for a in P.oa], axis=0) - orc0
        assert dev[0] == orc[0] > 0, (dev, orc, act)
        labels = np.array([[1, -1], [-1, 1]], dtype=np.int32)
        hits = P.ag.update_control(st, act, labels)
        for e in range(2):
            assert (hits[e] == P.oa[e].update_control(st[e], act[e], labels[e])).all(), e
        assert (P.ag.dictionary_sizes() == [[P.oa[e].m(s) for s in range(2)] for e in range(2)]).all()
        P.select(st)
        P.select(random_states(P, np.random.default_rng(9)))
        dev, orc = np.array(P.ag.stats()[:2], dtype=np.int64) - dev0, np.sum([a.stats() for a in P.oa], axis=0) - orc0
        assert dev[0] == orc[0] and dev[1] == orc[1], (dev, orc)
    finally:
        P.close()


def test_update_control_reuses_the_selects_scores():
    """update_control of the state select_action scored, with labels that make no mistake: F stays bit for bit, hits equal the
    oracle's, no dictionary changes"""
    n = 50
    P = Pair(1, [10, 3], n, capacity=192)
    try:
        P.grow(0, 0, 130, 5000)
        P.grow(0, 1, 70, 5001)
        rng = np.random.default_rng(5)
        for _ in range(16):   # a state whose scores allow a label without a mistake for both learners
            st = random_states(P, rng)
            P.select(st)
            F = P.scores()[0][:, :n + 1]
            if all(F[t, n] > 0 or F[t, 0] < 0 for t in range(2)):
                break
        else:
            raise AssertionError('no state with a mistake-free label')
        act, lab = np.zeros((1, 2), dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
        for t in range(2):
            if F[t, n] > 0:    # label +1: the range [a, n] must score positive
                a = n
                while a > 0 and F[t, a - 1] > 0:
                    a -= 1
                act[0, t], lab[0, t] = a, 1
            else:              # label -1: the range [0, a] must score negative
                a = 0
                while a < n and F[t, a + 1] < 0:
                    a += 1
                act[0, t], lab[0, t] = a, -1
        before = P.scores()
        hits = P.ag.update_control(st, act, lab)
        assert (hits[0] == P.oa[0].update_control(st[0], act[0], lab[0])).all()
        after = P.scores()
        assert before[0][:, :n + 1].tobytes() == after[0][:, :n + 1].tobytes(), 'F changed'
        assert P.ag.dictionary_sizes()[0].tolist() == [130, 70] == [P.oa[0].m(0), P.oa[0].m(1)]
        P.select(st)
        assert P.scores()[0][:, :n + 1].tobytes() == before[0][:, :n + 1].tobytes()
    finally:
        P.close()
