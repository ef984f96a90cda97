"""The shared-dictionary step ON THE DEVICE, stage by stage (csrc/kb_kbrl.hip), against tests/shared_mirror.py, exact arithmetic and
the sequential oracle.

  (a) scan    kb_shared_scan on dictionaries around the threshold of the MFMA scoring (255 .. 513 landmarks): the eight partial
              sums of F = E Q and the parts' largest E (kb_dev_get_shared_scores of the test build) equal the mirror's as values
              bit for bit (zeros of either sign equal), their tree reproduces what the scan decided, F keeps its derived bound
              against exact arithmetic, and cstar, labels, proposal bytes, replica ids, counts and hits are those of the scan on
              the EXACT scores; then kb_select_action on the same states (select_scan<3>).
  (b) apply   kb_shared_apply of hand-made lists on full dictionaries: KF, DS, F0, A (kb_dev_get_shared_apply), the mistake count,
              the saturation flag and every coefficient equal the mirror's full_batch as bits, named by stage; DS and f_p keep their
              bounds; a twin built with KBRL_SERIAL_APPLY=1 leaves the same coefficient bits.
  (c) rounds  24 replicas, rounds driven by hand beside ONE oracle learner per slice fed the merged lists in order; then
              kb_shared_step on a fresh twin must leave the same bytes.

The dictionaries are grown by kb_fit on a per-replica handle from prefixes of ONE stream per kind (shared_mirror.stream), an
oracle learner beside them with equal branches, and crossed into shared handles with to_shared.  A (replica, slice) pair whose
exact score is within the bound of zero at or before its first mistake would be left out of the comparison; the seeds are
chosen so that NONE is, and the tests fail when that is broken.  Run with -s for the largest error / bound ratios (DESIGN.md
section 2 quotes them).
"""
import ctypes as C

import numpy as np
import pytest

import scoring_mirror as sm
import shared_mirror as shm
import update_mirror as um

pytestmark = pytest.mark.gpu

GAMMA, ETA = 1.0, 0.1
DIMS = [10, 3]
OFF = [0, 10]
SEEDS = {10: 41, 3: 43}
_ip, _dp, _fp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)


def _bind(L):
    """the accessors of the test build (csrc/kb_probe.hip; not part of ranslice._lib's product surface)"""
    L.kb_dev_get_shared_scores.argtypes = [C.c_void_p, _dp, _dp]
    L.kb_dev_get_shared_scores.restype = C.c_int
    L.kb_dev_get_shared_apply.argtypes = [C.c_void_p, C.c_int, C.c_int32, _dp, _dp, _dp, _dp]
    L.kb_dev_get_shared_apply.restype = C.c_int
    L.kb_dev_get_rows.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32, _ip, _dp, _dp, _ip, _dp, _dp, _dp]
    L.kb_dev_get_rows.restype = C.c_int
    L.kb_dev_get_scores.argtypes = [C.c_void_p, _dp, _dp, _ip]
    L.kb_dev_get_scores.restype = C.c_int


def _p(a, t):
    return a.ctypes.data_as(t)


def values_equal(a, b):
    """bit for bit as values: zeros of either sign are equal (a padding term fma(0, 0, acc) turns -0.0 into +0.0), NaN never is"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a == b).all())


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ growing the dictionaries
_grown = {}


def grown(n_prbs, capacity, sizes, off_grid=None):
    """ONE per-replica VecKBRL (test build) of len(sizes) agents (+ one more of sizes[off_grid] with a landmark off the grid),
    agent i holding sizes[i] = (m of the learner of ten state variables, m of the one of three), grown by kb_fit from prefixes of
    one stream per kind; an oracle learner walks each stream beside it and must take the same branch at every sample"""
    key = (n_prbs, capacity, tuple(sizes), off_grid)
    if key in _grown:
        return _grown[key]
    from ranslice.kbrl_dev import VecKBRL
    n = len(sizes) + (1 if off_grid is not None else 0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        mp.delenv('KBRL_SERIAL_APPLY', raising=False)
        ag = VecKBRL(n, DIMS, n_prbs, capacity=capacity, gamma=GAMMA, eta=ETA)
    _bind(ag.L)
    ag.reset(np.zeros((n, 2), dtype=np.int32), np.full((n, 2), 2, dtype=np.int32))
    learners, X, Y, want = [], [], [], []
    for s in (0, 1):
        top = max(sz[s] for sz in sizes)
        _, Xs, Ys, m_after, _ = shm.oracle_trace(DIMS[s], n_prbs, 3 * top + 64, SEEDS[DIMS[s]], capacity)
        for i, sz in enumerate(sizes):
            cut = shm.prefix_for(m_after, sz[s])
            learners.append((i, s)); X.append(Xs[:cut]); Y.append(Ys[:cut]); want.append(m_after[:cut])
        if off_grid is not None:
            _, Xo, Yo, mo, _ = shm.oracle_trace(DIMS[s], n_prbs, 3 * top + 64, SEEDS[DIMS[s]], capacity, off_grid=100)
            cut = shm.prefix_for(mo, sizes[off_grid][s])
            learners.append((n - 1, s)); X.append(Xo[:cut]); Y.append(Yo[:cut]); want.append(mo[:cut])
    r = ag.fit(learners, X, Y)
    for (e, s), got, w in zip(learners, r['m'], want):
        assert (np.asarray(got) == w).all(), ('kb_fit and the oracle took different branches', e, s, int(np.argmin(np.asarray(got) == w)))
    _grown[key] = ag
    return ag


def shared_of(ag, agent, n_envs, budget=64, serial=False):
    """a shared handle (test build) holding agent's dictionaries; serial: the one-by-one apply (KBRL_SERIAL_APPLY, read at creation)"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        if serial:
            mp.setenv('KBRL_SERIAL_APPLY', '1')
        else:
            mp.delenv('KBRL_SERIAL_APPLY', raising=False)
        sh = ag.to_shared(agent, n_envs, budget=budget)
    _bind(sh.L)
    return sh


def device_rows(sh, s, cap):
    m = C.c_int32()
    idx, coeff, lam, gtab = np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(cap), np.zeros(256)
    rc = sh.L.kb_dev_get_rows(sh.h, 0, s, cap, C.byref(m), None, None, _p(idx, _ip), _p(coeff, _dp), _p(lam, _dp), _p(gtab, _dp))
    assert rc == 0
    return m.value, idx[:m.value], coeff[:m.value], gtab


# ------------------------------------------------------------------ (a) the scan
SCAN_SIZES = [(255, 255), (256, 256), (257, 257), (259, 259), (260, 260), (288, 288), (320, 320), (513, 257)]
SCAN_CASES = [  # (n_prbs, agent = index into the handle's sizes, n_envs)
    (200, 0, 17), (200, 1, 33), (200, 2, 1), (200, 3, 15), (200, 4, 16), (200, 5, 17), (200, 6, 33), (200, 7, 17), (200, 8, 16),
    (15, 0, 17), (16, 0, 16), (17, 0, 15), (127, 0, 17), (128, 0, 16), (255, 0, 17)]
_worst = dict(scan=0.0)


def _states(sh_learners, n_envs, seed):
    far = 3 if n_envs > 3 else None
    X = np.zeros((n_envs, 13), dtype=np.float32)
    for s in (0, 1):
        X[:, OFF[s]:OFF[s] + DIMS[s]] = shm.replica_states(sh_learners[s]['landmarks'], n_envs, seed + s, far=far)
    return X, far


@pytest.mark.parametrize('n_prbs,agent,n_envs', SCAN_CASES)
def test_scan_scores_are_the_mirrors_bits_and_its_decisions_the_exact_ones(n_prbs, agent, n_envs):
    """n_prbs 200: the size ladder 255 (below the threshold: the streaming pass), 256, 257 (nk = 65: per = 9, a short last part),
    259, 260, 288 (nk = 72), 320, 513 (a second group of candidates' landmarks) and, as agent 8, 260 landmarks one of which lies off
    the grid (the product is off for the slice); the other n_prbs at 257 landmarks: 15 / 16 / 17 (one and two candidate tiles),
    127 / 128 (the second chunk of eight tiles), 255.  Replica 3 lies where every E_j < 1e-250: it takes the streaming pass while
    its tile neighbours take the product.  a_i at 0, at n_prbs and in between, both labels."""
    sizes = SCAN_SIZES if n_prbs == 200 else [(257, 257)]
    ag = grown(n_prbs, 576, sizes, off_grid=4 if n_prbs == 200 else None)
    budget = 64
    sh = shared_of(ag, agent, n_envs, budget)
    try:
        Ld = [sh.learner(0, s) for s in (0, 1)]
        X, far = _states(Ld, n_envs, 1000 * n_prbs + 10 * agent)
        rng = np.random.default_rng(n_prbs + agent)
        kinds = [0, n_prbs, n_prbs // 2, n_prbs // 3, 1, n_prbs - 1]
        action = np.array([[kinds[(e + 2 * s) % 6] if e % 7 else int(rng.integers(0, n_prbs + 1)) for s in (0, 1)] for e in range(n_envs)],
                          dtype=np.int32)
        labels = np.array([[1 if (e // 2 + s) % 2 == 0 else -1 for s in (0, 1)] for e in range(n_envs)], dtype=np.int32)
        hits = np.full((n_envs, 2), -9, dtype=np.int32)
        counts, props = np.zeros(2, dtype=np.int32), np.zeros((2, budget, 18))
        sh._check(sh.L.kb_shared_scan(sh.h, _p(X, _fp), _p(action, _ip), _p(labels, _ip), 0, budget, _p(hits, _ip), _p(counts, _ip),
                                      _p(props, _dp)))
        Fp, Ep = np.zeros((2, 8, n_envs, 256)), np.zeros((2, 8, n_envs))
        assert sh.L.kb_dev_get_shared_scores(sh.h, _p(Fp, _dp), _p(Ep, _dp)) == 0
        security = sh.control(False)['security_factors']
        act, adj = sh.select_action(X)
        ctl = sh.control(False)
        Fp2 = np.zeros_like(Fp)
        assert sh.L.kb_dev_get_shared_scores(sh.h, _p(Fp2, _dp), None) == 0
        want_cstar = np.full((n_envs, 2), -1, dtype=np.int64)
        found = np.full((n_envs, 2), -1, dtype=np.int64)
        sel_open = np.zeros(n_envs, dtype=bool)
        left_out = 0
        for s in (0, 1):
            tag = ('n_prbs %d' % n_prbs, 'agent %d' % agent, 'slice %d' % s)
            m, idx, co, G = device_rows(sh, s, 576)
            L = Ld[s]['landmarks']
            assert m == Ld[s]['m'] == (SCAN_SIZES[4 if agent == 8 else agent][s] if n_prbs == 200 else 257) and same(co, Ld[s]['coeff'])
            assert same(G, sm.gtable(GAMMA, n_prbs)), tag + ('G table',)
            assert (idx == sm.grid_index(L[:, -1], n_prbs)).all() and ((idx < 0).sum() == 1) == (agent == 8), tag + ('grid indices',)
            applies = shm.gemm_applies(m, idx)
            assert applies == (m >= 256 and agent != 8), tag
            xs = X[:, OFF[s]:OFF[s] + DIMS[s]]
            took = np.zeros(n_envs, dtype=bool)
            if applies:
                mir = shm.gemm_scores(L, co, idx, xs, G, n_prbs, GAMMA)
                assert values_equal(Ep[s], mir['emax']), tag + ('E: the largest E of a part', int((Ep[s] != mir['emax']).sum()))
                bad = Fp[s][:, :, :n_prbs + 1] != mir['parts']
                assert not bad.any(), tag + ('F partial sums: %d differ, first (part, replica, candidate) %s'
                                             % (int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad))))
                assert values_equal(Fp2[s][:, :, :n_prbs + 1], mir['parts']), tag + ('F partial sums after kb_select_action',)
                took = shm.takes_product(Ep[s])
                assert far is None or (not took[far] and took[np.arange(n_envs) != far].all()), tag + ('who takes the product', took)
                Fdev = um.tree8(Fp[s][:, :, :n_prbs + 1])
            for e in range(n_envs):
                y, a_i = int(labels[e, s]), int(action[e, s])
                f, S, A = shm.exact_scores(L, co, idx, xs[e], n_prbs, GAMMA)
                if took[e]:
                    tol = shm.tolerance(m, DIMS[s] + 1, GAMMA, S, A, float(np.abs(co).max()))
                    err = sm.errors(Fdev[e], f)
                    assert (err <= tol).all(), tag + ('accuracy of F, replica %d' % e, float((err / tol).max()))
                    _worst['scan'] = max(_worst['scan'], float((err / tol).max()))
                else:
                    tol = shm.streaming_tolerance(L, co, idx, xs[e], n_prbs, GAMMA, S, A)
                is_open = shm.open_candidates(f, tol)
                ex = shm.scan(f, y, a_i, 0, 0, n_prbs, m)
                lo, hi = (a_i, n_prbs) if y == 1 else (0, a_i)
                last = ex['cstar'] if ex['cstar'] >= 0 else hi
                if is_open[lo:last + 1].any() or is_open[a_i]:
                    left_out += 1
                    want_cstar[e, s] = -2
                else:
                    want_cstar[e, s] = ex['cstar']
                    assert hits[e, s] == ex['hit'], tag + ('hit of replica %d' % e, hits[e, s], ex['hit'])
                    if took[e]:   # the tree of the device's own partial sums decides what the device decided
                        assert shm.scan(Fdev[e], y, a_i, 0, 0, n_prbs, m) == ex, tag + ('the tree, replica %d' % e,)
                pos = [c for c in range(n_prbs + 1) if f[c] > 0]
                found[e, s] = pos[0] if pos else -1
                sel_open[e] |= bool(is_open[:(pos[0] if pos else n_prbs) + 1].any())
        assert left_out == 0, 'pairs left out of the comparison: %d of %d (the seeds were chosen so that none is)' % (left_out, 2 * n_envs)
        cnt, lists, wprops = shm.collect(want_cstar, budget, X, labels, 0, OFF, DIMS)
        assert (counts == cnt).all(), ('counts', counts, cnt)
        for s in (0, 1):
            assert props[s, :cnt[s]].tobytes() == wprops[s, :cnt[s]].tobytes(), ('proposals of slice %d' % s,)
        assert not sel_open.any()
        for e in range(n_envs):
            a, mg, dj = shm.select(found[e], security[e], n_prbs)
            assert list(act[e]) == a and list(ctl['margins'][e]) == mg and adj[e] == dj, ('select_action, replica %d' % e, act[e], a)
        assert (labels == 1).any() and (labels == -1).any() and (counts > 0).any()
        print('scan n_prbs %d agent %d: %d + %d proposers; F error / bound so far %.3g' % (n_prbs, agent, counts[0], counts[1], _worst['scan']))
    finally:
        sh.close()


# ------------------------------------------------------------------ (b) the batched apply of a full dictionary
APPLY_CASES = shm.FULL_CASES + [(128, 1, 'none'), (256, 65, 'none'), (1024, 17, 'none')]     # (1,024: the bench's capacity)
_worst.update(ds=0.0, A=0.0, f=0.0)


@pytest.mark.parametrize('cap,n,kind', APPLY_CASES)
def test_full_batch_apply_is_the_mirrors_stage_by_stage(cap, n, kind):
    """capacities 2, 63, 65 (d* by the column walk) and 64, 128, 256, 320, 576, 1,024 (on the matrix cores; nine and sixteen blocks); lists of 1, 15, 16,
    17, 64, 65 and 256 proposals, counts[s] above the budget, both labels; 'stop': later proposals stop being mistakes once earlier
    ones are applied, 'none': none does.  Up to 128 landmarks the learner of three state variables is full as well and takes a list
    of its own; above, it holds 64 landmarks and an EMPTY list beside the full one."""
    n_prbs = 200
    both = cap <= 128
    ag = grown(n_prbs, cap, [(cap, cap if both else 64)])
    budget = max(n, 2)
    sh, tw = shared_of(ag, 0, 1, budget), shared_of(ag, 0, 1, budget, serial=True)
    try:
        before = [sh.learner(0, s, with_kinv=True) for s in (0, 1)]
        props, counts = np.zeros((2, budget, 18)), np.zeros(2, dtype=np.int32)
        n_of = [n, min(n, 17) if both else 0]
        for s in (0, 1):
            if n_of[s]:
                props[s, :n_of[s]] = shm.apply_list(before[s]['landmarks'], before[s]['coeff'], n_prbs, n_of[s], 1000 + cap + s, kind)
        counts[:] = [n + 5 if n == budget else n, n_of[1]]       # (a full list says that more proposers stood behind it)
        flagged = bool(sh.flagged_replicas()['saturated'])
        for h in (sh, tw):
            m0 = h.stats()[1]
            h._check(h.L.kb_shared_apply(h.h, _p(counts, _ip), _p(props, _dp), budget))
            h._check(h.L.kb_shared_commit(h.h, _p(np.zeros(2, dtype=np.int32), _ip)))
            h.mistakes = h.stats()[1] - m0
        capr = (cap + 63) & ~63
        total, sat = 0, False
        for s in (0, 1):
            tag = ('capacity %d' % cap, '%d proposals' % n_of[s], 'slice %d' % s)
            b, a, t = before[s], sh.learner(0, s, with_kinv=True), tw.learner(0, s, with_kinv=True)
            assert a['m'] == b['m'] == t['m'] and same(a['kinv'], b['kinv']) and same(a['landmarks'], b['landmarks']), tag
            if not n_of[s]:
                assert same(a['coeff'], b['coeff']) and same(t['coeff'], b['coeff']), tag + ('an empty list changed the coefficients',)
                continue
            assert b['m'] == cap, tag
            KF, DS, A, F0 = np.zeros((budget, capr)), np.zeros((budget, capr)), np.zeros((budget, budget)), np.zeros(budget)
            assert sh.L.kb_dev_get_shared_apply(sh.h, s, budget, _p(KF, _dp), _p(DS, _dp), _p(A, _dp), _p(F0, _dp)) == 0
            k = n_of[s]
            mir = shm.full_batch(b['kinv'], b['coeff'], b['landmarks'], props[s], GAMMA, n_prbs, ETA, count=k)
            low = shm.lower_tiles(k)
            Ad = A[:k, :k].T        # (stored by column)
            for stage, dev, want in (('KF', KF[:k, :cap], mir['KF']), ('DS', DS[:k, :cap], mir['DS']), ('F0', F0[:k], mir['F0']),
                                     ('A', np.where(low, Ad, 0.0), np.where(low, mir['A'], 0.0))):
                ok = values_equal(dev, want) if stage == 'A' else same(dev, want)
                assert ok, tag + ('stage %s: %d of %d values differ' % (stage, int((np.asarray(dev) != np.asarray(want)).sum()), np.asarray(want).size),)
            ex = shm.exact_full_batch(b['kinv'], b['coeff'], KF[:k, :cap], mir['y'])
            assert not ex['open'].any(), tag + ('a proposal is within the bound of zero: the seeds were chosen so that none is',)
            assert (ex['applied'] == mir['applied']).all(), tag + ('applied set against exact arithmetic',)
            B = um.bound_units(cap, 'col') + um.exact_units(cap)
            ld = np.longdouble
            rd = float((np.abs(DS[:k, :cap].astype(ld) - ex['ds']) / np.maximum(B * um.U * ex['S'], ld(1e-4000))).max())
            ra = float((np.abs(Ad.astype(ld) - ex['A'])[low] / ex['EA'][low]).max())
            rf = float((np.abs(mir['f'].astype(ld) - ex['f']) / ex['Ef']).max())
            assert rd <= 1.0 and ra <= 1.0 and rf <= 1.0, tag + ('accuracy: d* %.3g, A %.3g, f_p %.3g of the bound' % (rd, ra, rf),)
            _worst.update(ds=max(_worst['ds'], rd), A=max(_worst['A'], ra), f=max(_worst['f'], rf))
            assert same(a['coeff'], mir['coeff']), tag + ('coefficients: %d differ (applied %d of %d)' % (
                int((a['coeff'] != mir['coeff']).sum()), mir['n_mist'], k),)
            assert same(t['coeff'], a['coeff']), tag + ('the one-by-one apply leaves other coefficient bits',)
            if s == 0:     # the list is what its kind says
                assert mir['applied'][0] and (kind != 'stop' or k < 2 or not mir['applied'].all()) and (kind != 'none' or k > 64 or mir['applied'].all())
            total += mir['n_mist']
            sat = sat or mir['sat']
        assert sh.mistakes == total == tw.mistakes, ('mistake count', sh.mistakes, tw.mistakes, total)
        assert bool(sh.flagged_replicas()['saturated']) == (flagged or sat), ('saturation flag', flagged, sat)
        print('apply capacity %d, %d proposals: error / bound so far d* %.3g, A %.3g, f_p %.3g' % (cap, n, _worst['ds'], _worst['A'], _worst['f']))
    finally:
        sh.close()
        tw.close()


# ------------------------------------------------------------------ (c) rounds with several replicas
@pytest.mark.parametrize('budget', [4, 64])
def test_rounds_by_hand_are_the_sequential_oracle_and_kb_shared_step_leaves_the_same_bytes(budget):
    """24 replicas, dims [10, 3], 50 PRBs, 4 rounds a step, 12 steps from empty dictionaries on the product's library: scan, a host
    merge of one rank, apply, commit, beside shared_mirror.OracleRounds (one oracle learner per slice, the merged lists in order) and
    the mirror's growing_apply on the device's own dictionaries (bits)."""
    from ranslice.kbrl_dev import PROP_W, SharedVecKBRL, merge_proposals
    N, n_prbs, rounds, steps = 24, 50, 4, 12
    assert PROP_W == 18
    ref = shm.OracleRounds(DIMS, n_prbs, N, GAMMA, ETA, 256)
    inputs = shm.round_inputs(N, DIMS, n_prbs, steps, seed=8)
    ia, sf = np.zeros((N, 2), dtype=np.int32), np.full((N, 2), 2, dtype=np.int32)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('RANSLICE_DEV_BUILD', raising=False)
        sh = SharedVecKBRL(N, DIMS, n_prbs, budget=budget, max_rounds=rounds, capacity=256, gamma=GAMMA, eta=ETA)
        tw = SharedVecKBRL(N, DIMS, n_prbs, budget=budget, max_rounds=rounds, capacity=256, gamma=GAMMA, eta=ETA)
    try:
        sh.reset(ia, sf)
        tw.reset(ia, sf)
        seen = dict(retaken=0, resumed=0, silent=0, over_budget=0, rounds=0)
        for step, (states, actions, labels) in enumerate(inputs):
            ref.begin(states, actions, labels)
            prev = None
            hits = np.full((N, 2), -9, dtype=np.int32)
            for rnd in range(rounds):
                tag = ('step %d' % step, 'round %d' % rnd)
                want, whits, out = ref.scan()
                assert not out.any(), tag + ('pairs within 1e-9 of zero: the seeds were chosen so that none is', int(out.sum()))
                counts, props = np.zeros(2, dtype=np.int32), np.zeros((2, budget, PROP_W))
                first = rnd == 0
                n_pred = sh.stats()[0]
                sh._check(sh.L.kb_shared_scan(sh.h, _p(states, _fp) if first else None, _p(actions, _ip) if first else None,
                                              _p(labels, _ip) if first else None, rnd, budget, _p(hits, _ip), _p(counts, _ip), _p(props, _dp)))
                cnt, lists, wprops = shm.collect(want, budget, states, labels, 0, OFF, DIMS)
                assert (counts == cnt).all(), tag + ('counts: all proposers', counts, cnt)
                for s in (0, 1):
                    k = min(int(cnt[s]), budget)
                    assert props[s, :k].tobytes() == wprops[s, :k].tobytes(), tag + ('proposals of slice %d: replica order, cut at the budget' % s,)
                if first:
                    assert (hits == whits).all(), tag + ('hits',)
                # every replica scanned from where the commit left its cursor: the device's own count of predictions says so even
                # where the candidate it was taken for has stopped being a mistake
                assert sh.stats()[0] - n_pred == ref.n_pred, tag + ('predictions of the scan: the cursors', sh.stats()[0] - n_pred, ref.n_pred)
                if prev is not None:
                    for s in (0, 1):
                        for e in range(N):
                            if prev['cstar'][e, s] >= 0 and not prev['taken'][e, s]:
                                seen['retaken'] += int(want[e, s] == prev['cstar'][e, s])
                            elif prev['cstar'][e, s] >= 0:
                                assert want[e, s] < 0 or want[e, s] > prev['cstar'][e, s]
                                seen['resumed'] += 1
                            else:
                                assert want[e, s] < 0
                                seen['silent'] += 1
                if counts.sum() == 0:
                    break
                seen['rounds'] += 1
                seen['over_budget'] += int((counts > budget).sum())
                mc, mp_, taken = merge_proposals(counts[None], props[None], budget)
                mc, mp_ = np.ascontiguousarray(mc, dtype=np.int32), np.ascontiguousarray(mp_)
                before = [sh.learner(0, s, with_kinv=True) for s in (0, 1)]
                sh._check(sh.L.kb_shared_apply(sh.h, _p(mc, _ip), _p(mp_, _dp), budget))
                acc = np.ascontiguousarray(taken[0], dtype=np.int32)
                sh._check(sh.L.kb_shared_commit(sh.h, _p(acc, _ip)))
                res = ref.apply(lists)
                tk = np.zeros((N, 2), dtype=bool)
                for s in (0, 1):
                    assert acc[s] == len(lists[s])
                    a, o, b = sh.learner(0, s, with_kinv=True), ref.oa[s], before[s]
                    assert a['m'] == o.m(0), tag + ('size of slice %d' % s, a['m'], o.m(0))
                    assert same(a['landmarks'], o.landmarks(0)), tag + ('landmarks',)
                    np.testing.assert_allclose(a['coeff'], o.coeff(0), rtol=1e-8, atol=1e-9)
                    np.testing.assert_allclose(a['kinv'], o.kinv(0), rtol=1e-8, atol=1e-8 * np.abs(o.kinv(0)).max())
                    g = shm.growing_apply(b['kinv'] if b['m'] else np.zeros((0, 0)), b['coeff'], b['landmarks'], mp_[s], GAMMA, n_prbs,
                                          DIMS[s] + 1, ETA, 256, count=int(mc[s]))
                    assert [int(v) for v in g['branch']] == [br for _, _, br in res[s]], tag + ('branches of slice %d' % s,)
                    assert g['m'] == a['m'] and same(g['coeff'], a['coeff']) and same(g['kinv'], a['kinv']), tag + (
                        'the mirror of the one-by-one apply, slice %d: coefficients %d, Kinv %d differ' % (
                            s, int((g['coeff'] != a['coeff']).sum()), int((g['kinv'] != a['kinv']).sum())),)
                    for e, _ in lists[s]:
                        tk[e, s] = True
                prev = dict(cstar=want.copy(), taken=tk)
                ref.commit([len(l) for l in lists])
            assert (tw.update_control(states, actions, labels) == hits).all(), ('kb_shared_step: hits', step)
        assert ref.open == 0
        assert seen['resumed'] > 0 and seen['silent'] > 0 and (budget >= N or (seen['retaken'] > 0 and seen['over_budget'] > 0)), seen
        for s in (0, 1):
            a, t = sh.learner(0, s, with_kinv=True), tw.learner(0, s, with_kinv=True)
            assert a['m'] == t['m'] >= 3, (s, a['m'], t['m'])
            for k in ('landmarks', 'coeff', 'kinv'):
                assert same(a[k], t[k]), ('kb_shared_step leaves other bytes than the rounds by hand', s, k)
        print('rounds budget %d: %s; sizes %s' % (budget, seen, [sh.learner(0, s)['m'] for s in (0, 1)]))
    finally:
        sh.close()
        tw.close()
