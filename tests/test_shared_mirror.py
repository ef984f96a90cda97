"""tests/shared_mirror.py on the CPU: the restated shared-dictionary step against exact arithmetic (within the derived bounds),
against the ORACLE applied sequentially (one learner per slice, the merged list in order through predict and, when mistaken, update:
what csrc/kb_kbrl.hip says the shared step is), and against other summation orders -- the inputs must tell the orders apart, or
the device test that compares bits with the mirror (tests/test_gpu_shared_chain.py) would pass whatever the kernels did.
Run with -s for the largest error / bound ratios (DESIGN.md section 2 quotes them)."""
import numpy as np
import pytest

import scoring_mirror as sm
import shared_mirror as shm
import update_mirror as um
from oracle import pyoracle as po

GAMMA, ETA, N_PRBS = 1.0, 0.1, 200
MAX_LEFT_OUT = 0.01


def differ(a, b):
    return int((np.ascontiguousarray(a, dtype=np.float64) != np.ascontiguousarray(b, dtype=np.float64)).sum())


@pytest.fixture(scope='module')
def grown():
    d10, _ = shm.oracle_grown(10, N_PRBS, [m for m in shm.GEMM_SIZES] + [c for c, _, _ in shm.FULL_CASES], seed=41)
    d3, _ = shm.oracle_grown(3, N_PRBS, [257, 65], seed=43)
    return {10: d10, 3: d3}


def test_exact_scores_is_the_scoring_mirrors_exact_value(grown):
    Kinv, co, L = grown[10][63]
    x = shm.replica_states(L, 2, 5)[0]
    idx = sm.grid_index(L[:, -1], N_PRBS)
    f1, S1, A1 = shm.exact_scores(L, co, idx, x, N_PRBS, GAMMA)
    f2, S2, A2 = sm.exact_scores(L, co, x, N_PRBS, GAMMA)
    for c in range(N_PRBS + 1):
        assert abs(f1[c] - f2[c]) <= 2.0 ** -200 * float(S2[c]), c
    assert (S1 == S2).all() and (A1 == A2).all()


@pytest.mark.parametrize('dims,m', [(10, m) for m in shm.GEMM_SIZES if m >= 256] + [(3, 257)])
def test_gemm_scores_keep_their_bound_and_tell_the_orders_apart(grown, dims, m):
    """six replicas (one of them far away: all E_j underflow) against a dictionary of m landmarks: every score within bound_units of
    the exact value; the linear tree and the seven-way split each change at least one score; no candidate of the replicas that
    take the product is open (exact |f| above the bound), so the scan on the mirror's scores is the scan on the exact ones"""
    Kinv, co, L = grown[dims][m]
    idx = sm.grid_index(L[:, -1], N_PRBS)
    assert (idx >= 0).all()
    X = shm.replica_states(L, 6, 100 + m, far=3)
    G = sm.gtable(GAMMA, N_PRBS)
    mir = shm.gemm_scores(L, co, idx, X, G, N_PRBS, GAMMA)
    ranges, per = shm.part_ranges(m)
    assert per == -(-((m + 3) // 4) // 8) and ranges[-1][1] >= m
    took = shm.takes_product(mir['emax'])
    assert not took[3] and took[[0, 1, 2, 4, 5]].all()
    worst, left_out, pairs = 0.0, 0, 0
    rng = np.random.default_rng(m)
    for e in np.nonzero(took)[0]:
        f, S, A = shm.exact_scores(L, co, idx, X[e], N_PRBS, GAMMA)
        tol = shm.tolerance(m, dims + 1, GAMMA, S, A, float(np.abs(co).max()))
        err = sm.errors(mir['F'][e], f)
        assert (err <= tol).all(), (m, e, float((err / tol).max()))
        worst = max(worst, float((err / tol).max()))
        is_open = shm.open_candidates(f, tol)
        for y in (1, -1):
            a_i = int(rng.integers(0, N_PRBS + 1))
            ex = shm.scan(f, y, a_i, 0, 0, N_PRBS, m)
            mr = shm.scan(mir['F'][e], y, a_i, 0, 0, N_PRBS, m)
            lo, hi = (a_i, N_PRBS) if y == 1 else (0, a_i)
            last = ex['cstar'] if ex['cstar'] >= 0 else hi
            pairs += 1
            if is_open[lo:last + 1].any() or is_open[a_i]:
                left_out += 1
                continue
            assert ex == mr, (m, e, y, a_i)
    assert left_out == 0, 'the seeds were chosen so that no pair is left out: %d of %d' % (left_out, pairs)
    lin = shm.gemm_scores(L, co, idx, X, G, N_PRBS, GAMMA, linear_tree=True)
    sev = shm.gemm_scores(L, co, idx, X, G, N_PRBS, GAMMA, ks=7)
    n_lin, n_sev = differ(lin['F'][took], mir['F'][took]), differ(sev['F'][took], mir['F'][took])
    print('gemm m %d dims %d: error / bound %.3g; a linear tree changes %d scores, a seven-way split %d' % (m, dims, worst, n_lin, n_sev))
    assert n_lin > 0 and n_sev > 0


@pytest.mark.parametrize('cap,n,kind', shm.FULL_CASES)
def test_full_batch_against_exact_arithmetic_the_oracle_and_other_orders(cap, n, kind):
    """a full dictionary of `cap` landmarks (the oracle's own, grown along the stream, capacity = cap) takes a list of n proposals:
    the mirror's DS and f_p keep their bounds against exact arithmetic of the same doubles; its applied set and mistake count are
    those of the oracle fed the list in order, f within 1e-9 (1 + sum |k c|), the coefficients within 1e-8; A summed in plain k and a
    walk that forms k_p . coeff afresh give other bits wherever the case can tell (a chain of eight terms and more; a list in which
    something was applied before the last proposal)"""
    X, Y = shm.stream(10, N_PRBS, 2 * cap + 64, 41)
    oa = po.OracleKBRL([10], N_PRBS, [0], [1], gamma=GAMMA, eta=ETA, capacity=cap)
    oa.set_seed(0)
    i = 0
    while oa.m(0) < cap:
        if oa.predict(0, X[i])[1] * Y[i] <= 0:
            oa.update(0, X[i], int(Y[i]))
        i += 1
    Kinv, co, L = oa.kinv(0), oa.coeff(0), oa.landmarks(0)
    props = shm.apply_list(L, co, N_PRBS, n, 1000 + cap, kind)
    mir = shm.full_batch(Kinv, co, L, props, GAMMA, N_PRBS, ETA)
    ex = shm.exact_full_batch(Kinv, co, mir['KF'], mir['y'])
    assert not ex['open'].any(), 'the seeds were chosen so that no proposal is open'
    assert (ex['applied'] == mir['applied']).all()
    B = um.bound_units(cap, 'col') + um.exact_units(cap)
    rd = float((np.abs(mir['DS'].astype(np.longdouble) - ex['ds']) / np.maximum(B * um.U * ex['S'], np.longdouble(1e-4000))).max())
    rf = float((np.abs(mir['f'].astype(np.longdouble) - ex['f']) / ex['Ef']).max())
    low = shm.lower_tiles(n)
    ra = float((np.abs(mir['A'].astype(np.longdouble) - ex['A'])[low] / ex['EA'][low]).max())
    assert rd <= 1.0 and rf <= 1.0 and ra <= 1.0, (cap, rd, rf, ra)
    # the oracle, sequentially
    Xp, yp, _, _ = shm.unpack(props, n, 11, N_PRBS)
    applied = np.zeros(n, dtype=bool)
    for p in range(n):
        f = oa.predict(0, Xp[p])[1]
        k = np.exp(-GAMMA * ((L - Xp[p][None]) ** 2).sum(axis=1))
        assert abs(f - mir['f'][p]) <= 1e-9 * (1.0 + np.abs(k * oa.coeff(0)).sum()), (cap, p, f, mir['f'][p])
        if f * yp[p] <= 0:
            applied[p] = True
            assert oa.update(0, Xp[p], int(yp[p]))[0] == 1 and oa.m(0) == cap
    assert (applied == mir['applied']).all() and mir['n_mist'] == int(applied.sum())
    np.testing.assert_allclose(mir['coeff'], oa.coeff(0), rtol=1e-8, atol=1e-9)
    assert applied[0] and (kind != 'stop' or n < 2 or not applied.all())
    # other orders
    alt_a = shm.full_batch(Kinv, co, L, props, GAMMA, N_PRBS, ETA, plain_k=True)
    alt_f = shm.full_batch(Kinv, co, L, props, GAMMA, N_PRBS, ETA, fresh_dot=True)
    n_a, n_f = differ(alt_a['A'][low], mir['A'][low]), differ(alt_f['f'], mir['f'])
    print('full batch cap %d, %d proposals (%d applied): error / bound d* %.3g, A %.3g, f_p %.3g; plain k changes %d entries of A, '
          'a fresh dot %d of the f_p' % (cap, n, int(applied.sum()), rd, ra, rf, n_a, n_f))
    if cap >= 8:
        assert n_a > 0
    if applied[:-1].any():
        assert n_f > 0


@pytest.mark.parametrize('budget', [4, 64])
def test_rounds_of_the_mirror_are_the_sequential_oracle(budget):
    """24 replicas, dims [10, 3], 50 PRBs, 4 rounds a step, 6 steps from empty dictionaries: the mirror's scan (on plain float64
    scores of ITS dictionaries), collect, growing_apply and commit beside ONE oracle learner per slice fed the merged lists in
    order.  Proposals come in replica order, cut at the budget; counts are all proposers; a proposer that was not taken scans again FROM its
    candidate (and proposes it again while it is still a mistake), a taken one resumes past it; sizes, branches and the applied set are exact, f within
    1e-9 (1 + sum |k c|), coefficients and Kinv within 1e-8; no pair is left out."""
    N, dims, n_prbs, rounds, steps = 24, [10, 3], 50, 4, 6
    ref = shm.OracleRounds(dims, n_prbs, N, GAMMA, ETA, 256)
    off = ref.off
    D = [dict(kinv=np.zeros((0, 0)), coeff=np.zeros(0), landmarks=np.zeros((0, d + 1))) for d in dims]
    inputs = shm.round_inputs(N, dims, n_prbs, steps, seed=8)
    seen = dict(retaken=0, resumed=0, silent=0, over_budget=0)
    for states, actions, labels in inputs:
        ref.begin(states, actions, labels)
        cursor = np.zeros((N, 2), dtype=np.int64)
        prev = None
        for rnd in range(rounds):
            want, hits, out = ref.scan()
            cstar = np.full((N, 2), -1, dtype=np.int64)
            for s in range(2):
                for e in range(N):
                    f, _ = shm.plain_scores(D[s]['landmarks'], D[s]['coeff'], states[e, off[s]:off[s] + dims[s]], n_prbs, GAMMA)
                    r = shm.scan(f, int(labels[e, s]), int(actions[e, s]), int(cursor[e, s]), rnd, n_prbs, len(D[s]['coeff']))
                    cstar[e, s], cursor[e, s] = r['cstar'], r['cursor']
                    assert rnd > 0 or r['hit'] == hits[e, s]
            assert not out.any() and (cstar == want).all(), rnd
            counts, lists, props = shm.collect(cstar, budget, states, labels, 0, off, dims)
            if prev is not None:
                for s in range(2):
                    for e in range(N):
                        if prev['cstar'][e, s] >= 0 and not prev['taken'][e, s]:
                            # (its cursor stayed ON the candidate: it proposes it again unless the round's applied
                            # samples put it right, and then the next mistake behind it, if any)
                            assert cstar[e, s] < 0 or cstar[e, s] >= prev['cstar'][e, s]
                            seen['retaken'] += int(cstar[e, s] == prev['cstar'][e, s])
                        elif prev['cstar'][e, s] >= 0:
                            assert cstar[e, s] < 0 or cstar[e, s] > prev['cstar'][e, s]
                            seen['resumed'] += 1
                        else:
                            assert cstar[e, s] < 0
                            seen['silent'] += 1
            if counts.sum() == 0:
                break
            seen['over_budget'] += int((counts > budget).sum())
            res = ref.apply(lists)
            taken = np.zeros((N, 2), dtype=bool)
            for s in range(2):
                assert [e for e, _ in lists[s]] == sorted(e for e, _ in lists[s]) and len(lists[s]) == min(counts[s], budget)
                g = shm.growing_apply(D[s]['kinv'], D[s]['coeff'], D[s]['landmarks'], props[s], GAMMA, n_prbs, dims[s] + 1, ETA, 256,
                                      count=len(lists[s]))
                for p, (fo, ap, br) in enumerate(res[s]):
                    assert ap == g['applied'][p] and br == g['branch'][p], (rnd, s, p)
                    assert abs(fo - g['f'][p]) <= 1e-9 * (1.0 + np.abs(g['coeff']).sum())
                D[s] = g
                o = ref.oa[s]
                assert o.m(0) == g['m']
                np.testing.assert_allclose(g['coeff'], o.coeff(0), rtol=1e-8, atol=1e-9)
                np.testing.assert_allclose(g['kinv'], o.kinv(0), rtol=1e-8, atol=1e-8 * np.abs(o.kinv(0)).max())
                for e, _ in lists[s]:
                    taken[e, s] = True
            n_taken = [len(l) for l in lists]
            prev = dict(cstar=cstar.copy(), taken=taken)
            cursor = shm.commit(cstar, n_taken, cursor)
            ref.commit(n_taken)
            assert (cursor == ref.cursor).all()
    assert ref.open == 0 and ref.open <= MAX_LEFT_OUT * ref.pairs
    assert seen['resumed'] > 0 and seen['silent'] > 0 and (budget >= N or (seen['retaken'] > 0 and seen['over_budget'] > 0)), seen
    assert min(len(d['coeff']) for d in D) >= 3
