"""The shared-dictionary rounds under the margin rule ON THE DEVICE (kb_set_shared_plus; csrc/kb_kbrl.hip:
shared_scan_plus_kernel, shared_apply_plus_kernel) against tests/shared_plus_mirror.py and the sequential learner.

  (a) scan     kb_shared_scan with the switch on against scan_plus on the exact scores (shared_mirror.exact_scores): 257 landmarks
               (the product's scores) and 255 (the streaming pass); with the switch off the same inputs give shared_mirror.scan's
               answer, and the two differ.
  (b) apply    kb_shared_apply of update_mirror's picked lists on full dictionaries: every coefficient, the count of changed
               samples, the saturation flag and kb_get_repair_work's work[6] equal full_batch_plus as bits, KF / DS / F0 / A by
               stage; a twin under KBRL_SERIAL_APPLY=1 counts the same and ends within 1e-8.
  (c) rounds   24 replicas from empty, rounds by hand beside PlusRounds; kb_shared_step on a twin; two shards through the host merge.
  (d) one replica equals a per-replica VecKBRL in Projectron++ mode taught the same rows by fit_steps.
  (e) the switch leaves Projectron alone; (f) refusals; (g) together with kb_shared_prune.
"""
import ctypes as C
import os

import numpy as np
import pytest

import shared_mirror as shm
import shared_plus_mirror as spm
import test_gpu_shared_chain as chain

pytestmark = pytest.mark.gpu

GAMMA, ETA = chain.GAMMA, chain.ETA
DIMS, OFF = chain.DIMS, chain.OFF
_ip, _dp, _fp = chain._ip, chain._dp, chain._fp
_p, same, values_equal = chain._p, chain.same, chain.values_equal


def _work6(h):
    return int(h._repair_raw()[6])


# ------------------------------------------------------------------ (a) the scan
@pytest.mark.parametrize('n_prbs,size,n_envs', [(200, 257, 17), (200, 255, 16), (15, 257, 1), (16, 257, 17)])
def test_scan_proposes_the_first_candidate_inside_the_margin(n_prbs, size, n_envs):
    sizes = chain.SCAN_SIZES if n_prbs == 200 else [(257, 257)]
    ag = chain.grown(n_prbs, 576, sizes, off_grid=4 if n_prbs == 200 else None)
    agent = [s[0] for s in sizes].index(size)
    budget = 64
    got, exact = {}, {}
    for plus in (True, False):
        sh = chain.shared_of(ag, agent, n_envs, budget)
        try:
            sh.set_shared_plus(plus)
            assert sh.shared_plus is plus
            Ld = [sh.learner(0, s) for s in (0, 1)]
            X, _ = chain._states(Ld, n_envs, 1000 * n_prbs + 10 * agent)
            kinds = [0, n_prbs, n_prbs // 2, n_prbs // 3, 1, n_prbs - 1]
            action = np.array([[kinds[(e + 2 * s) % 6] for s in (0, 1)] for e in range(n_envs)], dtype=np.int32)
            labels = np.array([[1 if (e // 2 + s) % 2 == 0 else -1 for s in (0, 1)] for e in range(n_envs)], dtype=np.int32)
            hits = np.full((n_envs, 2), -9, dtype=np.int32)
            counts, props = np.zeros(2, dtype=np.int32), np.zeros((2, budget, 18))
            n_pred = sh.stats()[0]
            sh._check(sh.L.kb_shared_scan(sh.h, _p(X, _fp), _p(action, _ip), _p(labels, _ip), 0, budget, _p(hits, _ip), _p(counts, _ip),
                                          _p(props, _dp)))
            n_pred = sh.stats()[0] - n_pred
            want = np.full((n_envs, 2), -1, dtype=np.int64)
            want_pred, inside_first, left_out = 0, 0, 0
            for s in (0, 1):
                m, idx, co, _ = chain.device_rows(sh, s, 576)
                L = Ld[s]['landmarks']
                for e in range(n_envs):
                    y, a_i = int(labels[e, s]), int(action[e, s])
                    xs = X[e, OFF[s]:OFF[s] + DIMS[s]]
                    if (e, s) not in exact:      # (both handles hold the same dictionaries and see the same states)
                        f, S, A = shm.exact_scores(L, co, idx, xs, n_prbs, GAMMA)
                        tol = shm.streaming_tolerance(L, co, idx, xs, n_prbs, GAMMA, S, A)
                        if shm.gemm_applies(m, idx):     # (the larger of the two paths' bounds: a far replica streams)
                            tol = np.maximum(tol, shm.tolerance(m, DIMS[s] + 1, GAMMA, S, A, float(np.abs(co).max())))
                        exact[e, s] = (f, tol)
                    f, tol = exact[e, s]
                    ex = (spm.scan_plus if plus else shm.scan)(f, y, a_i, 0, 0, n_prbs, m)
                    lo, hi = (a_i, n_prbs) if y == 1 else (0, a_i)
                    last = ex['cstar'] if ex['cstar'] >= 0 else hi
                    near = [abs(f[c]) <= shm.sm_float(tol[c]) or (plus and abs(f[c] * y - 1) <= shm.sm_float(tol[c])) for c in range(lo, last + 1)]
                    if any(near) or abs(f[a_i]) <= shm.sm_float(tol[a_i]):
                        left_out += 1
                        want[e, s] = -2
                        continue
                    want[e, s] = ex['cstar']
                    want_pred += 1 + last - lo + 1
                    assert hits[e, s] == ex['hit'], (plus, e, s)
                    if plus and ex['cstar'] >= 0 and f[ex['cstar']] * y > 0:
                        inside_first += 1      # a candidate with 0 < y f < 1 before any mistake
            assert left_out == 0, 'pairs left out: the seeds were chosen so that none is'
            cnt, lists, wprops = shm.collect(want, budget, X, labels, 0, OFF, DIMS)
            assert (counts == cnt).all(), ('counts', plus, counts, cnt)
            for s in (0, 1):
                k = min(int(cnt[s]), budget)
                assert props[s, :k].tobytes() == wprops[s, :k].tobytes(), ('proposals', plus, s)
            assert n_pred == want_pred, ('predictions counted by the scan', plus, n_pred, want_pred)
            got[plus] = (want.copy(), inside_first)
        finally:
            sh.close()
    assert got[True][1] > 0 and (got[True][0] != got[False][0]).any(), 'the inputs do not tell the two rules apart'


# ------------------------------------------------------------------ (b) the batched apply of a full dictionary
@pytest.mark.parametrize('cap,dims,n', [c for c in spm.PLUS_CASES if c[1] == 10])
def test_full_batch_apply_is_the_mirrors(cap, dims, n):
    n_prbs = 200
    both = cap <= 128
    ag = chain.grown(n_prbs, cap, [(cap, cap if both else 64)])
    budget = max(n, 2)
    sh, tw = chain.shared_of(ag, 0, 1, budget), chain.shared_of(ag, 0, 1, budget, serial=True)
    try:
        before = [sh.learner(0, s, with_kinv=True) for s in (0, 1)]
        props, counts = np.zeros((2, budget, 18)), np.zeros(2, dtype=np.int32)
        n_of = [n, min(n, 17) if both else 0]
        for s in (0, 1):
            if n_of[s]:
                b = before[s]
                props[s, :n_of[s]] = spm.plus_list(b['kinv'], b['coeff'], b['landmarks'], n_prbs, n_of[s], GAMMA, ETA, seed=cap + s)[0]
        counts[:] = [n + 5 if n == budget else n, n_of[1]]
        flagged = bool(sh.flagged_replicas()['saturated'])
        for h in (sh, tw):
            h.set_shared_plus(True)
            m0, w0 = h.stats()[1], _work6(h)
            h._check(h.L.kb_shared_apply(h.h, _p(counts, _ip), _p(props, _dp), budget))
            h._check(h.L.kb_shared_commit(h.h, _p(np.zeros(2, dtype=np.int32), _ip)))
            h.changed, h.work = h.stats()[1] - m0, _work6(h) - w0
        capr = (cap + 63) & ~63
        changed = work = 0
        sat = False
        for s in (0, 1):
            tag = ('capacity %d' % cap, '%d proposals' % n_of[s], 'slice %d' % s)
            b, a, t = before[s], sh.learner(0, s, with_kinv=True), tw.learner(0, s, with_kinv=True)
            assert a['m'] == b['m'] == t['m'] and same(a['kinv'], b['kinv']) and same(a['landmarks'], b['landmarks']), tag
            if not n_of[s]:
                assert same(a['coeff'], b['coeff']) and same(t['coeff'], b['coeff']), tag
                continue
            k = n_of[s]
            KF, DS, A, F0 = np.zeros((budget, capr)), np.zeros((budget, capr)), np.zeros((budget, budget)), np.zeros(budget)
            assert sh.L.kb_dev_get_shared_apply(sh.h, s, budget, _p(KF, _dp), _p(DS, _dp), _p(A, _dp), _p(F0, _dp)) == 0
            mir = spm.full_batch_plus(b['kinv'], b['coeff'], b['landmarks'], props[s], GAMMA, n_prbs, ETA, count=k)
            low = shm.lower_tiles(k)
            Ad = A[:k, :k].T
            for stage, dev, want in (('KF', KF[:k, :cap], mir['KF']), ('DS', DS[:k, :cap], mir['DS']), ('F0', F0[:k], mir['F0']),
                                     ('A', np.where(low, Ad, 0.0), np.where(low, mir['A'], 0.0))):
                ok = values_equal(dev, want) if stage == 'A' else same(dev, want)
                assert ok, tag + ('stage %s' % stage,)
            print(tag, 'branches', np.bincount(mir['branch'], minlength=5).tolist(), 'coefficients that differ',
                  int((a['coeff'] != mir['coeff']).sum()))
            assert same(a['coeff'], mir['coeff']), tag + ('coefficients: %d differ' % int((a['coeff'] != mir['coeff']).sum()),)
            # the one-by-one path forms f_p afresh: other bits in this mode, the same decisions
            assert np.abs(t['coeff'] - a['coeff']).max() <= 1e-8 * np.abs(a['coeff']).max(), tag + ('the one-by-one twin',)
            if k >= 15 and s == 0:
                assert {1, 3, 4} <= set(int(v) for v in mir['branch'])
            changed += mir['n_changed']
            work += mir['n_work']
            sat = sat or mir['sat']
        assert sh.changed == changed == tw.changed, ('samples that changed a dictionary', sh.changed, tw.changed, changed)
        assert sh.work == work == tw.work, ('work[6]: branches 1-4', sh.work, tw.work, work)
        assert bool(sh.flagged_replicas()['saturated']) == (flagged or sat), ('saturation flag', flagged, sat)
    finally:
        sh.close()
        tw.close()


# ------------------------------------------------------------------ (c) rounds with several replicas
def _scan(h, states, actions, labels, rnd, budget, hits):
    counts, props = np.zeros(2, dtype=np.int32), np.zeros((2, budget, 18))
    first = rnd == 0
    h._check(h.L.kb_shared_scan(h.h, _p(states, _fp) if first else None, _p(actions, _ip) if first else None,
                                _p(labels, _ip) if first else None, rnd, budget, _p(hits, _ip), _p(counts, _ip), _p(props, _dp)))
    return counts, props


@pytest.mark.parametrize('budget', [4, 64])
def test_rounds_by_hand_are_the_sequential_learner_and_the_other_entry_points_leave_the_same_bytes(budget):
    from ranslice.kbrl_dev import PROP_W, SharedVecKBRL, merge_proposals
    N, n_prbs, rounds, steps = 24, 50, 4, 12
    assert PROP_W == 18
    ref = spm.PlusRounds(DIMS, n_prbs, N, GAMMA, ETA)
    inputs = shm.round_inputs(N, DIMS, n_prbs, steps, seed=8)
    ia, sf = np.zeros((N, 2), dtype=np.int32), np.full((N, 2), 2, dtype=np.int32)
    kw = dict(budget=budget, max_rounds=rounds, capacity=256, gamma=GAMMA, eta=ETA)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('RANSLICE_DEV_BUILD', raising=False)
        sh = SharedVecKBRL(N, DIMS, n_prbs, shared_plus=True, **kw)
        tw = SharedVecKBRL(N, DIMS, n_prbs, shared_plus=True, **kw)
        parts = [SharedVecKBRL(N // 2, DIMS, n_prbs, shared_plus=True, first_env=w * (N // 2), **kw) for w in range(2)]
        # the host-driven rounds of the class itself (update_control with an exchange callback), a world of one
        cb = SharedVecKBRL(N, DIMS, n_prbs, shared_plus=True, exchange=lambda c, p: (c[None], p[None], 0), **kw)
    try:
        for h in [sh, tw, cb] + parts:
            h.reset(ia[:h.n_envs], sf[:h.n_envs])
            assert h.shared_plus
        seen = dict(rounds=0, over_budget=0, branches=set())
        for step, (states, actions, labels) in enumerate(inputs):
            ref.begin(states, actions, labels)
            hits = np.full((N, 2), -9, dtype=np.int32)
            phits = [np.full((N // 2, 2), -9, dtype=np.int32) for _ in parts]
            for rnd in range(rounds):
                tag = ('step %d' % step, 'round %d' % rnd)
                want, whits, out = ref.scan()
                assert not out.any(), tag + ('pairs within 1e-9 of a threshold: the seeds were chosen so that none is',)
                n_pred = sh.stats()[0]
                counts, props = _scan(sh, states, actions, labels, rnd, budget, hits)
                cnt, lists, wprops = shm.collect(want, budget, states, labels, 0, OFF, DIMS)
                assert (counts == cnt).all(), tag + ('counts', counts, cnt)
                for s in (0, 1):
                    k = min(int(cnt[s]), budget)
                    assert props[s, :k].tobytes() == wprops[s, :k].tobytes(), tag + ('proposals of slice %d' % s,)
                if rnd == 0:
                    assert (hits == whits).all(), tag + ('hits',)
                assert sh.stats()[0] - n_pred == ref.n_pred, tag + ('predictions of the scan',)
                # the two shards: their own scans, the host merge of both
                pc = [_scan(p, np.ascontiguousarray(states[w * 12:(w + 1) * 12]), np.ascontiguousarray(actions[w * 12:(w + 1) * 12]),
                            np.ascontiguousarray(labels[w * 12:(w + 1) * 12]), rnd, budget, phits[w]) for w, p in enumerate(parts)]
                if counts.sum() == 0:
                    assert sum(int(c.sum()) for c, _ in pc) == 0
                    break
                seen['rounds'] += 1
                seen['over_budget'] += int((counts > budget).sum())
                mc, mp_, taken = merge_proposals(counts[None], props[None], budget)
                mc, mp_ = np.ascontiguousarray(mc, dtype=np.int32), np.ascontiguousarray(mp_)
                pmc, pmp, ptaken = merge_proposals(np.stack([c for c, _ in pc]), np.stack([q for _, q in pc]), budget)
                pmc, pmp = np.ascontiguousarray(pmc, dtype=np.int32), np.ascontiguousarray(pmp)
                assert (pmc == mc).all() and all(pmp[s, :mc[s]].tobytes() == mp_[s, :mc[s]].tobytes() for s in (0, 1)), tag + ('the shards\' merged list',)
                before = [sh.learner(0, s, with_kinv=True) for s in (0, 1)]
                c0, w0, g0 = sh.stats()[1], _work6(sh), sh.stats()[2]
                sh._check(sh.L.kb_shared_apply(sh.h, _p(mc, _ip), _p(mp_, _dp), budget))
                sh._check(sh.L.kb_shared_commit(sh.h, _p(np.ascontiguousarray(taken[0], dtype=np.int32), _ip)))
                for w, p in enumerate(parts):
                    p._check(p.L.kb_shared_apply(p.h, _p(pmc, _ip), _p(pmp, _dp), budget))
                    p._check(p.L.kb_shared_commit(p.h, _p(np.ascontiguousarray(ptaken[w], dtype=np.int32), _ip)))
                res = ref.apply(lists)
                brs = []
                for s in (0, 1):
                    a, o, b = sh.learner(0, s, with_kinv=True), ref.oa[s], before[s]
                    assert a['m'] == o.m, tag + ('size of slice %d' % s, a['m'], o.m)
                    assert same(a['landmarks'], o.L), tag + ('landmarks',)
                    np.testing.assert_allclose(a['coeff'], o.c, rtol=1e-8, atol=1e-9)
                    np.testing.assert_allclose(a['kinv'], o.P, rtol=1e-8, atol=1e-8 * np.abs(o.P).max())
                    g = spm.growing_apply_plus(b['kinv'] if b['m'] else np.zeros((0, 0)), b['coeff'], b['landmarks'], mp_[s], GAMMA, n_prbs,
                                               DIMS[s] + 1, ETA, 256, count=int(mc[s]))
                    assert [int(v) for v in g['branch']] == [br for _, br in res[s]], tag + ('branches of slice %d' % s,)
                    assert g['m'] == a['m'] and same(g['coeff'], a['coeff']) and same(g['kinv'], a['kinv']), tag + (
                        'the mirror of the one-by-one apply, slice %d: coefficients %d, Kinv %d differ' % (
                            s, int((g['coeff'] != a['coeff']).sum()), int((g['kinv'] != a['kinv']).sum())),)
                    brs += [int(v) for v in g['branch']]
                seen['branches'] |= set(brs)
                assert sh.stats()[1] - c0 == sum(1 for v in brs if v in (1, 2, 3)), tag + ('kb_get_stats[1]',)
                assert sh.stats()[2] - g0 == brs.count(2), tag + ('kb_get_stats[2]',)
                assert _work6(sh) - w0 == sum(1 for v in brs if v), tag + ('work[6]',)
                ref.commit([len(l) for l in lists])
            assert (tw.update_control(states, actions, labels) == hits).all(), ('kb_shared_step: hits', step)
            assert (np.concatenate(phits) == hits).all(), ('the shards\' hits', step)
            assert (cb.update_control(states, actions, labels) == hits).all(), ('update_control through the exchange callback: hits', step)
        assert ref.open == 0 and ref.near == 0, (ref.open, ref.near, ref.samples)
        # branch 4 too: a sample that changes nothing counts in work[6] alone, and what follows it is predicted again
        assert seen['branches'] >= {1, 2, 3, 4} and (budget >= N or seen['over_budget'] > 0), seen
        for s in (0, 1):
            a = sh.learner(0, s, with_kinv=True)
            assert a['m'] >= 3
            for name, h in [('kb_shared_step', tw), ('shard 0', parts[0]), ('shard 1', parts[1]), ('the exchange callback', cb)]:
                t = h.learner(0, s, with_kinv=True)
                assert a['m'] == t['m'], (name, s)
                for k in ('landmarks', 'coeff', 'kinv'):
                    assert same(a[k], t[k]), (name + ' leaves other bytes than the rounds by hand', s, k)
        print('rounds budget %d: %s; sizes %s' % (budget, seen, [sh.learner(0, s)['m'] for s in (0, 1)]))
    finally:
        for h in [sh, tw, cb] + parts:
            h.close()


# ------------------------------------------------------------------ (d) one replica is the sequential loop
def test_one_replica_equals_fit_steps_in_projectron_plus_mode():
    """one replica, one proposal a round, rounds enough for every candidate of a step: the reference's sequential loop with a
    ProjectronPlus learner, which kb_fit_steps runs per replica.  The two storages sum d* in different orders: no bits claimed.
    Compared per step: the samples that changed a dictionary (branches 1-3), the insertions (branch 2) and the sizes -- all that
    fit_steps reports.  Branch 4 and work[6] are NOT compared on this path: kb_fit_steps counts neither per row and does not add
    to kb_get_repair_work (the rounds test above checks work[6] per round against the mirror's branches)."""
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    n_prbs, steps = 15, 10
    inputs = shm.round_inputs(1, DIMS, n_prbs, steps, seed=5)
    sh = SharedVecKBRL(1, DIMS, n_prbs, budget=4, max_rounds=n_prbs + 2, capacity=256, gamma=GAMMA, eta=ETA, shared_plus=True)
    pr = VecKBRL(1, DIMS, n_prbs, capacity=256, gamma=GAMMA, eta=ETA, algorithm='projectron_plus')
    try:
        ia, sf = np.zeros((1, 2), dtype=np.int32), np.full((1, 2), 2, dtype=np.int32)
        sh.reset(ia, sf)
        pr.reset(ia, sf)
        for states, actions, labels in inputs:
            c0, g0 = sh.stats()[1], sh.stats()[2]
            sh.update_control(states, actions, labels)
            assert sh.rounds_last <= n_prbs + 1
            r = pr.fit_steps([0], [states], [actions], [labels])
            assert sh.stats()[1] - c0 == int(r['changed'][0].sum()) and sh.stats()[2] - g0 == int(r['grown'][0].sum())
            assert list(sh.dictionary_sizes()) == list(r['m'][0][-1])
        for s in (0, 1):
            a, b = sh.learner(0, s, with_kinv=True), pr.learner(0, s, with_kinv=True)
            assert a['m'] == b['m'] >= 2 and same(a['landmarks'], b['landmarks'])
            np.testing.assert_allclose(a['coeff'], b['coeff'], rtol=1e-8, atol=1e-9)
            np.testing.assert_allclose(a['kinv'], b['kinv'], rtol=1e-8, atol=1e-8 * np.abs(b['kinv']).max())
    finally:
        sh.close()
        pr.close()


# ------------------------------------------------------------------ (e) the switch leaves Projectron alone
def test_the_switch_off_is_projectron_byte_for_byte(golden_dir):
    """ten resident steps on three handles: the switch never set, set to 0, set to 1 and back to 0 before the first step.  Equal as
    bytes: dictionaries, control state, statistics, kb_get_repair_work, and the histories.  kb_shared_step_resident records no
    column of kb_history_begin's arrays (only kb_step_resident does: history_fetch answers `recorded` 0 on a shared handle, on
    the parent commit as here), so the histories are compared twice: what history_fetch returns on the three handles, and the
    quantities its columns are made of -- reward, allocations, SLA labels, violations, and the observations -- fetched from the
    simulator after every step."""
    from ranslice.config import make_config
    from ranslice.kbrl_dev import SharedVecKBRL
    from ranslice.vec_env import VecRanSlice
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    fading = [g['t0'], g['t1'], g['t2']]
    N, n_prbs = 8, 200
    ia = np.tile(np.array([10, 5], dtype=np.int32), (N, 1))
    sf = np.tile(np.array([3, 2], dtype=np.int32), (N, 1))
    outs = []
    for kind in ('never', 'zero', 'back'):
        env = VecRanSlice(n_envs=N, cfg=make_config(3, n_envs=N, n_prbs=n_prbs), fading=fading, seed=5)
        h = SharedVecKBRL(N, DIMS, n_prbs, budget=8, max_rounds=2, capacity=64)
        try:
            env.reset()
            h.reset(ia, sf)
            if kind == 'zero':
                h.set_shared_plus(False)
            if kind == 'back':
                h.set_shared_plus(True)
                assert h.shared_plus
                h.set_shared_plus(False)
            assert not h.shared_plus
            env.step(ia)
            viol = []
            h.history_begin(10)
            for _ in range(10):
                h.step_resident(env)
                env.step_resident()
                viol.append(env.fetch())
            h.synchronize()
            ctl = h.control()
            hist = h.history_fetch()
            assert hist['recorded'] == 0      # (see the docstring)
            outs.append(dict(dic=[h.learner(0, s, with_kinv=True) for s in (0, 1)], ctl=ctl, stats=h.stats(), work=h._repair_raw(),
                             steps={q: np.stack([v[q] for v in viol]) for q in viol[0]}, hist=hist))
        finally:
            h.close()
            env.close()
    a = outs[0]
    hist_keys = {'actions', 'obs', 'reward', 'labels', 'violations'}
    assert a['stats'][1] > 0 and a['dic'][0]['m'] > 0 and a['steps']['violations'].shape[0] == 10
    assert len({a['steps']['actions'][i].tobytes() for i in range(10)}) > 1      # (the fleet acts on what it learns)
    for b in outs[1:]:
        assert a['stats'] == b['stats'] and a['work'] == b['work']
        assert hist_keys == set(b['steps'])
        for q in hist_keys:      # the per-step histories, from the simulator
            assert a['steps'][q].tobytes() == b['steps'][q].tobytes(), ('per step', q)
        assert a['hist']['recorded'] == b['hist']['recorded']
        for q in ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation'):      # the handle's own histories
            assert a['hist'][q].tobytes() == b['hist'][q].tobytes(), ('history', q)
        for q in ('margins', 'security_factors', 'action', 'adjusted', 'accuracies'):
            assert a['ctl'][q].tobytes() == b['ctl'][q].tobytes(), q
        for s in (0, 1):
            assert a['dic'][s]['m'] == b['dic'][s]['m']
            for k in ('landmarks', 'coeff', 'kinv'):
                assert same(a['dic'][s][k], b['dic'][s][k]), (s, k)


# ------------------------------------------------------------------ (f) refusals
def test_refusals():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    sh = SharedVecKBRL(4, DIMS, 50, budget=4, capacity=64)
    pr = VecKBRL(1, DIMS, 50, capacity=64)
    try:
        L = sh.L
        err = lambda h: L.kb_last_error(h.h).decode()
        for v in (2, -1):
            assert L.kb_set_shared_plus(sh.h, v) == _lib.RS_EINVAL
        on = C.c_int32(7)
        assert L.kb_get_shared_plus(sh.h, C.byref(on)) == 0 and on.value == 0          # off by default
        assert L.kb_get_shared_plus(sh.h, None) == _lib.RS_EINVAL
        assert L.kb_set_shared_plus(pr.h, 1) == _lib.RS_ESTATE and 'kb_set_control_plus' in err(pr)
        assert L.kb_set_shared_plus(pr.h, 0) == _lib.RS_ESTATE
        assert L.kb_set_shared_plus(sh.h, 1) == 0 and sh.shared_plus
        alg = C.c_int32(9)
        assert L.kb_get_algorithm(sh.h, C.byref(alg)) == 0 and alg.value == 0          # KB_ALG_PROJECTRON still
        # a round open between scan and commit
        sh.reset(np.zeros((4, 2), dtype=np.int32), np.full((4, 2), 2, dtype=np.int32))
        states, actions, labels = shm.round_inputs(4, DIMS, 50, 1, seed=3)[0]
        hits = np.zeros((4, 2), dtype=np.int32)
        counts, props = _scan(sh, states, actions, labels, 0, 4, hits)
        assert counts.sum() > 0
        assert L.kb_set_shared_plus(sh.h, 0) == _lib.RS_ESTATE and 'round' in err(sh)
        assert sh.shared_plus
        sh._check(L.kb_shared_apply(sh.h, _p(np.minimum(counts, 4).astype(np.int32), _ip), _p(props, _dp), 4))
        assert L.kb_set_shared_plus(sh.h, 0) == _lib.RS_ESTATE
        sh._check(L.kb_shared_commit(sh.h, _p(np.minimum(counts, 4).astype(np.int32), _ip)))
        assert L.kb_set_shared_plus(sh.h, 0) == 0 and not sh.shared_plus
        # the other Projectron++ switches refuse the shared handle as they did, whatever this one says
        sh.set_shared_plus(True)
        assert L.kb_set_algorithm(sh.h, 1) == _lib.RS_ESTATE
        for call in (lambda: L.kb_set_control_plus(sh.h, 1), lambda: L.kb_set_control_plus_batch(sh.h, 4, 64),
                     lambda: L.kb_set_control_plus_wide(sh.h, 64, 64, 4), lambda: L.kb_set_fit_wide_plus(sh.h, 1),
                     lambda: L.kb_set_fit_steps_batch(sh.h, 4, 64)):
            assert call() == _lib.RS_ESTATE and 'shared' in err(sh)
        for m in (sh.set_control_plus, lambda: sh.set_control_plus_batch(4), lambda: sh.set_control_plus_wide(64)):
            with pytest.raises(_lib.RanSliceError):
                m()
    finally:
        sh.close()
        pr.close()


# ------------------------------------------------------------------ (g) together with kb_shared_prune
def test_shrink_between_two_margin_rule_steps():
    import test_gpu_shared_prune as pt
    ag = pt._grown((128, 128), 128)
    X = ag.to_shared(0, 8)
    try:
        X.set_shared_plus(True)
        rng = np.random.default_rng(23)
        st, ac, lb = pt._control_batch(rng, 8)
        c0 = X.stats()[1]
        X.update_control(st, ac, lb)
        assert list(X.dictionary_sizes()) == [128, 128] and X.stats()[1] > c0
        used = X.pool()['used_bytes']
        assert X.shrink(64) == 128 and list(X.dictionary_sizes()) == [64, 64]
        assert X.shared_plus                        # neither carried nor changed by the prune
        st, ac, lb = pt._control_batch(rng, 8)
        X.update_control(st, ac, lb)
        assert X.dictionary_sizes().min() >= 64 and X.dictionary_sizes().max() <= 128
        assert X.pool()['used_bytes'] == used
        one = X.to_agents([0])
        try:
            assert X.shared_plus
            for s in (0, 1):
                k = one.learner(0, s, with_kinv=True)['kinv']
                assert k.shape[0] == X.dictionary_sizes()[s] and same(np.triu(k), np.triu(k.T)), ('Kinv: the upper triangle is the transpose', s)
        finally:
            one.close()
    finally:
        X.close()
