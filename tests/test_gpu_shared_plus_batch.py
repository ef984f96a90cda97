"""The segmented apply of growing shared dictionaries under the margin rule ON THE DEVICE (kb_set_shared_plus_batch; DESIGN.md
section 8r; csrc/kb_shared_plus_batch.hip) against tests/shared_plus_batch_mirror.py.

  (a) apply     kb_shared_apply of shared_plus_batch_mirror's lists on dictionaries that can still grow: landmarks, every
                coefficient, all of Kinv, the size, the changed / inserted / work[6] counts and work[0..3] of
                kb_shared_plus_batch_info equal segmented_apply_plus as bits; a twin under KBRL_SERIAL_APPLY=1 takes the same branches
                and counts and ends within 1e-8.
  (b) segments  0, 1, 4 and 16 segment rounds leave the same bytes; the finishing launch works at 0 and idles at 16.
  (c) min_landmarks is respected.
  (d) rounds    24 replicas from empty, rounds by hand beside PlusRounds with the segmented mirror as its apply; kb_shared_step on a
                twin, update_control through an exchange callback, two shards through the host merge.
  (e) the switch off, or set and taken back, leaves the parent's path byte for byte (ten resident steps).
  (f) refusals; kb_save_state blobs do not carry the switch.  (g) together with kb_shared_prune.
"""
import ctypes as C
import os

import numpy as np
import pytest

import shared_mirror as shm
import shared_plus_batch_mirror as sbm
import shared_plus_mirror as spm
import test_gpu_shared_chain as chain

pytestmark = pytest.mark.gpu

GAMMA, ETA = chain.GAMMA, chain.ETA
DIMS, OFF = chain.DIMS, chain.OFF
_ip, _dp, _fp = chain._ip, chain._dp, chain._fp
_p, same = chain._p, chain.same
N_PRBS = 200


def _work6(h):
    return int(h._repair_raw()[6])


def _setup(case, serial=False):
    """-> (the shared handle of the case's dictionary, its slice, the budget)"""
    m, dims, n, ins, extra = case
    s = 0 if dims == 10 else 1
    ag = chain.grown(N_PRBS, m + extra, [(m, 2) if s == 0 else (2, m)])
    return chain.shared_of(ag, 0, 1, max(n, 2), serial=serial), s, max(n, 2)


_lists = {}


def _list_of(case, before):
    """the case's list against the dictionary as the device holds it, and the mirror's answer"""
    if case not in _lists:
        m, dims, n, ins, extra = case
        props, seq = sbm.batch_list(before['kinv'], before['coeff'], before['landmarks'], N_PRBS, n, ins, m + extra, GAMMA, ETA, seed=m + n)
        mir = sbm.segmented_apply_plus(before['kinv'], before['coeff'], before['landmarks'], props, GAMMA, N_PRBS, dims + 1, ETA, m + extra, 2)
        assert mir['near'] == 0, 'applied samples within CLEARANCE of a threshold: the seeds were to leave none'
        assert mir['branch'].tolist() == seq
        _lists[case] = (props, mir)
    return _lists[case]


def _apply(h, s, props, n, budget):
    """the list to slice s of h, the other slice none -> (changed, inserted, work[6]) of the call"""
    P, counts = np.zeros((2, budget, 18)), np.zeros(2, dtype=np.int32)
    P[s, :n] = props[:n]
    counts[s] = n
    c0, g0, w0 = h.stats()[1], h.stats()[2], _work6(h)
    h._check(h.L.kb_shared_apply(h.h, _p(counts, _ip), _p(P, _dp), budget))
    h._check(h.L.kb_shared_commit(h.h, _p(np.zeros(2, dtype=np.int32), _ip)))
    return h.stats()[1] - c0, h.stats()[2] - g0, _work6(h) - w0


# ------------------------------------------------------------------ (a) the segmented apply against the mirror, as bits
@pytest.mark.parametrize('case', sbm.BATCH_CASES)
def test_segmented_apply_is_the_mirrors_bits(case):
    m, dims, n, ins, extra = case
    sh, s, budget = _setup(case)
    tw = _setup(case, serial=True)[0]
    try:
        before = sh.learner(0, s, with_kinv=True)
        other = sh.learner(0, 1 - s, with_kinv=True)
        assert before['m'] == m
        props, mir = _list_of(case, before)
        flagged = bool(sh.flagged_replicas()['saturated'])
        for h in (sh, tw):
            h.set_shared_plus(True)
            h.set_shared_plus_batch(2, 4)
            assert h.shared_plus_batch == (2, 4)
        got, got_tw = _apply(sh, s, props, n, budget), _apply(tw, s, props, n, budget)
        a, t = sh.learner(0, s, with_kinv=True), tw.learner(0, s, with_kinv=True)
        tag = (case,)
        print(tag, 'branches', np.bincount(mir['branch'], minlength=5).tolist(), 'work', sh.shared_plus_batch_work(), 'differ: coeff',
              int((a['coeff'] != mir['coeff']).sum()) if a['m'] == mir['m'] else 'size', 'Kinv',
              int((a['kinv'] != mir['kinv']).sum()) if a['m'] == mir['m'] else 'size')
        assert a['m'] == mir['m'] == t['m'], tag + ('sizes', a['m'], mir['m'], t['m'])
        assert same(a['landmarks'], mir['landmarks']) and same(t['landmarks'], mir['landmarks']), tag + ('landmarks',)
        assert same(a['coeff'], mir['coeff']), tag + ('coefficients: %d differ' % int((a['coeff'] != mir['coeff']).sum()),)
        assert same(a['kinv'], mir['kinv']), tag + ('Kinv: %d differ' % int((a['kinv'] != mir['kinv']).sum()),)
        want = (mir['n_changed'], mir['n_grow'], mir['n_work'])
        assert got == want == got_tw, tag + ('changed, inserted, work[6]', got, got_tw, want)
        w = sh.shared_plus_batch_work()
        assert w[:4] == mir['work'] and w[5:] == [0, 0, 0], tag + ('kb_shared_plus_batch_info', w, mir['work'])
        assert w[4] == max(0, mir['work'][1] - 4)
        assert tw.shared_plus_batch_work() == [0] * 8      # (the serial apply engages nothing)
        assert bool(sh.flagged_replicas()['saturated']) == (flagged or mir['sat']) == bool(tw.flagged_replicas()['saturated'])
        # the one-by-one twin forms every f_p afresh: the same branches (the counts above), other bits
        assert np.abs(t['coeff'] - a['coeff']).max() <= 1e-8 * np.abs(a['coeff']).max(), tag + ('the one-by-one twin: coefficients',)
        assert np.abs(t['kinv'] - a['kinv']).max() <= 1e-8 * np.abs(a['kinv']).max(), tag + ('the one-by-one twin: Kinv',)
        # the slice without proposals keeps every byte
        o = sh.learner(0, 1 - s, with_kinv=True)
        assert o['m'] == other['m'] and all(same(o[k], other[k]) for k in ('landmarks', 'coeff', 'kinv'))
    finally:
        sh.close()
        tw.close()


# ------------------------------------------------------------------ (b) the number of segment rounds does not enter the result
def test_the_result_does_not_depend_on_the_segment_rounds():
    case = sbm.BATCH_CASES[6]      # 64 proposals, three insertions: four segments
    m, dims, n, ins, extra = case
    outs = {}
    for segments in (0, 1, 4, 16):
        sh, s, budget = _setup(case)
        try:
            props, mir = _list_of(case, sh.learner(0, s, with_kinv=True))
            sh.set_shared_plus(True)
            sh.set_shared_plus_batch(2, segments)
            counts = _apply(sh, s, props, n, budget)
            outs[segments] = (sh.learner(0, s, with_kinv=True), counts, sh.shared_plus_batch_work(), sh.stats())
        finally:
            sh.close()
    a = outs[4]
    assert a[2][1] == 4 and same(a[0]['coeff'], mir['coeff']) and same(a[0]['kinv'], mir['kinv'])
    for segments, b in outs.items():
        assert b[0]['m'] == a[0]['m'] and all(same(a[0][k], b[0][k]) for k in ('landmarks', 'coeff', 'kinv')), segments
        assert b[1] == a[1] and b[2][:4] == a[2][:4] and b[3] == a[3], (segments, b[1:], a[1:])
        assert b[2][4] == max(0, 4 - segments), (segments, b[2])
    assert outs[0][2][4] > 0 and outs[16][2][4] == 0


# ------------------------------------------------------------------ (c) min_landmarks
def test_min_landmarks_is_respected():
    case = sbm.BATCH_CASES[3]      # 64 landmarks, the insertion first
    m, dims, n, ins, extra = case
    outs = {}
    for kind, lo in (('off', None), ('above', m + 1), ('at', m)):
        sh, s, budget = _setup(case)
        try:
            props, mir = _list_of(case, sh.learner(0, s, with_kinv=True))
            sh.set_shared_plus(True)
            if lo:
                sh.set_shared_plus_batch(lo, 4)
            _apply(sh, s, props, n, budget)
            outs[kind] = (sh.learner(0, s, with_kinv=True), sh.shared_plus_batch_work(), sh.stats(), sh._repair_raw())
        finally:
            sh.close()
    off, above, at = outs['off'], outs['above'], outs['at']
    assert above[1] == [0] * 8 and above[2] == off[2] and above[3] == off[3]
    assert above[0]['m'] == off[0]['m'] and all(same(above[0][k], off[0][k]) for k in ('landmarks', 'coeff', 'kinv'))
    assert at[1][:4] == mir['work'] and at[0]['m'] == mir['m']
    assert same(at[0]['coeff'], mir['coeff']) and same(at[0]['kinv'], mir['kinv']) and same(at[0]['landmarks'], mir['landmarks'])
    # the one-by-one path forms f_p afresh: these inputs tell the two apart
    assert not same(at[0]['coeff'], off[0]['coeff'])
    assert np.abs(at[0]['coeff'] - off[0]['coeff']).max() <= 1e-8 * np.abs(off[0]['coeff']).max()


# ------------------------------------------------------------------ (d) rounds with several replicas
class SegmentedRounds(spm.PlusRounds):
    """PlusRounds whose apply is the segmented mirror: the learners hold the device's bits"""

    def __init__(self, *a, capacity, min_landmarks, **kw):
        super().__init__(*a, **kw)
        self.capacity, self.min_landmarks = capacity, min_landmarks
        self.work = [0, 0, 0, 0]
        self.near_seg = 0

    def apply_props(self, counts, props):
        """counts [S], props [S][budget][18]: the merged lists -> per slice the mirror's result"""
        res = []
        for s in range(len(self.dims)):
            o, d = self.oa[s], self.dims[s] + 1
            L = o.L if o.m else np.zeros((0, d))
            r = sbm.segmented_apply_plus(o.P, o.c, L, props[s], self.gamma, self.n_prbs, d, o.eta, self.capacity, self.min_landmarks,
                                         count=int(counts[s]))
            if r['m']:
                o.L, o.c, o.P = r['landmarks'], r['coeff'], r['kinv']
            self.work = [a + b for a, b in zip(self.work, r['work'])]
            self.near_seg += r['near']
            res.append(r)
        return res


@pytest.mark.parametrize('budget', [4, 64])
def test_rounds_by_hand_are_the_segmented_mirror_and_the_other_entry_points_leave_the_same_bytes(budget):
    from ranslice.kbrl_dev import SharedVecKBRL, merge_proposals
    N, n_prbs, rounds, steps = 24, 50, 4, 12
    ref = SegmentedRounds(DIMS, n_prbs, N, GAMMA, ETA, capacity=256, min_landmarks=2)
    inputs = shm.round_inputs(N, DIMS, n_prbs, steps, seed=8)
    ia, sf = np.zeros((N, 2), dtype=np.int32), np.full((N, 2), 2, dtype=np.int32)
    kw = dict(budget=budget, max_rounds=rounds, capacity=256, gamma=GAMMA, eta=ETA, shared_plus=True, shared_plus_batch=2)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv('RANSLICE_DEV_BUILD', raising=False)
        sh = SharedVecKBRL(N, DIMS, n_prbs, **kw)
        tw = SharedVecKBRL(N, DIMS, n_prbs, shared_plus_segments=1, **kw)
        parts = [SharedVecKBRL(N // 2, DIMS, n_prbs, first_env=w * (N // 2), shared_plus_segments=2 * w, **kw) for w in range(2)]
        cb = SharedVecKBRL(N, DIMS, n_prbs, exchange=lambda c, p: (c[None], p[None], 0), **kw)
    try:
        for h in [sh, tw, cb] + parts:
            h.reset(ia[:h.n_envs], sf[:h.n_envs])
            assert h.shared_plus and h.shared_plus_batch[0] == 2
        seen = dict(rounds=0, branches=set(), engaged=0)
        for step, (states, actions, labels) in enumerate(inputs):
            ref.begin(states, actions, labels)
            hits = np.full((N, 2), -9, dtype=np.int32)
            phits = [np.full((N // 2, 2), -9, dtype=np.int32) for _ in parts]
            for rnd in range(rounds):
                tag = ('step %d' % step, 'round %d' % rnd)
                want, whits, out = ref.scan()
                assert not out.any(), tag + ('pairs within 1e-9 of a threshold: the seeds were chosen so that none is',)
                counts, props = _scan(sh, states, actions, labels, rnd, budget, hits)
                cnt, lists, wprops = shm.collect(want, budget, states, labels, 0, OFF, DIMS)
                assert (counts == cnt).all(), tag + ('counts', counts, cnt)
                for s in (0, 1):
                    k = min(int(cnt[s]), budget)
                    assert props[s, :k].tobytes() == wprops[s, :k].tobytes(), tag + ('proposals of slice %d' % s,)
                if rnd == 0:
                    assert (hits == whits).all(), tag + ('hits',)
                pc = [_scan(p, np.ascontiguousarray(states[w * 12:(w + 1) * 12]), np.ascontiguousarray(actions[w * 12:(w + 1) * 12]),
                            np.ascontiguousarray(labels[w * 12:(w + 1) * 12]), rnd, budget, phits[w]) for w, p in enumerate(parts)]
                if counts.sum() == 0:
                    assert sum(int(c.sum()) for c, _ in pc) == 0
                    break
                seen['rounds'] += 1
                mc, mp_, taken = merge_proposals(counts[None], props[None], budget)
                mc, mp_ = np.ascontiguousarray(mc, dtype=np.int32), np.ascontiguousarray(mp_)
                pmc, pmp, ptaken = merge_proposals(np.stack([c for c, _ in pc]), np.stack([q for _, q in pc]), budget)
                pmc, pmp = np.ascontiguousarray(pmc, dtype=np.int32), np.ascontiguousarray(pmp)
                assert (pmc == mc).all() and all(pmp[s, :mc[s]].tobytes() == mp_[s, :mc[s]].tobytes() for s in (0, 1)), tag + ('the shards\' merged list',)
                c0, w0, g0 = sh.stats()[1], _work6(sh), sh.stats()[2]
                sh._check(sh.L.kb_shared_apply(sh.h, _p(mc, _ip), _p(mp_, _dp), budget))
                sh._check(sh.L.kb_shared_commit(sh.h, _p(np.ascontiguousarray(taken[0], dtype=np.int32), _ip)))
                for w, p in enumerate(parts):
                    p._check(p.L.kb_shared_apply(p.h, _p(pmc, _ip), _p(pmp, _dp), budget))
                    p._check(p.L.kb_shared_commit(p.h, _p(np.ascontiguousarray(ptaken[w], dtype=np.int32), _ip)))
                res = ref.apply_props(mc, mp_)
                brs = []
                for s in (0, 1):
                    a, r = sh.learner(0, s, with_kinv=True), res[s]
                    assert a['m'] == r['m'], tag + ('size of slice %d' % s, a['m'], r['m'])
                    if a['m']:
                        assert same(a['landmarks'], r['landmarks']), tag + ('landmarks of slice %d' % s,)
                        assert same(a['coeff'], r['coeff']) and same(a['kinv'], r['kinv']), tag + (
                            'slice %d: coefficients %d, Kinv %d differ' % (s, int((r['coeff'] != a['coeff']).sum()), int((r['kinv'] != a['kinv']).sum())),)
                    brs += [int(v) for v in r['branch']]
                    seen['engaged'] += int(r['engaged'])
                seen['branches'] |= set(brs)
                assert sh.stats()[1] - c0 == sum(1 for v in brs if v in (1, 2, 3)), tag + ('kb_get_stats[1]',)
                assert sh.stats()[2] - g0 == brs.count(2), tag + ('kb_get_stats[2]',)
                assert _work6(sh) - w0 == sum(1 for v in brs if v), tag + ('work[6]',)
                assert sh.shared_plus_batch_work()[:4] == ref.work, tag + ('kb_shared_plus_batch_info', sh.shared_plus_batch_work(), ref.work)
                ref.commit([len(l) for l in lists])
            assert (tw.update_control(states, actions, labels) == hits).all(), ('kb_shared_step: hits', step)
            assert (np.concatenate(phits) == hits).all(), ('the shards\' hits', step)
            assert (cb.update_control(states, actions, labels) == hits).all(), ('update_control through the exchange callback: hits', step)
        assert ref.open == 0 and ref.near_seg == 0, (ref.open, ref.near_seg)
        assert seen['branches'] >= {1, 2, 3, 4} and seen['engaged'] > 0 and ref.work[3] > 0, (seen, ref.work)
        for s in (0, 1):
            a = sh.learner(0, s, with_kinv=True)
            assert a['m'] >= 3
            for name, h in [('kb_shared_step', tw), ('shard 0', parts[0]), ('shard 1', parts[1]), ('the exchange callback', cb)]:
                t = h.learner(0, s, with_kinv=True)
                assert a['m'] == t['m'], (name, s)
                for k in ('landmarks', 'coeff', 'kinv'):
                    assert same(a[k], t[k]), (name + ' leaves other bytes than the rounds by hand', s, k)
        print('rounds budget %d: %s; work %s; sizes %s' % (budget, seen, ref.work, [sh.learner(0, s)['m'] for s in (0, 1)]))
    finally:
        for h in [sh, tw, cb] + parts:
            h.close()


def _scan(h, states, actions, labels, rnd, budget, hits):
    counts, props = np.zeros(2, dtype=np.int32), np.zeros((2, budget, 18))
    first = rnd == 0
    h._check(h.L.kb_shared_scan(h.h, _p(states, _fp) if first else None, _p(actions, _ip) if first else None,
                                _p(labels, _ip) if first else None, rnd, budget, _p(hits, _ip), _p(counts, _ip), _p(props, _dp)))
    return counts, props


# ------------------------------------------------------------------ (e) the switch off is the parent's path
def test_the_switch_off_is_the_margin_rule_byte_for_byte(golden_dir):
    """ten resident steps under kb_set_shared_plus on three handles: the batch switch never set, set to 0, set and taken back before
    the first step.  Equal as bytes: dictionaries, control state, statistics, kb_get_repair_work."""
    from ranslice.config import make_config
    from ranslice.kbrl_dev import SharedVecKBRL
    from ranslice.vec_env import VecRanSlice
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    fading = [g['t0'], g['t1'], g['t2']]
    N, n_prbs = 8, 200
    ia = np.tile(np.array([10, 5], dtype=np.int32), (N, 1))
    sf = np.tile(np.array([3, 2], dtype=np.int32), (N, 1))
    outs = []
    for kind in ('never', 'zero', 'back', 'on'):
        env = VecRanSlice(n_envs=N, cfg=make_config(3, n_envs=N, n_prbs=n_prbs), fading=fading, seed=5)
        h = SharedVecKBRL(N, DIMS, n_prbs, budget=8, max_rounds=2, capacity=64, shared_plus=True)
        try:
            env.reset()
            h.reset(ia, sf)
            if kind == 'zero':
                h.set_shared_plus_batch(0, 4)
            if kind == 'back':
                h.set_shared_plus_batch(2, 4)
                assert h.shared_plus_batch == (2, 4)
                h.set_shared_plus_batch(None)
            if kind == 'on':
                h.set_shared_plus_batch(2, 4)
            else:
                assert h.shared_plus_batch[0] == 0
            env.step(ia)
            for _ in range(10):
                h.step_resident(env)
                env.step_resident()
                env.fetch()
            h.synchronize()
            outs.append(dict(dic=[h.learner(0, s, with_kinv=True) for s in (0, 1)], ctl=h.control(), stats=h.stats(), work=h._repair_raw(),
                             info=h.shared_plus_batch_work()))
        finally:
            h.close()
            env.close()
    a, on = outs[0], outs[3]
    assert a['stats'][1] > 0 and a['dic'][0]['m'] > 1
    for b in outs[1:3]:
        assert a['stats'] == b['stats'] and a['work'] == b['work'] and b['info'] == [0] * 8
        for q in ('margins', 'security_factors', 'action', 'adjusted', 'accuracies'):
            assert a['ctl'][q].tobytes() == b['ctl'][q].tobytes(), q
        for s in (0, 1):
            assert a['dic'][s]['m'] == b['dic'][s]['m']
            for k in ('landmarks', 'coeff', 'kinv'):
                assert same(a['dic'][s][k], b['dic'][s][k]), (s, k)
    assert on['info'][0] > 0 and on['info'][1] >= on['info'][0]      # (the resident loop goes through the segments when it is on)


# ------------------------------------------------------------------ (f) refusals
def test_refusals_and_the_switch_is_in_no_saved_state():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    sh = SharedVecKBRL(4, DIMS, 50, budget=4, capacity=64)
    ot = SharedVecKBRL(4, DIMS, 50, budget=4, capacity=64)
    pr = VecKBRL(1, DIMS, 50, capacity=64)
    try:
        L = sh.L
        err = lambda h: L.kb_last_error(h.h).decode()
        a, b = C.c_int32(7), C.c_int32(7)
        assert L.kb_get_shared_plus_batch(sh.h, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)      # off by default
        for lo, seg in ((1, 4), (-1, 4), (65, 4), (2, -1), (2, 17), (0, 17)):
            assert L.kb_set_shared_plus_batch(sh.h, lo, seg) == _lib.RS_EINVAL, (lo, seg)
            assert ('segments' if seg in (-1, 17) and lo in (0, 2) else 'min_landmarks') in err(sh)
        assert L.kb_set_shared_plus_batch(None, 2, 4) == _lib.RS_EINVAL
        assert L.kb_get_shared_plus_batch(sh.h, None, C.byref(b)) == _lib.RS_EINVAL
        assert L.kb_get_shared_plus_batch(sh.h, C.byref(a), None) == _lib.RS_EINVAL
        assert L.kb_shared_plus_batch_info(sh.h, None) == _lib.RS_EINVAL and L.kb_shared_plus_batch_info(None, (C.c_uint64 * 8)()) == _lib.RS_EINVAL
        assert L.kb_set_shared_plus_batch(pr.h, 2, 4) == _lib.RS_ESTATE and 'shared' in err(pr)
        assert L.kb_set_shared_plus_batch(pr.h, 0, 0) == _lib.RS_ESTATE
        # remembered while kb_set_shared_plus is off; the ends of both ranges
        assert L.kb_set_shared_plus_batch(sh.h, 64, 16) == 0 and sh.shared_plus_batch == (64, 16) and not sh.shared_plus
        assert L.kb_set_shared_plus_batch(sh.h, 2, 0) == 0 and sh.shared_plus_batch == (2, 0)
        sh.set_shared_plus(True)
        assert sh.shared_plus_batch == (2, 0)
        # a round open between scan and commit
        sh.reset(np.zeros((4, 2), dtype=np.int32), np.full((4, 2), 2, dtype=np.int32))
        assert sh.shared_plus_batch == (2, 0) and sh.shared_plus_batch_work() == [0] * 8
        states, actions, labels = shm.round_inputs(4, DIMS, 50, 1, seed=3)[0]
        hits = np.zeros((4, 2), dtype=np.int32)
        counts, props = _scan(sh, states, actions, labels, 0, 4, hits)
        assert counts.sum() > 0
        assert L.kb_set_shared_plus_batch(sh.h, 0, 0) == _lib.RS_ESTATE and 'round' in err(sh)
        sh._check(L.kb_shared_apply(sh.h, _p(np.minimum(counts, 4).astype(np.int32), _ip), _p(props, _dp), 4))
        assert L.kb_set_shared_plus_batch(sh.h, 2, 4) == _lib.RS_ESTATE
        sh._check(L.kb_shared_commit(sh.h, _p(np.minimum(counts, 4).astype(np.int32), _ip)))
        assert sh.shared_plus_batch == (2, 0)
        assert L.kb_set_shared_plus_batch(sh.h, 2, 4) == 0
        # a saved state does not carry the switch: loaded into a handle that never set it, it stays off there
        ot.reset(np.zeros((4, 2), dtype=np.int32), np.full((4, 2), 2, dtype=np.int32))
        blob = sh.save_state()
        ot.load_state(blob)
        assert ot.shared_plus_batch == (0, 0) and not ot.shared_plus and sh.shared_plus_batch == (2, 4)
        assert list(ot.dictionary_sizes()) == list(sh.dictionary_sizes())
        sh.load_state(blob)
        assert sh.shared_plus_batch == (2, 4) and sh.shared_plus
    finally:
        sh.close()
        ot.close()
        pr.close()


# ------------------------------------------------------------------ (g) together with kb_shared_prune
def test_shrink_between_two_segmented_steps():
    import test_gpu_shared_prune as pt
    ag = pt._grown((100, 100), 128)
    X = ag.to_shared(0, 8)
    try:
        X.set_shared_plus(True)
        X.set_shared_plus_batch(2, 4)
        rng = np.random.default_rng(23)
        st, ac, lb = pt._control_batch(rng, 8)
        c0 = X.stats()[1]
        X.update_control(st, ac, lb)
        w1 = X.shared_plus_batch_work()
        assert X.stats()[1] > c0 and w1[0] > 0 and X.dictionary_sizes().min() >= 100
        held = int(X.dictionary_sizes().sum())
        assert X.shrink(64) == held - 128
        assert list(X.dictionary_sizes()) == [64, 64]
        assert X.shared_plus and X.shared_plus_batch == (2, 4)      # neither carried nor changed by the prune
        st, ac, lb = pt._control_batch(rng, 8)
        X.update_control(st, ac, lb)
        w2 = X.shared_plus_batch_work()
        assert w2[0] > w1[0] and X.dictionary_sizes().min() >= 64 and X.dictionary_sizes().max() <= 128
        one = X.to_agents([0])
        try:
            for s in (0, 1):
                k = one.learner(0, s, with_kinv=True)['kinv']
                assert k.shape[0] == X.dictionary_sizes()[s] and same(np.triu(k), np.triu(k.T)), ('Kinv: the upper triangle is the transpose', s)
        finally:
            one.close()
    finally:
        X.close()
