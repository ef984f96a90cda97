"""kb_shared_prune (SharedVecKBRL.shrink) on the device: bit for bit what kb_prune leaves on the dictionary's unshared copy, on
the storage a shared handle has -- both block triangles of Kinv, one dictionary per slice.

No tolerance anywhere: the reference is the per-replica kb_prune (tests/test_gpu_prune.py holds it to the float64 mirror and the
longdouble inverse), and the claim is equality of bits.  Dictionaries are grown by VecKBRL.fit on random streams over learners
of ten and of three state variables (so the float32-copy path and the plain path both move a landmark), then to_shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_mirror as pm   # noqa: E402
from test_gpu_prune import _random_stream   # noqa: E402
from ranslice import _lib   # noqa: E402
from ranslice.config import make_config   # noqa: E402

pytestmark = pytest.mark.gpu

DIMS, N_PRBS = [10, 3], 200
IA, SF = [10, 5], [3, 2]
VEC, TILE = 30 * 64, 4096
KB_GEMM_M = 256      # shared dictionaries from this size on (and on the candidate grid) are scored for all replicas at once
_ip, _fp, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------------ growing the dictionaries
_grown_cache = {}


def _grown(sizes, capacity, seed=1):
    """ONE per-replica agent whose two learners hold exactly sizes = (m of the learner of ten state variables, m of the one of
    three): kb_fit on the shortest prefixes of two random streams that reach them"""
    key = (tuple(sizes), capacity, seed)
    if key in _grown_cache:
        return _grown_cache[key]
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(1, DIMS, N_PRBS, capacity=capacity, pool_bytes=64 << 20)
    rng = np.random.default_rng(seed)
    x0, y0 = _random_stream(rng, 11, 900)
    x1, y1 = _random_stream(rng, 4, 1600, spread=4.0)   # (three state variables: spread out, or a few dozen landmarks span them)
    learners = [(0, 0), (0, 1)]
    ag.reset([IA], [SF])
    r = ag.fit(learners, [x0, x1], [y0, y1])
    cuts = []
    for s in (0, 1):
        m = np.asarray(r['m'][s])
        assert m.max() >= sizes[s], (s, m.max())
        cuts.append(int(np.argmax(m >= sizes[s])) + 1)
    ag.reset([IA], [SF])
    ag.fit(learners, [x0[:cuts[0]], x1[:cuts[1]]], [y0[:cuts[0]], y1[:cuts[1]]])
    assert list(ag.dictionary_sizes()[0]) == list(sizes)
    _grown_cache[key] = ag
    return ag


def _dictionaries(h):
    return [h.learner(0, s, with_kinv=True) for s in range(2)]


def _same_dictionaries(a, b, what):
    for s, (la, lb) in enumerate(zip(a, b)):
        assert la['m'] == lb['m'], (what, s)
        for q in ('landmarks', 'coeff', 'kinv'):
            assert _bits(la[q]) == _bits(lb[q]), (what, s, q)


def _victim(before, after):
    """the slot one removal took its landmark from, read off the landmark arrays: the last landmark moved into it"""
    m = len(before)
    assert len(after) == m - 1
    if np.array_equal(after, before[:m - 1]):
        return m - 1
    moved = np.nonzero((after != before[:m - 1]).any(axis=1))[0]
    assert len(moved) == 1 and np.array_equal(after[moved[0]], before[m - 1])
    return int(moved[0])


# ---- the checkpoint blob of a shared handle as a window on its device state: kb_state_header, then the arrays in allocation order
def _views(sh, blob):
    N, S, nv, n_prbs = sh.n_envs, sh.S, sh.nv, sh.n_prbs
    T, ND = N * S, S
    max_shells = (sh.capacity + 63) // 64
    capr = max_shells * 64
    used = int(np.frombuffer(blob[24:32].tobytes(), dtype=np.uint64)[0])    # kb_state_header.pool_doubles_used
    sizes = [('m', ND * 4), ('shell', ND * max_shells * 8), ('head', ND * 256 * 4), ('pool_top', 8), ('gtab', 264 * 8),
             ('kf_owner', ND * 4), ('heavy', (T + 4) * 4)] + [('hv%d' % q, T * 4) for q in range(5)] + \
            [('hv_pend', 2 * T * 4), ('hv_delta', T * 8), ('hv_f', 256 * T * 8), ('hv_mvbase', (T + 1) * 8), ('hv_r1base', (T + 1) * 8),
             ('hv_work', 64), ('big', 2 * (1 + 4096) * 4), ('isbig', 2 * T * 4), ('pool', used * 8),
             ('f_last', T * 8), ('m_last', T * 4), ('tie_ctr', T * 4), ('seeds', N * 8), ('action', T * 4), ('security', T * 4),
             ('margins', T * 4), ('adjusted', N * 4), ('acc', T * n_prbs * 8), ('err', N * 4), ('stats', T * 32),
             ('d_state', N * nv * 4), ('d_prev', N * nv * 4), ('d_action', T * 4), ('d_labels', T * 4), ('d_hits', T * 4),
             ('d_out', 32), ('d_cursor', T * 4), ('d_cstar', T * 4), ('workb', S * 2 * 256 * capr * 8), ('offgrid', ND * 4),
             ('f32bad', ND * 4), ('F', 8), ('fstate', 4), ('fver', T * 4)]
    out, o = {}, 72
    for name, b in sizes:
        out[name] = blob[o:o + b]
        o += b
    assert int(out['pool_top'].view(np.uint64)[0]) == used
    v = dict(m=out['m'].view(np.int32), shell=out['shell'].view(np.uint64).reshape(ND, max_shells),
             head=out['head'].view(np.int32).reshape(ND, 256), pool=out['pool'].view(np.float64),
             offgrid=out['offgrid'].view(np.int32), m_last=out['m_last'].view(np.int32).reshape(N, S),
             fver=out['fver'].view(np.int32).reshape(N, S), kf_owner=out['kf_owner'].view(np.int32),
             cursor=out['d_cursor'].view(np.int32), cstar=out['d_cstar'].view(np.int32))
    assert (v['m'] == sh.dictionary_sizes()).all()
    return v


def _page(v, s, b):
    at = int(v['shell'][s, b])
    assert at >= 64
    return v['pool'][at:at + VEC].reshape(30, 64)


def _tile(v, s, bi, bj):
    """tile (bi, bj) of the full storage: the lower tiles of shell bi, then its upper tiles (0, bi) .. (bi - 1, bi)"""
    at = int(v['shell'][s, bi]) + VEC + bj * TILE if bj <= bi else int(v['shell'][s, bj]) + VEC + (bj + 1 + bi) * TILE
    return v['pool'][at:at + TILE].reshape(64, 64)


def _structure_check(v, s, old_m, eMBB):
    """chains, heads and the off-grid count rebuilt; every vacated slot, row and column of Kinv -- in the tiles of both sides of
    the diagonal -- exact zeros, K_f and d* included (D0 / E are scratch of the state being processed: DESIGN.md §8d)"""
    m = int(v['m'][s])
    nbm, nbo = (m + 63) // 64, (old_m + 63) // 64
    idx = np.concatenate([_page(v, s, b)[21].view(np.int32)[:64] for b in range(nbm)])[:m]
    link = np.concatenate([_page(v, s, b)[21].view(np.int32)[64:] for b in range(nbm)])[:m]
    head, want_link = pm.chains(idx)
    assert (v['head'][s] == head).all() and (link == want_link).all()
    assert v['offgrid'][s] == (idx < 0).sum()
    for j in range(m, old_m):
        b, l = j >> 6, j & 63
        P = _page(v, s, b)
        rows = (list(range(11)) if eMBB else list(range(16))) + [16, 19, 20]
        assert not P[rows, l].any(), j
        if eMBB:
            assert not P[11:16].view(np.float32).reshape(10, 64)[:, l].any(), j
        assert not P[21].view(np.int32)[[l, 64 + l]].any(), j
        for o in range(nbo):
            # up to its own block the whole row / column of the tile; beyond it the entries that ever were Kinv's (what lies at
            # or beyond old_m in the last block was never written by this dictionary: to_shared copied it as it found it)
            n = 64 if o <= b else min(64, old_m - 64 * o)
            assert not _tile(v, s, b, o)[l, :n].any(), (j, 'row', o)
            assert not _tile(v, s, o, b)[:n, l].any(), (j, 'column', o)


# ------------------------------------------------------------------ (a) bits against kb_prune
def test_every_removal_equals_kb_prune_on_the_unshared_copy():
    """X holds dictionaries of (200, 131) landmarks, A = X.to_agents([0]).  One removal per call down a ladder of targets from 199
    to 70 (across the block boundaries at 192 and 128; 70 is no multiple of 64), then one call to 64: after every call
    X.shrink(t) and A.prune(t) removed the same count, X.to_agents([0]) equals A bit for bit, X's own full Kinv equals A's and its
    own transpose (the upper tiles), pruned() are the counts and the pool's bytes have not moved.  The removals met the victim
    in the last slot and a victim in block 0 while the last slot lies in block 2.  A second handle does the whole ladder in one
    shrink and holds the same bytes; what was vacated reads zeros in both."""
    ag = _grown((200, 131), 256)
    X = ag.to_shared(0, 3)
    A = X.to_agents([0])
    sizes0 = X.dictionary_sizes().copy()
    assert list(sizes0) == [200, 131]
    used = X.pool()['used_bytes']
    _same_dictionaries(_dictionaries(X), _dictionaries(A), 'start')
    want = np.zeros(2, dtype=np.int64)
    prev = [d['landmarks'] for d in _dictionaries(X)]
    seen = set()
    for t in list(range(199, 69, -1)) + [64]:
        before = X.dictionary_sizes().astype(np.int64)
        over = np.maximum(before - t, 0)
        rx, ra = X.shrink(t), A.prune(t)
        assert rx == ra == over.sum(), t
        want += over
        B = X.to_agents([0])
        dx, da, db = _dictionaries(X), _dictionaries(A), _dictionaries(B)
        B.close()
        _same_dictionaries(db, da, ('unshared copy', t))
        _same_dictionaries(dx, da, ('full storage', t))
        for s in range(2):
            assert dx[s]['m'] == min(sizes0[s], t)
            assert _bits(dx[s]['kinv']) == _bits(dx[s]['kinv'].T), (t, s)
            if over[s] == 1:
                r, last = _victim(prev[s], dx[s]['landmarks']), int(before[s]) - 1
                if r == last:
                    seen.add('last')
                if r < 64 and last >= 128:
                    seen.add('block 0, last in block 2')
            prev[s] = dx[s]['landmarks']
        assert (X.pruned() == want).all() and (A.pruned()[0] == want).all()
        assert X.pool()['used_bytes'] == used
    assert seen == {'last', 'block 0, last in block 2'}, seen
    assert list(X.dictionary_sizes()) == [64, 64]
    v = _views(X, X.save_state())
    for s in range(2):
        _structure_check(v, s, int(sizes0[s]), eMBB=s == 0)
    assert (v['m_last'] == -1).all() and (v['fver'] == -1).all() and (v['kf_owner'] == -1).all()
    once = ag.to_shared(0, 3)
    assert once.shrink(64) == want.sum() and (once.pruned() == want).all()
    _same_dictionaries(_dictionaries(once), _dictionaries(X), 'one call')
    v1 = _views(once, once.save_state())
    for s in range(2):
        _structure_check(v1, s, int(sizes0[s]), eMBB=s == 0)
        for b in range(4):     # every page and every tile of both triangles: the same bytes, however the ladder was cut
            if v['shell'][s, b]:
                pick = list(range(17)) + [19, 20, 21]
                assert _bits(_page(v, s, b)[pick]) == _bits(_page(v1, s, b)[pick]), (s, b)
                for o in range(b + 1):
                    assert _bits(_tile(v, s, b, o)) == _bits(_tile(v1, s, b, o)) and _bits(_tile(v, s, o, b)) == _bits(_tile(v1, s, o, b))
    assert once.pool()['used_bytes'] == used
    for h in (once, A, X):
        h.close()


# ------------------------------------------------------------------ (b) nothing stale
def _control_batch(rng, n):
    state = np.concatenate([rng.random((n, 10)), rng.random((n, 3)) * 4.0], axis=1).astype(np.float32)
    action = rng.integers(5, 120, size=(n, 2)).astype(np.int32)
    labels = rng.choice([-1, 1], size=(n, 2)).astype(np.int32)
    return state, action, labels


def _with_one_off_grid_landmark():
    """dictionaries of (264, 300) landmarks; the second then takes ONE landmark off the candidate grid through kb_update, far from
    every other landmark, and a second kb_update of the same point with the other label projects onto it alone and takes its
    coefficient to zero: the smallest key there is, so it is the first victim of a prune"""
    key = 'off grid'
    if key in _grown_cache:
        return _grown_cache[key]
    from ranslice.kbrl_dev import VecKBRL
    src = _grown((264, 300), 512)
    ag = VecKBRL(1, DIMS, N_PRBS, capacity=512, pool_bytes=64 << 20)
    ag.fork_from(src, [0])
    x = np.array([40.0, 40.0, 40.0, 0.5 + 0.0012345])
    yp, f = ag.predict(0, 1, x)
    assert f == 0.0                                  # (every kernel value underflows: the landmark stands alone)
    assert ag.update(0, 1, x, 1)[0] == 2
    yp, f = ag.predict(0, 1, x)
    assert f == 1.0 and ag.update(0, 1, x, -1)[0] == 1
    L = ag.learner(0, 1)
    assert L['m'] == 301 and abs(L['coeff'][300]) < 1e-12 and (L['landmarks'][300] == x).all()
    _grown_cache[key] = ag
    return ag


def _off_grid(L):
    """landmarks whose last coordinate is no a / n_prbs (the device's own test: kb_kbrl.hip, grid_index)"""
    t = L['landmarks'][:, -1]
    return int((np.rint(t * N_PRBS) / N_PRBS != t).sum())


def _compare(X, Tw, what):
    assert (X.dictionary_sizes() == Tw.dictionary_sizes()).all(), what
    cx, ct = X.control(), Tw.control()
    for q in ('margins', 'security_factors', 'action', 'adjusted', 'accuracies'):
        assert _bits(cx[q]) == _bits(ct[q]), (what, q)
    _same_dictionaries(_dictionaries(X), _dictionaries(Tw), what)


def test_nothing_stale_through_the_host_entry_points():
    """Eight replicas: three update_control + select_action steps, shrink, three more -- twice.  The first shrink removes one
    landmark, the only off-grid one of the second dictionary (which is then scored on the wide path again); the second takes
    both dictionaries from KB_GEMM_M landmarks or more to below.  After each, every step (hits, actions, adjusted, margins,
    sizes, dictionaries) equals, bit for bit, that of a twin that loaded the save_state blob taken right after the shrink."""
    ag = _with_one_off_grid_landmark()
    X, Tw = ag.to_shared(0, 8, max_rounds=1), ag.to_shared(0, 8, max_rounds=1)   # (one round: at most 8 insertions per slice and step)
    rng = np.random.default_rng(17)

    def steps(both, what):
        for i in range(3):
            st, ac, lb = _control_batch(rng, 8)
            nxt = _control_batch(rng, 8)[0]
            outs = []
            for h in ([X, Tw] if both else [X]):
                hits = h.update_control(st, ac, lb)
                a, j = h.select_action(nxt)
                outs.append((hits, a, j))
            if both:
                for p, q in zip(*outs):
                    assert _bits(p) == _bits(q), (what, i)
                _compare(X, Tw, (what, i))

    steps(False, 'before')
    sizes = X.dictionary_sizes()
    assert sizes[0] >= KB_GEMM_M and sizes[0] <= sizes[1] - 1 and _off_grid(X.learner(0, 1)) == 1
    assert X.shrink(int(sizes[1]) - 1) == 1 and list(X.pruned()) == [0, 1]
    assert _off_grid(X.learner(0, 1)) == 0 and X.dictionary_sizes()[1] >= KB_GEMM_M
    v = _views(X, X.save_state())
    assert v['offgrid'][1] == 0 and (v['cursor'] == -1).all() and (v['cstar'] == -1).all()
    assert (v['m_last'][:, 1] == -1).all() and (v['fver'][:, 1] == -1).all() and v['kf_owner'][1] == -1
    Tw.load_state(X.save_state())
    steps(True, 'after the off-grid landmark left')
    sizes = X.dictionary_sizes()
    assert sizes.min() >= KB_GEMM_M
    assert X.shrink(200) == sizes.sum() - 400 and list(X.dictionary_sizes()) == [200, 200]
    Tw.load_state(X.save_state())
    steps(True, 'below KB_GEMM_M')
    X.close()
    Tw.close()


def test_nothing_stale_in_the_resident_loop(golden_dir):
    """The same through step_resident on a small environment (one eMBB and one mMTC slice, 200 PRBs), the shrink called directly
    after a resident step -- whose select_action left the scores of the next step's first scan behind (gemm_fresh): the pruned
    handle must not reuse them.  Twin: an agent and an environment that loaded the two checkpoints taken right after the shrink."""
    from ranslice.vec_env import VecRanSlice
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    fading = [g['t0'], g['t1'], g['t2']]
    ag = _grown((264, 300), 512)
    N = 8
    X, Tw = ag.to_shared(0, N), ag.to_shared(0, N)
    envs = [VecRanSlice(n_envs=N, cfg=make_config(3, n_envs=N, n_prbs=N_PRBS), fading=fading, seed=5) for _ in range(2)]
    env, envT = envs
    env.reset()
    env.step(np.tile(np.array(IA, dtype=np.int32), (N, 1)))
    for _ in range(3):
        X.step_resident(env)
        env.step_resident()
    X.step_resident(env)
    sizes = X.dictionary_sizes()
    assert sizes.min() >= KB_GEMM_M
    assert X.shrink(200) == sizes.sum() - 400
    X.synchronize()
    env.synchronize()
    Tw.load_state(X.save_state())
    envT.load_state(env.save_state())
    for i in range(3):
        for h, e in ((X, env), (Tw, envT)):
            e.step_resident()
            h.step_resident(e)
            h.synchronize()
        _compare(X, Tw, ('resident', i))
    assert X.dictionary_sizes().max() <= 512
    for h in (X, Tw, env, envT):
        h.close()


# ------------------------------------------------------------------ (c) learning resumes
def test_learning_resumes_after_a_shrink():
    """capacity 128, both dictionaries filled: further steps insert nothing (kb_get_stats[2]); after shrink(96) the same inputs
    insert again, and no dictionary ever exceeds the capacity"""
    ag = _grown((128, 128), 128)
    X = ag.to_shared(0, 8)
    rng = np.random.default_rng(23)
    batches = [_control_batch(rng, 8) for _ in range(3)]
    grown0 = X.stats()[2]
    for st, ac, lb in batches:
        X.update_control(st, ac, lb)
        assert list(X.dictionary_sizes()) == [128, 128]
    assert X.stats()[2] == grown0
    used = X.pool()['used_bytes']
    assert X.shrink(96) == 64 and list(X.dictionary_sizes()) == [96, 96]
    for st, ac, lb in batches:
        X.update_control(st, ac, lb)
        assert X.dictionary_sizes().max() <= 128
    added = X.stats()[2] - grown0
    sizes = X.dictionary_sizes()
    print('insertions after the shrink: %d, sizes %s' % (added, list(sizes)))
    assert added > 0 and sizes.sum() == 192 + added and sizes.max() > 96
    assert X.pool()['used_bytes'] == used             # (grown back into the shells that were kept)
    X.close()


# ------------------------------------------------------------------ (d) shards stay identical
def test_shards_hold_the_same_bytes_through_a_shrink():
    """W = 2 handles of 4 replicas exchanging their proposals by hand beside one handle of 8: steps, shrink on all three (no
    collective, nothing exchanged), more steps -- the three hold the same dictionary bytes throughout"""
    from ranslice.kbrl_dev import PROP_W, merge_proposals
    ag = _grown((200, 131), 256)
    N, W, n, S, budget, rounds = 8, 2, 4, 2, 16, 3
    whole = ag.to_shared(0, N, budget=budget, max_rounds=rounds)
    parts = [ag.to_shared(0, n, budget=budget, max_rounds=rounds, first_env=w * n) for w in range(W)]

    def parts_update(state, action, labels):
        hits = [np.zeros((n, S), dtype=np.int32) for _ in range(W)]
        for rnd in range(rounds):
            cs, ps = [], []
            for w, p in enumerate(parts):
                st = np.ascontiguousarray(state[w * n:(w + 1) * n], dtype=np.float32)
                ac = np.ascontiguousarray(action[w * n:(w + 1) * n], dtype=np.int32)
                lb = np.ascontiguousarray(labels[w * n:(w + 1) * n], dtype=np.int32)
                counts = np.zeros(S, dtype=np.int32)
                props = np.zeros((S, budget, PROP_W))
                p._check(p.L.kb_shared_scan(p.h, st.ctypes.data_as(_fp) if rnd == 0 else None,
                                            ac.ctypes.data_as(_ip) if rnd == 0 else None,
                                            lb.ctypes.data_as(_ip) if rnd == 0 else None, rnd, budget,
                                            hits[w].ctypes.data_as(_ip), counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp)))
                cs.append(counts)
                ps.append(props)
            if int(np.sum(cs)) == 0:
                break
            mc, mp, taken = merge_proposals(np.stack(cs), np.stack(ps), budget)
            mc, mp = np.ascontiguousarray(mc, dtype=np.int32), np.ascontiguousarray(mp)
            for w, p in enumerate(parts):
                p._check(p.L.kb_shared_apply(p.h, mc.ctypes.data_as(_ip), mp.ctypes.data_as(_dp), budget))
                acc = np.ascontiguousarray(taken[w], dtype=np.int32)
                p._check(p.L.kb_shared_commit(p.h, acc.ctypes.data_as(_ip)))
        return np.concatenate(hits)

    def same(what):
        dw = _dictionaries(whole)
        for p in parts:
            _same_dictionaries(_dictionaries(p), dw, what)

    rng = np.random.default_rng(29)

    def steps(what):
        for i in range(3):
            st, ac, lb = _control_batch(rng, N)
            hw = whole.update_control(st, ac, lb)
            assert (hw == parts_update(st, ac, lb)).all(), (what, i)
            nxt = _control_batch(rng, N)[0]
            aw = whole.select_action(nxt)[0]
            ap = np.concatenate([p.select_action(nxt[w * n:(w + 1) * n])[0] for w, p in enumerate(parts)])
            assert (aw == ap).all(), (what, i)
            same((what, i))

    steps('before')
    sizes = whole.dictionary_sizes()
    assert sizes.min() > 100
    removed = [h.shrink(100) for h in [whole] + parts]
    assert removed == [sizes.sum() - 200] * 3
    same('shrunk')
    steps('after')
    for h in [whole] + parts:
        h.close()


# ------------------------------------------------------------------ (e) refusals
def test_refusals():
    """each refusal returns its code with a message that names kb_shared_prune and leaves the handle usable"""
    from ranslice.kbrl_dev import PROP_W, SharedVecKBRL, VecKBRL
    ag = _grown((200, 131), 256)
    X = ag.to_shared(0, 4, budget=16)

    def refused(obj, target, code, call=None):
        with pytest.raises(_lib.RanSliceError) as ei:
            (call or SharedVecKBRL.shrink)(obj, target)
        assert ei.value.code == code and 'kb_shared_prune' in str(ei.value)

    refused(X, 63, _lib.RS_EINVAL)
    refused(X, 257, _lib.RS_EINVAL)
    assert list(X.dictionary_sizes()) == [200, 131]
    refused(ag, 64, _lib.RS_ESTATE)                            # one agent per replica
    assert ag.prune(256) == 0
    with pytest.raises(_lib.RanSliceError) as ei:              # and the per-replica call keeps refusing the shared handle
        X.prune(64)
    assert ei.value.code == _lib.RS_ESTATE and 'kb_prune' in str(ei.value)
    fresh = SharedVecKBRL(4, DIMS, N_PRBS, capacity=256)       # never reset
    refused(fresh, 64, _lib.RS_ESTATE)
    fresh.close()
    # between kb_shared_scan and kb_shared_commit: a scan that found proposals leaves the round open
    rng = np.random.default_rng(31)
    st, ac, lb = _control_batch(rng, 4)
    hits, counts, props = np.zeros((4, 2), dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros((2, 16, PROP_W))
    X._check(X.L.kb_shared_scan(X.h, st.ctypes.data_as(_fp), ac.ctypes.data_as(_ip), lb.ctypes.data_as(_ip), 0, 16,
                                hits.ctypes.data_as(_ip), counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp)))
    assert counts.sum() > 0
    refused(X, 100, _lib.RS_ESTATE)
    assert list(X.dictionary_sizes()) == [200, 131]
    X._check(X.L.kb_shared_apply(X.h, counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp), 16))
    refused(X, 100, _lib.RS_ESTATE)
    X._check(X.L.kb_shared_commit(X.h, counts.ctypes.data_as(_ip)))
    sizes = X.dictionary_sizes().copy()
    # a diagonal entry of Kinv that is not finite and positive: that dictionary is left untouched, the other is pruned
    clean = X.save_state()
    blob = clean.copy()
    v = _views(X, blob)
    v['pool'][int(v['shell'][0, 0]) + VEC + 5 * 64 + 5] = -1.0          # Kinv[5][5] of dictionary 0
    X.load_state(blob)
    before = X.learner(0, 0, with_kinv=True)
    refused(X, 100, _lib.RS_ESTATE)
    after = X.learner(0, 0, with_kinv=True)
    assert after['m'] == sizes[0] and all(_bits(before[q]) == _bits(after[q]) for q in ('landmarks', 'coeff', 'kinv'))
    assert list(X.dictionary_sizes()) == [sizes[0], 100] and list(X.pruned()) == [0, sizes[1] - 100]
    assert X.shrink(256) == 0                                  # nothing above the target: nothing to do, no error
    X.load_state(clean)                                        # (the sound Kinv again)
    assert X.shrink(100) == sizes.sum() - 200
    X.update_control(*_control_batch(rng, 4))
    X.select_action(st)
    X.close()
