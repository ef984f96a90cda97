"""kb_prune on the device against its float64 mirror (tests/prune_mirror.py) and against itself.

Tolerances are the project's: 1e-8 relative for coefficients, Kinv and f in dictionaries of hundreds of
landmarks -- the sizes used here -- each measured against its array's scale (the largest entry).
Decisions (the victim of every removal, predicted signs, update branches, sizes) are exact, and the streams are chosen so that
none of them lies near its threshold: that is asserted, not assumed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_mirror as pm   # noqa: E402
from ranslice import _lib   # noqa: E402
from ranslice.config import make_config   # noqa: E402

pytestmark = pytest.mark.gpu

KINV_RTOL = 1e-8
COEFF_RTOL = 1e-8
F_RTOL, F_ATOL = 1e-8, 1e-9   # f of kb_predict, as tests/test_gpu_kbrl.py holds it
GAP = 1e-6        # relative distance between the winner's key and the runner-up's at every removal
F_MARGIN = 1e-7   # |f| of every prediction whose sign is compared
D_MARGIN = 1e-7   # |delta - eta| of every update whose branch is compared
ETA = 0.1


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _g14(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g14_projectron_long.npz'))
    return g['x'], g['y'].astype(int)


def _compare_dictionary(ag, e, s, mr, what):
    L = ag.learner(e, s, with_kinv=True)
    assert L['m'] == mr.m, what
    np.testing.assert_array_equal(L['landmarks'], mr.L, err_msg=str(what))      # which slot every survivor occupies
    scale = np.abs(mr.P).max()
    dist = np.abs(L['kinv'] - mr.P).max() / scale
    cdist = np.abs(L['coeff'] - mr.c).max() / np.abs(mr.c).max()
    print('%s: m %d, |Kinv - mirror| / scale %.3e, |coeff - mirror| / scale %.3e' % (what, mr.m, dist, cdist))
    assert cdist <= COEFF_RTOL, what
    assert dist <= KINV_RTOL, what
    assert np.array_equal(L['kinv'], L['kinv'].T), what
    return L


def _feed(ag, mirrors, e, x, y, exact, what):
    """one sample through kb_predict / kb_update into dictionary (e, 0) and into its mirror; exact: signs and branches are
    compared and the mirror's margins asserted"""
    mr = mirrors[e]
    yp, f = ag.predict(e, 0, x)
    fm = mr.predict(x)
    br, dl = ag.update(e, 0, x, int(y))
    brm, dlm = mr.update(x, int(y))
    if exact:
        if mr.m > 1 or brm == 0:
            assert abs(fm) > F_MARGIN, (what, fm)
            assert yp == (1 if fm > 0 else -1), what
        assert f == pytest.approx(fm, rel=F_RTOL, abs=F_ATOL), what
        if brm:
            assert abs(dlm - ETA) > D_MARGIN, (what, dlm)
        assert br == brm, (what, dl, dlm)
    else:
        assert br == brm, (what, dl, dlm)


def test_teacher_forced_parity(golden_dir):
    """The G14 stream into three dictionaries (all of it; its even samples; its odd samples), pruned at two points to targets that
    are not multiples of 64 -- the first prune one removal per call, so that every victim is compared, the second in one call --
    and continued: at every prune the removal sequence, the sizes and the slot of every survivor are exact, coefficients and
    all of Kinv within tolerance; afterwards every predicted sign, update branch and size is exact to the end of the stream."""
    from ranslice.kbrl_dev import VecKBRL
    xs, ys = _g14(golden_dir)
    ag = VecKBRL(3, [10], 200, capacity=4096)
    ag.reset([[10]] * 3, [[3]] * 3)
    mirrors = [pm.Mirror(11, eta=ETA) for _ in range(3)]
    n = 5200
    prunes = {2600: (150, 'stepwise'), 4200: (201, 'one call')}
    pruned_once = False
    want_pruned = np.zeros((3, 1), dtype=np.int64)
    for i in range(n):
        for e in (0, 1 + i % 2):
            _feed(ag, mirrors, e, xs[i], ys[i], pruned_once, (i, e))
        if i % 400 == 0:
            assert list(ag.dictionary_sizes()[:, 0]) == [m.m for m in mirrors], i
        if i in prunes:
            target, how = prunes[i]
            before = [m.m for m in mirrors]
            assert max(before) > target and target % 64
            if how == 'stepwise':
                for t in range(max(before) - 1, target - 1, -1):
                    removed = ag.prune(t) if t >= 64 else 0
                    logs = [m.prune(t) for m in mirrors]
                    assert removed == sum(len(lg) for lg in logs) and all(len(lg) <= 1 for lg in logs)
                    for e, lg in enumerate(logs):
                        for step in lg:
                            assert step['gap'] >= GAP, (i, e, step['gap'])
                        if lg:   # the victim and the slot of every survivor
                            np.testing.assert_array_equal(ag.learner(e, 0)['landmarks'], mirrors[e].L, err_msg=str((i, e, t)))
            else:
                removed = ag.prune(target)
                logs = [m.prune(target) for m in mirrors]
                assert removed == sum(len(lg) for lg in logs)
                assert all(step['gap'] >= GAP for lg in logs for step in lg)
            for e in range(3):
                want_pruned[e, 0] += max(before[e] - target, 0)
                assert mirrors[e].m == min(before[e], target)
                _compare_dictionary(ag, e, 0, mirrors[e], (i, e, how))
            assert (ag.pruned() == want_pruned).all()
            pruned_once = True
    assert list(ag.dictionary_sizes()[:, 0]) == [m.m for m in mirrors]
    for e in range(3):
        _compare_dictionary(ag, e, 0, mirrors[e], ('end', e))
    ag.close()


# ---- the checkpoint blob as a window on the device state: kb_state_header, then the handle's arrays in allocation order
def _blob_views(ag, blob):
    N, S, nv, n_prbs = ag.n_envs, ag.S, ag.nv, ag.n_prbs
    T = ND = N * S
    max_shells = (ag.capacity + 63) // 64
    used = int(np.frombuffer(blob[24:32].tobytes(), dtype=np.uint64)[0])    # kb_state_header.pool_doubles_used
    sizes = [('m', ND * 4), ('shell', ND * max_shells * 8), ('head', ND * 256 * 4), ('pool_top', 8), ('gtab', 264 * 8),
             ('kf_owner', ND * 4), ('heavy', (T + 4) * 4)] + [('hv%d' % q, T * 4) for q in range(5)] + \
            [('hv_pend', 2 * T * 4), ('hv_delta', T * 8), ('hv_f', 256 * T * 8), ('hv_mvbase', (T + 1) * 8), ('hv_r1base', (T + 1) * 8),
             ('hv_work', 64), ('big', 2 * (1 + 4096) * 4), ('isbig', 2 * T * 4), ('pool', used * 8),
             ('f_last', T * 8), ('m_last', T * 4), ('tie_ctr', T * 4), ('seeds', N * 8), ('action', T * 4), ('security', T * 4),
             ('margins', T * 4), ('adjusted', N * 4), ('acc', T * n_prbs * 8), ('err', N * 4), ('stats', T * 32),
             ('d_state', N * nv * 4), ('d_prev', N * nv * 4), ('d_action', T * 4), ('d_labels', T * 4), ('d_hits', T * 4),
             ('d_out', 32), ('d_cursor', T * 4), ('d_cstar', T * 4), ('workb', 8), ('offgrid', ND * 4), ('f32bad', ND * 4)]
    out, o = {}, 72
    for name, b in sizes:
        out[name] = blob[o:o + b]
        o += b
    assert int(out['pool_top'].view(np.uint64)[0]) == used
    v = dict(m=out['m'].view(np.int32), shell=out['shell'].view(np.uint64).reshape(ND, max_shells),
             head=out['head'].view(np.int32).reshape(ND, 256), pool=out['pool'].view(np.float64),
             offgrid=out['offgrid'].view(np.int32), f32bad=out['f32bad'].view(np.int32), m_last=out['m_last'].view(np.int32),
             kf_owner=out['kf_owner'].view(np.int32))
    assert (v['m'] == ag.dictionary_sizes().reshape(-1)).all()
    return v


VEC, TILE = 30 * 64, 4096


def _page(v, dict_, b):
    at = int(v['shell'][dict_, b])
    assert at >= 64
    return v['pool'][at:at + VEC].reshape(30, 64)


def _tile(v, dict_, bi, bj):
    at = int(v['shell'][dict_, bi]) + VEC + bj * TILE
    return v['pool'][at:at + TILE].reshape(64, 64)


def _structure_check(ag, v, dict_, old_m, eMBB):
    m = int(v['m'][dict_])
    idx = np.concatenate([_page(v, dict_, b)[21].view(np.int32)[:64] for b in range((m + 63) // 64)])[:m]
    link = np.concatenate([_page(v, dict_, b)[21].view(np.int32)[64:] for b in range((m + 63) // 64)])[:m]
    head, want_link = pm.chains(idx)
    assert (v['head'][dict_] == head).all() and (link == want_link).all()
    for a in np.nonzero(head >= 0)[0]:          # the invariant itself: head = the largest slot, links strictly decrease
        j, seen = head[a], []
        while j >= 0:
            seen.append(j)
            assert idx[j] == a and link[j] < j
            j = link[j]
        assert seen == sorted(np.nonzero(idx == a)[0], reverse=True)
    assert v['offgrid'][dict_] == (idx < 0).sum()
    # vacated slots and Kinv rows / columns: exact zeros
    for j in range(m, old_m):
        b, l = j >> 6, j & 63
        P = _page(v, dict_, b)
        # the landmark's own rows: coordinates (and the float32 copy below), coefficient, K_f, d*, grid index and link.  Rows 17
        # and 18 (D0, E) are scratch of the state being processed: the binning pass of select_action writes them for all 64
        # lanes of a chunk, so a slot vacated by an earlier prune may hold them again -- they are nobody's state
        rows = (list(range(11)) if eMBB else list(range(16))) + [16, 19, 20]
        assert not P[rows, l].any(), j
        if eMBB:
            assert not P[11:16].view(np.float32).reshape(10, 64)[:, l].any(), j
        assert not P[21].view(np.int32)[[l, 64 + l]].any(), j
        for bj in range(b + 1):
            assert not _tile(v, dict_, b, bj)[l].any(), (j, bj)
        assert not _tile(v, dict_, b, b)[:, l].any(), j
        for bi in range(b + 1, (old_m + 63) // 64):
            assert not _tile(v, dict_, bi, b)[:, l].any(), (j, bi)


def _random_stream(rng, d, n, offgrid_every=0, notf32_every=0, spread=1.0):
    xs = (rng.random((n, d)) * spread).astype(np.float32).astype(np.float64)
    xs[:, d - 1] = rng.integers(0, 201, size=n) / 200.0
    if offgrid_every:
        xs[::offgrid_every, d - 1] += 0.0012345
    if notf32_every:
        xs[::notf32_every, 0] += 1e-9
    return xs, rng.choice([-1, 1], size=n)


@pytest.fixture(scope='module')
def grown():
    """two agents x (an eMBB learner of 10 state variables, an mMTC learner of 3) fed random streams: dictionaries of about
    411 / 204 / 103 / a few dozen landmarks, with off-grid landmarks and (agent 0) coordinates that are not float32 values"""
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(2, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
    ag.reset([[10, 5]] * 2, [[3, 2]] * 2)
    rng = np.random.default_rng(5)
    mirrors = {}
    for (e, s, d, n, og, nf) in ((0, 0, 11, 900, 17, 40), (0, 1, 4, 2500, 13, 0), (1, 0, 11, 200, 0, 0), (1, 1, 4, 120, 0, 0)):
        xs, ys = _random_stream(rng, d, n, og, nf, spread=3.0 if d == 4 else 1.0)   # (three state variables: spread out, or ~25 landmarks span them)
        mr = pm.Mirror(d, eta=ETA)
        for i in range(n):
            ag.predict(e, s, xs[i])
            mr.predict(xs[i])
            br, _ = ag.update(e, s, xs[i], int(ys[i]))
            assert br == mr.update(xs[i], int(ys[i]))[0], (e, s, i)
        mirrors[(e, s)] = mr
    yield ag, mirrors
    ag.close()


def test_structure_memory_and_counters(grown):
    """After a prune to 330 and again after one to 100: select_action of the pruned handle equals, bit for bit, that of a handle
    loaded from its checkpoint -- at 330 one pruned dictionary holds more than 319 landmarks (the launch for large dictionaries),
    at 100 all are below (the other one).  After the second prune: chains, off-grid counts, zeros in what was vacated, the
    float32 mark kept; the pool's used bytes do not move, neither by the prune nor by growing back; counters; kb_state_bytes."""
    from ranslice.kbrl_dev import VecKBRL
    ag, mirrors = grown
    L = ag.L
    import ctypes as C
    nbytes0 = C.c_uint64()
    assert L.kb_state_bytes(ag.h, C.byref(nbytes0)) == 0
    sizes0 = ag.dictionary_sizes().copy()
    assert sizes0[0, 0] > 319 and 100 < sizes0[0, 1] < 319 and sizes0.min() < 100 < sizes0[1, 0], sizes0
    used0 = ag.pool()['used_bytes']
    v0 = _blob_views(ag, ag.save_state())
    assert v0['f32bad'][0] == 1 and v0['offgrid'][0] > 0 and v0['offgrid'][1] > 0
    assert not ag.pruned().any()
    # the big dictionary in two calls (above and below the 320-landmark launch order), everything else in the second
    rem1 = ag.prune(330)
    assert rem1 == sizes0[0, 0] - 330
    other = VecKBRL(2, [10, 3], 200, capacity=1024, pool_bytes=256 << 20)
    other.reset([[10, 5]] * 2, [[3, 2]] * 2)

    def same_select(seed):
        """the pruned handle and a handle that loaded its checkpoint"""
        blob = ag.save_state()
        other.load_state(blob)
        assert not other.pruned().any() and (other.dictionary_sizes() == ag.dictionary_sizes()).all()
        rng = np.random.default_rng(seed)
        for _ in range(6):
            st = rng.random((2, 13)).astype(np.float32)
            a1, j1 = ag.select_action(st)
            a2, j2 = other.select_action(st)
            assert _bits(a1) == _bits(a2) and _bits(j1) == _bits(j2)
        return blob

    assert ag.dictionary_sizes()[0, 0] == 330 > 319 > ag.dictionary_sizes()[0, 1]
    same_select(7)
    rem2 = ag.prune(100)
    want = np.maximum(sizes0 - 100, 0)
    assert rem1 + rem2 == want.sum() and (ag.pruned() == want).all()
    assert (ag.dictionary_sizes() == np.minimum(sizes0, 100)).all()
    assert ag.pool()['used_bytes'] == used0
    nbytes1 = C.c_uint64()
    assert L.kb_state_bytes(ag.h, C.byref(nbytes1)) == 0 and nbytes1.value == nbytes0.value
    blob = ag.save_state()
    assert blob.size == nbytes0.value
    v = _blob_views(ag, blob)
    for dict_ in range(4):
        _structure_check(ag, v, dict_, int(sizes0.reshape(-1)[dict_]), eMBB=dict_ % 2 == 0)
    assert v['f32bad'][0] == 1 and (v['shell'] == v0['shell']).all()
    touched = want.reshape(-1) > 0
    assert (v['m_last'][touched] == -1).all() and (v['kf_owner'][touched] == -1).all()
    assert v['m_last'][~touched].tolist() == v0['m_last'][~touched].tolist()
    # against the mirror (the mMTC dictionary takes the path without the float32 copy)
    for key, mr in mirrors.items():
        mr.prune(330)
        log = mr.prune(100)
        assert all(step['gap'] >= GAP for step in log), key
        _compare_dictionary(ag, key[0], key[1], mr, key)
    # a stale predict cache: kb_update without a new kb_predict
    x = np.full(11, 0.3)
    with pytest.raises(_lib.RanSliceError) as ei:
        ag.update(0, 0, x, 1)
    assert ei.value.code == _lib.RS_ESTATE
    assert ag.dictionary_sizes().max() == 100
    same_select(9)
    other.close()
    # growing back: the shells are still there
    rng = np.random.default_rng(11)
    xs, ys = _random_stream(rng, 11, 4000)
    i = 0
    while ag.dictionary_sizes()[0, 0] < sizes0[0, 0] and i < len(xs):
        for _ in range(50):
            ag.predict(0, 0, xs[i])
            ag.update(0, 0, xs[i], int(ys[i]))
            i += 1
    assert ag.dictionary_sizes()[0, 0] >= sizes0[0, 0]
    if ag.dictionary_sizes()[0, 0] <= ((sizes0[0, 0] + 63) // 64) * 64:
        assert ag.pool()['used_bytes'] == used0
    Lr = ag.learner(0, 0, with_kinv=True)
    assert np.array_equal(Lr['kinv'], Lr['kinv'].T) and np.isfinite(Lr['kinv']).all()
    assert ag.pool()['pool_full'] == 0
    # reset: counters at zero
    ag.reset([[10, 5]] * 2, [[3, 2]] * 2)
    assert not ag.pruned().any()


def test_regrowth_reuses_the_shells():
    """grow to 200, prune to 70, grow back to exactly the old size: used bytes are identical at the three points"""
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(1, [10], 200, capacity=1024, pool_bytes=64 << 20)
    ag.reset([[10]], [[3]])
    rng = np.random.default_rng(21)
    xs, ys = _random_stream(rng, 11, 3000)
    i = 0
    while ag.dictionary_sizes()[0, 0] < 200:
        ag.predict(0, 0, xs[i])
        ag.update(0, 0, xs[i], int(ys[i]))
        i += 1
    used = ag.pool()['used_bytes']
    assert ag.prune(70) == 130 and ag.pool()['used_bytes'] == used
    while ag.dictionary_sizes()[0, 0] < 200:
        ag.predict(0, 0, xs[i])
        ag.update(0, 0, xs[i], int(ys[i]))
        i += 1
    assert ag.dictionary_sizes()[0, 0] == 200 and ag.pool()['used_bytes'] == used
    assert ag.pruned()[0, 0] == 130
    ag.close()


def test_refusals():
    """each refusal returns its code with a message and leaves the handle usable"""
    from ranslice.kbrl_dev import VecKBRL, SharedVecKBRL
    ag = VecKBRL(2, [10], 200, capacity=512, pool_bytes=64 << 20)
    ag.reset([[10]] * 2, [[3]] * 2)
    rng = np.random.default_rng(3)
    xs, ys = _random_stream(rng, 11, 500)
    for e in range(2):
        for i in range(500):
            ag.predict(e, 0, xs[i])
            ag.update(e, 0, xs[i], int(ys[i]))
    sizes = ag.dictionary_sizes().copy()
    assert sizes.min() > 80

    def refused(obj, target, code):
        with pytest.raises(_lib.RanSliceError) as ei:
            obj.prune(target)
        assert ei.value.code == code and 'kb_prune' in str(ei.value)

    refused(ag, 63, _lib.RS_EINVAL)
    refused(ag, 513, _lib.RS_EINVAL)
    assert (ag.dictionary_sizes() == sizes).all()
    dep = ag.deploy([0, 1])
    refused(dep, 64, _lib.RS_ESTATE)
    assert dep.select_action(np.zeros((2, 10), dtype=np.float32))[0].shape == (2, 1)
    dep.close()
    sh = SharedVecKBRL(2, [10], 200, capacity=512)
    sh.reset([[10]] * 2, [[3]] * 2)
    refused(sh, 64, _lib.RS_ESTATE)
    sh.close()
    # a diagonal entry of Kinv that is not finite and positive: that dictionary is left untouched, the other is pruned
    blob = ag.save_state()
    v = _blob_views(ag, blob)
    at = int(v['shell'][0, 0]) + VEC + 5 * 64 + 5          # Kinv[5][5] of dictionary 0
    v['pool'][at] = -1.0
    ag.load_state(blob)
    before = ag.learner(0, 0, with_kinv=True)
    refused(ag, 70, _lib.RS_ESTATE)
    after = ag.learner(0, 0, with_kinv=True)
    assert after['m'] == sizes[0, 0] and all(_bits(before[q]) == _bits(after[q]) for q in ('landmarks', 'coeff', 'kinv'))
    assert ag.dictionary_sizes()[1, 0] == 70 and list(ag.pruned()[:, 0]) == [0, sizes[1, 0] - 70]
    assert ag.prune(512) == 0                                # nothing above the target: nothing to do, no error
    ag.predict(1, 0, xs[0])
    ag.update(1, 0, xs[0], 1)
    ag.close()


def test_independent_of_batching():
    """pruning four dictionaries in one call == pruning each in a call of its own (a one-agent fork each), bit for bit"""
    from ranslice.kbrl_dev import VecKBRL
    n = 4
    ag = VecKBRL(n, [10], 200, capacity=1024, pool_bytes=256 << 20)
    ag.reset([[10]] * n, [[3]] * n)
    rng = np.random.default_rng(8)
    for e, cnt in enumerate((300, 1300, 700, 120)):
        xs, ys = _random_stream(rng, 11, cnt, offgrid_every=29)
        for i in range(cnt):
            ag.predict(e, 0, xs[i])
            ag.update(e, 0, xs[i], int(ys[i]))
    sizes = ag.dictionary_sizes()[:, 0]
    assert (sizes > 97).sum() >= 3 and sizes.max() > 400
    alone = []
    for e in range(n):
        one = VecKBRL(1, [10], 200, capacity=1024, pool_bytes=64 << 20)
        one.fork_from(ag, [e])
        one.prune(97)
        alone.append(one.learner(0, 0, with_kinv=True))
        one.close()
    ag.prune(97)
    for e in range(n):
        got = ag.learner(e, 0, with_kinv=True)
        assert got['m'] == alone[e]['m'] == min(sizes[e], 97)
        for q in ('landmarks', 'coeff', 'kinv'):
            assert _bits(got[q]) == _bits(alone[e][q]), (e, q)
    ag.close()


def test_closed_loop_graph_equals_plain(golden_dir):
    """272 replicas of scenario 0, 600 steps in stretches of 100 with a prune to 128 between them: the captured graph and plain
    enqueueing give bit-equal histories; no flag other than 8 / 16.  No dictionary exceeds 128 plus what one stretch can add,
    and what a stretch added is taken from the agent's own count of insertions (kb_get_stats, [2]): after every stretch the
    landmarks held in all are those held after the last prune plus the insertions counted since, so no dictionary can hold
    more than 128 plus that count; a prune takes away exactly what it reports."""
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    fading = [g['t0'], g['t1'], g['t2']]
    cfg0 = make_config(0)
    dims, n_prbs = [10] * cfg0.n_embb + [3] * cfg0.n_mmtc, cfg0.n_prbs
    N, steps, stretch, target = 272, 600, 100, 128
    hist, final, pruned = [], [], []
    for graph in (True, False):
        env = VecRanSlice(n_envs=N, cfg=make_config(0, n_envs=N), fading=fading, seed=41)
        ag = VecKBRL(N, dims, n_prbs, capacity=1024, pool_bytes=2 << 30)
        ia = np.tile(np.array([10 if d == 10 else 5 for d in dims], dtype=np.int32), (N, 1))
        sf = np.tile(np.array([3 if d == 10 else 2 for d in dims], dtype=np.int32), (N, 1))
        env.reset()
        ag.reset(ia, sf, seeds=np.arange(N, dtype=np.uint64) + 5)
        env.step(ia)
        ag.history_begin(steps)
        held, grown = ag.dictionary_sizes().astype(np.int64), ag.stats()[2]
        for s0 in range(0, steps, stretch):
            ag.run_resident(env, stretch, graph=graph)
            ag.synchronize()
            sizes, now = ag.dictionary_sizes().astype(np.int64), ag.stats()[2]
            added = now - grown
            print('graph %d, steps %d..%d: %d insertions, largest dictionary %d, largest growth of one %d'
                  % (graph, s0, s0 + stretch, added, sizes.max(), (sizes - held).max()))
            assert (sizes >= held).all() and sizes.sum() == held.sum() + added
            assert sizes.max() <= (target if s0 else held.max()) + added
            # (and the bound that needs no counter: one landmark per candidate of the augmentation range per step)
            assert (sizes - held).max() <= stretch * (n_prbs + 1)
            held, grown = sizes, now
            if s0 + stretch < steps:
                removed = ag.prune(target)
                held = ag.dictionary_sizes().astype(np.int64)
                assert held.max() <= target and (held == np.minimum(sizes, target)).all() and removed == (sizes - held).sum()
        flags = np.zeros(N, dtype=np.int32)
        assert ag.L.kb_get_flags(ag.h, flags.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))) == 0
        assert not (flags & ~(8 | 16)).any()
        hist.append(ag.history_fetch())
        final.append(ag.dictionary_sizes().copy())
        pruned.append(ag.pruned().copy())
        ag.close()
        env.close()
    assert hist[0]['recorded'] == hist[1]['recorded'] == steps
    for key in ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation'):
        assert _bits(hist[0][key]) == _bits(hist[1][key]), key
    assert (final[0] == final[1]).all() and (pruned[0] == pruned[1]).all() and pruned[0].sum() > 0
    print('closed loop: largest dictionary at the end %d, landmarks pruned %d' % (final[0].max(), pruned[0].sum()))


def test_evaluators_prune_between_stretches(golden_dir, tmp_path):
    """BatchedEvaluator / evaluate_grid with prune_to, prune_every.  Defaults: the six keys and no `pruned`.  A budget that never
    bites (prune_to = the capacity) gives the default's files bit for bit, with pruned = 0.  A budget of 64 every 50 steps:
    `pruned` is what the agent counted (train() advances as evaluate_all does), the same through evaluate_grid, and the same
    when the evaluation is cut at step 130 and resumed from its checkpoint (the device counters restart on load)."""
    import experiments_kbrl as ek
    import scenario_creator as sc
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    sc.set_fading([g['t0'], g['t1'], g['t2']])
    try:
        steps, runs, a_range, cap = 240, [0, 1, 2, 3], [0.97, 0.99], 1024
        kw = dict(verbose=False, capacity=cap, pool_bytes=1 << 30)
        keys = ['SLA', 'adjusted', 'hits', 'resources', 'reward', 'violation']
        plain = [np.load(f) for f in ek.BatchedEvaluator(0, a_range, steps=steps, out_dir=str(tmp_path / 'plain')).evaluate_all(runs, **kw)]
        idle = [np.load(f) for f in ek.BatchedEvaluator(0, a_range, steps=steps, out_dir=str(tmp_path / 'idle'), prune_to=cap,
                                                        prune_every=50).evaluate_all(runs, **kw)]
        for a, b in zip(plain, idle):
            assert sorted(a.files) == keys and sorted(b.files) == sorted(keys + ['pruned'])
            assert b['pruned'].dtype == np.int64 and b['pruned'] == 0
            for key in keys:
                assert a[key].dtype == b[key].dtype and _bits(a[key]) == _bits(b[key]), key
        new = lambda d: ek.BatchedEvaluator(0, a_range, steps=steps, out_dir=str(tmp_path / d), prune_to=64, prune_every=50)
        cut = [np.load(f) for f in new('cut').evaluate_all(runs, **kw)]
        ev = new('train')
        agent, _ = ev.train(runs, capacity=cap, pool_bytes=1 << 30)
        agent.synchronize()
        counted = agent.pruned().sum(axis=1)
        ev.release()
        print('landmarks pruned per run:', counted)
        assert counted.sum() > 0 and [int(z['pruned']) for z in cut] == list(counted)
        grid = ek.evaluate_grid([(0, a_range)], runs, steps=steps, out_dir=str(tmp_path / 'grid'), capacity=cap, pool_bytes=1 << 30,
                                prune_to=64, prune_every=50)[(0, a_range[0])]
        ck = str(tmp_path / 'cell.npz')
        assert new('resumed').evaluate_all(runs, checkpoint=ck, stop_after=130, **kw) is None
        resumed = new('resumed').evaluate_all(runs, checkpoint=ck, **kw)
        for a, fb, fc in zip(cut, grid, resumed):
            for f in (fb, fc):
                b = np.load(f)
                assert sorted(a.files) == sorted(b.files)
                for key in a.files:
                    assert _bits(a[key]) == _bits(b[key]), (f, key)
    finally:
        sc.set_fading(None)
