"""kb_set_shared_online_prune (SharedVecKBRL.set_shared_online_prune) on the device: the budget stage at
the end of every shared learning step leaves, bit for bit, what kb_shared_prune (shrink) leaves at the same point.

No comparison carries a tolerance.  The references are shrink() itself on a twin that took the same inputs, and
tests/prune_mirror.py loaded with the device's own state (the way tests/test_gpu_prune_chain.py loads it).  Dictionaries are
those tests/test_gpu_shared_prune.py grows: learners of ten and of three state variables, (200, 131), (264, 300) and (128, 128)
landmarks at capacities 256 / 512 / 128 -- on both sides of a shell seam and of KB_GEMM_M = 256 -- shared by 4 to 8 replicas.

A stage removes at most `rounds` <= 64 landmarks per dictionary.  Where a case asks for equality with shrink(target) after a
step whose excess is larger (dictionaries of 200 landmarks and target 100: the first step), the handle under test takes the
missing stages through kb_shared_online_prune_stage directly behind the step: the removals are the same ones in the same order
however they are cut into stages."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_prune_chain as tpc   # noqa: E402
import test_gpu_shared_prune as tsp   # noqa: E402
from test_gpu_shared_prune import _compare, _control_batch, _dictionaries, _grown, _views   # noqa: E402
from ranslice import _lib   # noqa: E402
from ranslice.config import make_config   # noqa: E402

pytestmark = pytest.mark.gpu

ROUNDS_MAX = 64     # KB_ONLINE_ROUNDS_MAX
_ip, _fp, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
_bits = tsp._bits


def _stage(h):
    h._check(h.L.kb_shared_online_prune_stage(h.h))


def _same_state(X, Tw, what):
    """sizes, control state and dictionaries (_compare), then the two checkpoints side by side: every page row that is a
    dictionary's own (coordinates and their float32 copy, coefficient, K_f, d*, grid index and link), every stored tile of both
    triangles, heads, the off-grid count, the cache guards of every task, and the pruned counters"""
    _compare(X, Tw, what)
    vx, vt = _views(X, X.save_state()), _views(Tw, Tw.save_state())
    pick = list(range(17)) + [19, 20, 21]
    for s in range(X.S):
        for b in range(vx['shell'].shape[1]):
            assert bool(vx['shell'][s, b]) == bool(vt['shell'][s, b]), (what, s, b)
            if not vx['shell'][s, b]:
                continue
            assert _bits(tsp._page(vx, s, b)[pick]) == _bits(tsp._page(vt, s, b)[pick]), (what, 'page', s, b)
            for o in range(b + 1):
                assert _bits(tsp._tile(vx, s, b, o)) == _bits(tsp._tile(vt, s, b, o)), (what, 'lower tile', s, b, o)
                assert _bits(tsp._tile(vx, s, o, b)) == _bits(tsp._tile(vt, s, o, b)), (what, 'upper tile', s, o, b)
    for q in ('head', 'offgrid', 'm_last', 'fver', 'kf_owner'):
        assert _bits(vx[q]) == _bits(vt[q]), (what, q)
    assert (X.pruned() == Tw.pruned()).all(), what


# ------------------------------------------------------------------ 1, 7: equals shrink
def _equals_shrink(prepare, what):
    ag = _grown((200, 131), 256)
    X, Tw = ag.to_shared(0, 8), ag.to_shared(0, 8)
    for h in (X, Tw):
        prepare(h)
    X.set_shared_online_prune(100, ROUNDS_MAX)
    assert X.shared_online_prune == (100, ROUNDS_MAX) and Tw.shared_online_prune is None
    rng = np.random.default_rng(41)
    stages, removed = 0, []
    for i in range(3):
        st, ac, lb = _control_batch(rng, 8)
        nxt = _control_batch(rng, 8)[0]
        ht = Tw.update_control(st, ac, lb)
        excess = int(max(Tw.dictionary_sizes().max() - 100, 0))
        removed.append(Tw.shrink(100))
        hx = X.update_control(st, ac, lb)
        extra = max(-(-excess // ROUNDS_MAX) - 1, 0)       # the stages beyond the step's own that this excess needs
        for _ in range(extra):
            _stage(X)
        stages += 1 + extra
        assert (i == 0) == (extra > 0), (what, i, excess)  # (200 landmarks against a target of 100: the first step only)
        assert _bits(hx) == _bits(ht), (what, i, 'hits')
        assert list(X.dictionary_sizes()) == [100, 100]
        for p, q in zip(X.select_action(nxt), Tw.select_action(nxt)):
            assert _bits(p) == _bits(q), (what, i, 'actions / adjusted')
        _same_state(X, Tw, (what, i))
    info = X.shared_online_prune_info()
    assert info['stages'] == stages and info['removed'] == int(X.pruned().sum()) == sum(removed) and info['flagged'] == 0
    assert removed[0] >= 131 and sum(removed[1:]) > 0, removed      # (the later steps' stages met insertions to take back)
    X.close()
    Tw.close()


def test_equals_shrink():
    """two to_shared twins of (200, 131) take the same three update_control + select_action steps, one with the stage on (target
    100, rounds 64), the other calling shrink(100) after each update_control: equal after every step in everything listed in
    _same_state, hits and actions included"""
    _equals_shrink(lambda h: None, 'projectron')


def test_equals_shrink_under_the_margin_rule():
    """the same with the rounds learning by Projectron++ (kb_set_shared_plus)"""
    _equals_shrink(lambda h: h.set_shared_plus(True), 'shared_plus')


def test_equals_shrink_under_the_margin_rule_in_segments():
    """the same with growing dictionaries taking their lists in segments (kb_set_shared_plus_batch)"""
    def prepare(h):
        h.set_shared_plus(True)
        h.set_shared_plus_batch(64, 4)
    _equals_shrink(prepare, 'shared_plus_batch')


# ------------------------------------------------------------------ 2: carry, against the mirror
@pytest.mark.parametrize('rounds', [1, 2])
def test_carry_against_the_mirror(rounds):
    """target 120 on (200, 131): the excess (80 and 11 at least) is larger than `rounds`, so every stage takes exactly `rounds`
    from each dictionary and carries it.  Before each step a twin with the switch off loads X's checkpoint and takes the same
    update_control: its state is the state the stage met.  A mirror loaded from it and advanced `rounds` times holds X's bytes."""
    target = 120
    ag = _grown((200, 131), 256)
    X, Tw = ag.to_shared(0, 4), ag.to_shared(0, 4)
    X.set_shared_online_prune(target, rounds)
    rng = np.random.default_rng(43)
    want = dict(stages=0, removed=0, carry=0, max_excess=0, flagged=0)
    for i in range(3):
        Tw.load_state(X.save_state())
        st, ac, lb = _control_batch(rng, 4)
        ht = Tw.update_control(st, ac, lb)
        hx = X.update_control(st, ac, lb)
        assert _bits(hx) == _bits(ht), (rounds, i)
        dev_t, dev_x = tpc._Dev(Tw), tpc._Dev(X)
        vt, vx = dev_t.views(), dev_x.views()
        before = Tw.dictionary_sizes().astype(int)
        want['stages'] += 1
        for d in range(2):
            excess = int(before[d]) - target
            assert excess > rounds, (rounds, i, d, excess)
            k = min(excess, rounds)
            mr = tpc._load(dev_t, vt, d)
            for _ in range(k):
                assert mr.remove_one()['diag_ok']
            tpc._hold(dev_x, vx, d, mr, int(before[d]), 'rounds %d, step %d, dictionary %d' % (rounds, i, d))
            want['removed'] += k
            want['carry'] += 1 if excess > k else 0
            want['max_excess'] = max(want['max_excess'], excess)
        assert list(X.dictionary_sizes()) == list(before - rounds)
        info = X.shared_online_prune_info()
        assert {q: info[q] for q in want} == want, (rounds, i, info)
        assert info['downdate_bytes'] > 0
    assert int(X.pruned().sum()) == want['removed'] and Tw.shared_online_prune_info()['stages'] == 0
    X.close()
    Tw.close()


# ------------------------------------------------------------------ 3: the resident loop
def test_nothing_stale_in_the_resident_loop(golden_dir):
    """The small environment of tests/test_gpu_shared_prune.py, dictionaries of (264, 300) at capacity 512, one exchange round per
    step (at most 8 insertions per slice and step, so 64 rounds cover every excess over 255).  X runs step_resident with the stage
    on: it takes both dictionaries below KB_GEMM_M inside the step, between the rounds and the select.  The twin is driven from
    the host on the rows X's environment holds: update_control(previous observation, executed actions, labels), shrink(255),
    select_action(observation).  After every step the dictionaries are equal and the actions X left in its environment are the
    twin's.  (A stage enqueued behind the select, or scores kept from before the stage, show here: DESIGN.md section 8t.)"""
    from ranslice.vec_env import VecRanSlice
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    fading = [g['t0'], g['t1'], g['t2']]
    ag = _grown((264, 300), 512)
    N, target = 8, 255
    X, Tw = ag.to_shared(0, N, max_rounds=1), ag.to_shared(0, N, max_rounds=1)
    env = VecRanSlice(n_envs=N, cfg=make_config(3, n_envs=N, n_prbs=tsp.N_PRBS), fading=fading, seed=5)
    env.reset()
    env.step(np.tile(np.array(tsp.IA, dtype=np.int32), (N, 1)))
    # one resident step with the switch off on X alone, mirrored by nothing: from here on the observation X learns from next is
    # the one its environment held before the step, which the host can read
    prev = env.fetch()['obs']
    X.step_resident(env)
    X.synchronize()
    Tw.load_state(X.save_state())
    X.set_shared_online_prune(target, ROUNDS_MAX)
    assert X.dictionary_sizes().min() >= tsp.KB_GEMM_M
    removed, base = 0, (X.stats(), Tw.stats())
    for i in range(3):
        env.step_resident()
        env.synchronize()
        f = env.fetch()
        Tw.update_control(prev, f['actions'], f['labels'])
        over = Tw.dictionary_sizes().astype(int) - target
        assert over.max() <= ROUNDS_MAX and (i > 0 or over.min() > 0), (i, over)
        removed += Tw.shrink(target)
        want = Tw.select_action(f['obs'])[0]
        prev = f['obs']
        X.step_resident(env)
        X.synchronize()
        assert list(X.dictionary_sizes()) == [target, target] and target < tsp.KB_GEMM_M
        assert _bits(env.fetch()['actions']) == _bits(want), ('actions', i)
        _compare(X, Tw, ('resident', i))
        # the select counts its kernel evaluations with the size of the dictionary it read (kb_get_stats[3]): X's select read
        # the pruned dictionaries, as the twin's did.  (Where the actions happen to agree, this is what shows a stage enqueued
        # behind the select: DESIGN.md section 8t, mutation A.)
        dx, dt = ([a - b for a, b in zip(h.stats(), b0)] for h, b0 in ((X, base[0]), (Tw, base[1])))
        assert dx == dt, ('stats since the twin was loaded', i, dx, dt)
    info = X.shared_online_prune_info()
    assert info['stages'] == 3 and info['removed'] == removed and info['carry'] == 0, info
    for h in (X, Tw, env):
        h.close()


# ------------------------------------------------------------------ 4: learning goes on
def test_learning_goes_on():
    """capacity 128, both dictionaries full: with the switch off three batches insert nothing; with target 96 the same batches
    insert, no dictionary ever exceeds 128 and the pool's bytes in use do not move"""
    ag = _grown((128, 128), 128)
    rng = np.random.default_rng(23)
    batches = [_control_batch(rng, 8) for _ in range(3)]
    off, on = ag.to_shared(0, 8), ag.to_shared(0, 8)
    on.set_shared_online_prune(96, 32)
    grown0, used = on.stats()[2], on.pool()['used_bytes']
    assert off.stats()[2] == grown0
    for st, ac, lb in batches:
        off.update_control(st, ac, lb)
        on.update_control(st, ac, lb)
        assert list(off.dictionary_sizes()) == [128, 128]
        assert on.dictionary_sizes().max() <= 128
        assert on.pool()['used_bytes'] == used
    assert off.stats()[2] == grown0
    added = on.stats()[2] - grown0
    print('insertions with the stage on: %d, sizes %s' % (added, list(on.dictionary_sizes())))
    assert added > 0
    assert int(on.dictionary_sizes().sum()) == 256 + added - int(on.pruned().sum())
    off.close()
    on.close()


# ------------------------------------------------------------------ 5: shards
def test_shards_hold_the_same_bytes():
    """one handle of 8 replicas through kb_shared_step beside W = 2 handles of 4 that exchange their proposals by hand and end
    each step with kb_shared_online_prune_stage, all three with the same setting: two steps at a target nothing reaches (255: a
    step inserts at most 8 x 3 landmarks per slice), then three at target 100 -- the first of which takes 64 from the larger
    dictionary and carries it.
    Dictionary bytes, hits and actions are identical throughout; nothing is exchanged for the stage."""
    from ranslice.kbrl_dev import PROP_W, merge_proposals
    ag = _grown((200, 131), 256)
    N, W, n, S, budget, rounds = 8, 2, 4, 2, 16, 3
    whole = ag.to_shared(0, N, budget=budget, max_rounds=rounds)
    parts = [ag.to_shared(0, n, budget=budget, max_rounds=rounds, first_env=w * n) for w in range(W)]
    everyone = [whole] + parts

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
        for p in parts:
            _stage(p)
        return np.concatenate(hits)

    rng = np.random.default_rng(29)

    def steps(count, what):
        for i in range(count):
            st, ac, lb = _control_batch(rng, N)
            hw = whole.update_control(st, ac, lb)
            assert (hw == parts_update(st, ac, lb)).all(), (what, i)
            nxt = _control_batch(rng, N)[0]
            aw = whole.select_action(nxt)[0]
            ap = np.concatenate([p.select_action(nxt[w * n:(w + 1) * n])[0] for w, p in enumerate(parts)])
            assert (aw == ap).all(), (what, i)
            dw = _dictionaries(whole)
            for p in parts:
                tsp._same_dictionaries(_dictionaries(p), dw, (what, i))

    for h in everyone:
        h.set_shared_online_prune(255, 2)
    steps(2, 'nothing over the target')
    for h in everyone:
        info = h.shared_online_prune_info()
        assert info['stages'] == 2 and info['removed'] == 0 and info['carry'] == 0, info
    sizes = whole.dictionary_sizes().astype(int)
    assert sizes.min() > 100 and sizes.max() > 100 + ROUNDS_MAX     # (the larger one is carried by the first stage that removes)
    for h in everyone:
        h.set_shared_online_prune(100, ROUNDS_MAX)
    steps(3, 'over the target')
    infos = [h.shared_online_prune_info() for h in everyone]
    assert infos[0] == infos[1] == infos[2] and infos[0]['stages'] == 5 and infos[0]['removed'] > ROUNDS_MAX and infos[0]['carry'] >= 1, infos
    pruned = [h.pruned() for h in everyone]
    assert (pruned[0] == pruned[1]).all() and (pruned[0] == pruned[2]).all() and int(pruned[0].sum()) == infos[0]['removed']
    for h in everyone:
        h.close()


# ------------------------------------------------------------------ 6: idle and off
def _timeless(h, blob):
    """the checkpoint with the words zeroed that hold wall-clock time: the apply kernels add their duration per slice to
    d_gstats[8 .. 8 + S) in every build (kb_kbrl.hip: wall_clock64), and d_gstats is a saved region -- two untouched twins differ
    there.  d_gstats [32] is sought from the blob's end (behind it lie d_block, d_mprops, d_mcounts, d_taken and d_total:
    kb_api.hip, the allocation order) and then HELD to what the apply kernels keep in it, so that a change of the saved regions
    fails here instead of masking other bytes: gstats[1] (samples that changed a dictionary) is the sum of the per-slice counts
    gstats[16 + s], gstats[2] (insertions) is no larger, the per-slice list lengths gstats[24 + s] are no smaller than what was
    applied from them, and the words of the slices the handle does not have are zero.  (Words that are all zero pass, and
    zeroing them masks nothing.)"""
    from ranslice.kbrl_dev import PROP_W
    S, cap = h.S, 256                                        # (budget_cap)
    tail = 8 * S * (1 + cap * PROP_W) + 8 * S * cap * PROP_W + 4 * S + 4 * S + 8
    o = blob.size - tail - 8 * 32
    g = blob[o:o + 8 * 32].view(np.uint64)
    assert int(g[1]) == int(g[16:16 + S].sum()) and int(g[2]) <= int(g[1]) and (g[24:24 + S] >= g[16:16 + S]).all(), g
    assert not g[8 + S:16].any() and not g[16 + S:24].any() and not g[24 + S:32].any(), g
    out = blob.copy()
    out[o + 8 * 8:o + 8 * 16] = 0
    return out


def test_idle_and_off_leave_every_byte():
    """a target no dictionary exceeds (255: three steps of one round insert at most 24), and a switch set and cleared again: after
    every step the checkpoint holds the bytes of an untouched twin's (all of them but the eight words of wall-clock time every
    checkpoint carries: _timeless).  Only the stage counter moves."""
    ag = _grown((200, 131), 256)
    U, idle, cleared = (ag.to_shared(0, 4, max_rounds=1) for _ in range(3))
    idle.set_shared_online_prune(255, 2)
    cleared.set_shared_online_prune(100, 2)
    cleared.set_shared_online_prune(0)
    assert idle.shared_online_prune == (255, 2) and cleared.shared_online_prune is None and U.shared_online_prune is None
    rng = np.random.default_rng(47)
    for i in range(3):
        st, ac, lb = _control_batch(rng, 4)
        nxt = _control_batch(rng, 4)[0]
        for h in (U, idle, cleared):
            h.update_control(st, ac, lb)
            h.select_action(nxt)
        blob = _timeless(U, U.save_state())
        assert U.dictionary_sizes().max() <= 255
        for name, h in (('idle', idle), ('cleared', cleared)):
            got = _timeless(h, h.save_state())
            assert got.size == blob.size
            assert _bits(got) == _bits(blob), (name, i, np.nonzero(got != blob)[0][:8], blob.size)
    zero = dict(stages=0, removed=0, carry=0, max_excess=0, flagged=0, downdate_bytes=0)
    assert idle.shared_online_prune_info() == dict(zero, stages=3)
    assert cleared.shared_online_prune_info() == zero and U.shared_online_prune_info() == zero
    assert not idle.pruned().any() and not (idle.flags() & 32).any()
    for h in (U, idle, cleared):
        h.close()


# ------------------------------------------------------------------ 8: a dictionary the rule refuses
def test_poisoned_dictionary():
    """Kinv[5][5] = -1 edited into the checkpoint of slice 0, on dictionaries of (128, 128) at capacity 128: a full dictionary only
    projects, so the rounds never rewrite Kinv and the entry is still there when each stage comes (an insertion adds a rank-1
    term to every entry of Kinv, and took the entry back above zero in a growing dictionary).  X (stage on, target 96) keeps, in
    that dictionary, the bytes a twin with the same poison and the switch off holds after the same rounds; every replica's flag
    word carries bit 32 and nothing else has changed in it; the other dictionary is pruned as in a clean twin with the stage on;
    the dictionary is counted once however many stages meet it; synchronize() reports no error."""
    ag = _grown((128, 128), 128)
    X, R, Cl = (ag.to_shared(0, 4, max_rounds=1) for _ in range(3))
    blob = X.save_state().copy()
    v = _views(X, blob)
    v['pool'][int(v['shell'][0, 0]) + tsp.VEC + 5 * 64 + 5] = -1.0          # Kinv[5][5] of dictionary 0
    X.load_state(blob)
    R.load_state(blob)
    X.set_shared_online_prune(96, ROUNDS_MAX)
    Cl.set_shared_online_prune(96, ROUNDS_MAX)
    rng = np.random.default_rng(53)
    for i in range(2):
        st, ac, lb = _control_batch(rng, 4)
        for h in (X, R, Cl):
            h.update_control(st, ac, lb)
        dx, dr, dc = _dictionaries(X), _dictionaries(R), _dictionaries(Cl)
        tsp._same_dictionaries(dx[:1], dr[:1], ('the poisoned dictionary', i))
        tsp._same_dictionaries(dx[1:], dc[1:], ('the other dictionary', i))
        assert dx[1]['m'] == 96 and dx[0]['m'] == 128 and dx[0]['kinv'][5, 5] == -1.0
        assert (X.flags() == (R.flags() | 32)).all() and not (R.flags() & 32).any() and not (Cl.flags() & 32).any(), i
        info = X.shared_online_prune_info()
        assert info['flagged'] == 1 and info['stages'] == i + 1, info
    assert list(X.pruned()) == [0, int(Cl.pruned()[1])] and Cl.shared_online_prune_info()['flagged'] == 0
    X.synchronize()
    for h in (X, R, Cl):
        h.close()


# ------------------------------------------------------------------ 9: refusals
def test_refusals():
    """every code and message of the four entry points; the setting survives a refusal and reset(), and is absent after load_state
    into another handle and after to_shared"""
    from ranslice.kbrl_dev import PROP_W, SharedVecKBRL
    ag = _grown((200, 131), 256)
    X = ag.to_shared(0, 4, budget=16)
    X.set_shared_online_prune(128, 3)

    def refused(call, code, *names):
        with pytest.raises(_lib.RanSliceError) as ei:
            call()
        assert ei.value.code == code, str(ei.value)
        for n in names:
            assert n in str(ei.value), (n, str(ei.value))

    who = 'kb_set_shared_online_prune'
    refused(lambda: X.set_shared_online_prune(63), _lib.RS_EINVAL, who, 'target')
    refused(lambda: X.set_shared_online_prune(256), _lib.RS_EINVAL, who, 'target', 'capacity - 1')
    refused(lambda: X.set_shared_online_prune(-1), _lib.RS_EINVAL, who, 'target')
    refused(lambda: X.set_shared_online_prune(128, 0), _lib.RS_EINVAL, who, 'rounds')
    refused(lambda: X.set_shared_online_prune(128, 65), _lib.RS_EINVAL, who, 'rounds')
    assert X.shared_online_prune == (128, 3)
    X.set_shared_online_prune(255, 64)                      # the ends of both ranges
    X.set_shared_online_prune(64, 1)
    X.set_shared_online_prune(128, 3)
    # a per-replica handle: the setter and the stage name its own switch
    refused(lambda: ag._check(ag.L.kb_set_shared_online_prune(ag.h, 128, 2)), _lib.RS_ESTATE, who, 'kb_set_online_prune')
    refused(lambda: _stage(ag), _lib.RS_ESTATE, 'kb_shared_online_prune_stage', 'kb_set_online_prune')
    assert ag.online_prune is None
    # and the per-replica switch keeps refusing the shared handle
    refused(lambda: X.set_online_prune(128, 2), _lib.RS_ESTATE, 'kb_set_online_prune', 'kb_shared_prune')
    with pytest.raises(ValueError, match='online_prune'):
        SharedVecKBRL(4, tsp.DIMS, tsp.N_PRBS, capacity=256, online_prune=128)
    assert X.online_prune is None and X.shared_online_prune == (128, 3)
    assert X.online_prune_info()['stages'] == 0            # (the per-replica counters never read the shared stages')
    zero = SharedVecKBRL(4, tsp.DIMS, tsp.N_PRBS, capacity=256, shared_online_prune=0)
    assert zero.shared_online_prune is None                 # (0 is off: nothing waits for reset())
    zero.close()
    # never reset: the keyword waits for the first reset()
    fresh = SharedVecKBRL(4, tsp.DIMS, tsp.N_PRBS, capacity=256, shared_online_prune=100, shared_online_prune_rounds=5)
    refused(lambda: fresh._check(fresh.L.kb_set_shared_online_prune(fresh.h, 128, 2)), _lib.RS_ESTATE, who, 'kb_reset')
    t, r = C.c_int32(-1), C.c_int32(-1)
    fresh._check(fresh.L.kb_get_shared_online_prune(fresh.h, C.byref(t), C.byref(r)))
    assert (t.value, r.value) == (0, 2) and fresh.shared_online_prune == (100, 5)
    fresh.reset([tsp.IA] * 4, [tsp.SF] * 4)
    fresh._check(fresh.L.kb_get_shared_online_prune(fresh.h, C.byref(t), C.byref(r)))
    assert (t.value, r.value) == (100, 5) and fresh.shared_online_prune == (100, 5)
    fresh.reset([tsp.IA] * 4, [tsp.SF] * 4)                 # kb_reset leaves it
    assert fresh.shared_online_prune == (100, 5)
    # the stage while the switch is off
    off = ag.to_shared(0, 4)
    assert off.shared_online_prune is None                  # to_shared makes a handle with the switch off
    refused(lambda: _stage(off), _lib.RS_ESTATE, 'kb_shared_online_prune_stage', 'kb_set_shared_online_prune')
    off.load_state(X.save_state())                          # checkpoints do not hold it
    assert off.shared_online_prune is None and X.shared_online_prune == (128, 3)
    X.load_state(off.save_state())                          # and loading one leaves the handle's own
    assert X.shared_online_prune == (128, 3)
    # between kb_shared_scan and kb_shared_commit: a scan that found proposals leaves the round open
    rng = np.random.default_rng(31)
    st, ac, lb = _control_batch(rng, 4)
    hits, counts, props = np.zeros((4, 2), dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros((2, 16, PROP_W))
    X._check(X.L.kb_shared_scan(X.h, st.ctypes.data_as(_fp), ac.ctypes.data_as(_ip), lb.ctypes.data_as(_ip), 0, 16,
                                hits.ctypes.data_as(_ip), counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp)))
    assert counts.sum() > 0
    refused(lambda: X.set_shared_online_prune(100, 2), _lib.RS_ESTATE, who, 'kb_shared_commit')
    refused(lambda: _stage(X), _lib.RS_ESTATE, 'kb_shared_online_prune_stage', 'kb_shared_commit')
    X._check(X.L.kb_shared_apply(X.h, counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp), 16))
    refused(lambda: _stage(X), _lib.RS_ESTATE, 'kb_shared_online_prune_stage', 'kb_shared_commit')
    X._check(X.L.kb_shared_commit(X.h, counts.ctypes.data_as(_ip)))
    assert X.shared_online_prune == (128, 3)
    sizes = X.dictionary_sizes().astype(int)
    _stage(X)                                               # the round is closed: one stage, three removals where over 128
    assert list(X.dictionary_sizes()) == [s - min(max(s - 128, 0), 3) for s in sizes]
    X.update_control(st, ac, lb)
    X.select_action(st)
    for h in (X, fresh, off):
        h.close()
