"""One pass over Kinv for a group of candidates in the closed loop's Projectron++ update phase (kb_set_control_plus_batch;
DESIGN.md §8m): whatever the width, the bytes are those of width 0.

1. G19 teacher-forced at width 8 beside a twin at width 0 (300 steps; 60 at widths 2 and 4): every step's hits, actions, adjusted,
   margins, security factors and sizes; at the end landmarks, coefficients and all of Kinv as bytes, the statistics,
   kb_get_repair_work, and kb_control_plus_batch_info against expected_work of the recording.
2. The size ladder: line learners (tests/control_plus_batch_rows.py) of 0 .. 320 landmarks, rows whose insertions fall on the walk's
   seams; update_control at widths 0 and 8, one kb_fit_steps call, and kb_fit on the augmented samples (whose per-sample record
   says where the insertions fell): equal bytes four ways.
3. Group edges: n_prbs = 9, rows of 1, 7, 8, 9 and 10 candidates for both labels, and a row that makes no pass at all.
4. The arena's limit: max_landmarks = 128 with learners of 127, 128 and 129 landmarks.
5. The resident paths, plain and captured, 24 replicas.  6. A checkpoint taken at width 8 continues at width 0.  7. The switch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ranslice.config import make_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_plus_batch_mirror as bm   # noqa: E402
import control_plus_batch_rows as rows_of   # noqa: E402
from test_gpu_control_plus import _load, _same_dictionaries, _same_learner   # noqa: E402

pytestmark = pytest.mark.gpu
POOL = 256 << 20
DIMS = [10, 3]


def _handle(n_envs, dims, n_prbs, width=0, max_landmarks=1024, capacity=1024, g=None, seeds=None, **kw):
    from ranslice.kbrl_dev import VecKBRL
    kw.setdefault('algorithm', 'projectron_plus')
    kw.setdefault('control_plus', True)
    h = VecKBRL(n_envs, dims, n_prbs, capacity=capacity, pool_bytes=POOL, control_plus_batch=width, control_plus_batch_max=max_landmarks,
                **(dict(accuracy_range=tuple(g['a_range'])) if g is not None else {}), **kw)
    ia = np.tile(g['init_action'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 1)
    sf = np.tile(g['init_sec'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 1)
    h.reset(ia, sf, seeds=seeds)
    return h


def _same_control(a, b):
    ca, cb = a.control(), b.control()
    for k in ca:
        assert ca[k].tobytes() == cb[k].tobytes(), k


def _same_everything(a, b):
    _same_dictionaries(a, b)
    _same_control(a, b)
    assert a.stats() == b.stats()
    assert [int(v) for v in a._repair_raw()] == [int(v) for v in b._repair_raw()]


# ---------------------------------------------------------------------------------------------- 1. G19, teacher-forced

@pytest.mark.parametrize('width,steps', [(8, 300), (2, 60), (4, 60)])
def test_g19_teacher_forced_beside_width_0(golden_dir, width, steps):
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    assert len(g['ties']) == 0
    a = _handle(1, dims, n_prbs, width, g=g, seeds=np.zeros(1, dtype=np.uint64))
    b = _handle(1, dims, n_prbs, 0, g=g, seeds=np.zeros(1, dtype=np.uint64))
    assert a.control_plus_batch == (width, 1024, 128 + 5 * 2 * width * 1024 * 8) and b.control_plus_batch == (0, 0, 0)
    nxt = np.concatenate([state[1:], np.asarray(g['final_state'], dtype=np.float32)[None]])
    for i in range(steps):
        ha, hb = (h.update_control(state[i][None], action[i][None], labels[i][None]) for h in (a, b))
        assert np.array_equal(ha, hb) and np.array_equal(ha[0], g['hits'][i]), i
        (act_a, adj_a), (act_b, adj_b) = (h.select_action(nxt[i][None]) for h in (a, b))
        assert np.array_equal(act_a, act_b) and np.array_equal(adj_a, adj_b) and np.array_equal(act_a[0], g['action_out'][i]), i
        ca, cb = a.control(with_accuracies=False), b.control(with_accuracies=False)
        for k in ('margins', 'security_factors', 'adjusted'):
            assert np.array_equal(ca[k], cb[k]), (i, k)
        assert np.array_equal(a.dictionary_sizes(), b.dictionary_sizes()) and np.array_equal(a.dictionary_sizes()[0], g['set_size'][i]), i
    _same_everything(a, b)
    # the counters, from the recording alone
    counts = np.where(labels[:steps] == 1, n_prbs - action[:steps] + 1, action[:steps] + 1).sum(axis=0)
    br = [g['branch%d' % s][:counts[s]] for s in range(len(dims))]
    want = bm.expected_work(br, [0] * len(dims), action[:steps], labels[:steps], width, 1024, n_prbs=n_prbs)
    got = a.control_plus_batch_work()
    print('width %d, %d steps: work %s' % (width, steps, got))
    assert got == want and got[2] > 0 and got[1] > 0 and got[5] > 0 and got[6] > 0
    assert b.control_plus_batch_work() == [0] * 8
    # kb_get_repair_work's work[6]: the candidates that used a d*, grouped or not
    assert int(a._repair_raw()[6]) == int(sum((x != 0).sum() for x in br))
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 2 - 4. hand-made learners and rows

def _scenario(sizes, n_prbs, make_rows):
    """sizes [N][S] of line learners; make_rows(m, d, e, s) -> rows of that learner -> the pre-growth lists for kb_fit and the log
    state [R, N, nv], action [R, N, S], labels [R, N, S]"""
    N, S = len(sizes), len(DIMS)
    off = np.concatenate([[0], np.cumsum(DIMS)])
    per = [[make_rows(sizes[e][s], DIMS[s], e, s) for s in range(S)] for e in range(N)]
    R = len(per[0][0])
    state = np.zeros((R, N, int(off[-1])), dtype=np.float32)
    action, labels = np.zeros((R, N, S), dtype=np.int64), np.zeros((R, N, S), dtype=np.int64)
    for e in range(N):
        for s in range(S):
            assert len(per[e][s]) == R
            for r, (st, act, lab) in enumerate(per[e][s]):
                state[r, e, off[s]:off[s + 1]] = st
                action[r, e, s], labels[r, e, s] = act, lab
    assert ((action >= 0) & (action <= n_prbs)).all()
    grow = [((e, s),) + rows_of.line_samples(sizes[e][s], DIMS[s]) for e in range(N) for s in range(S) if sizes[e][s] > 0]
    return grow, state, action, labels


def _pregrow(h, grow, sizes):
    out = h.fit([g[0] for g in grow], [g[1] for g in grow], [g[2] for g in grow])
    assert all((b == 2).all() for b in out['branch'])          # every sample of a line learner is inserted
    assert np.array_equal(h.dictionary_sizes(), np.asarray(sizes))


def _four_ways(sizes, n_prbs, make_rows, width, max_landmarks):
    """-> (the width-`width` handle's counters per row, expected_work of the recorded branches, the insertions of the record, the
    handles' common hits); asserts the bytes four ways on the way"""
    from ranslice.kbrl_dev import augmented_samples
    grow, state, action, labels = _scenario(sizes, n_prbs, make_rows)
    N, S, R = len(sizes), len(DIMS), len(state)
    a0, a8, b, c = (_handle(N, DIMS, n_prbs, w, max_landmarks) for w in (0, width, 0, 0))
    for h in (a0, a8, b, c):
        _pregrow(h, grow, sizes)
    base = [np.array(h.stats(), dtype=np.int64) for h in (a0, a8, b, c)]
    # update_control, row by row, at both widths
    hits, per_row, before = [], [], a8.control_plus_batch_work()
    for r in range(R):
        h0, h8 = (h.update_control(state[r], action[r], labels[r]) for h in (a0, a8))
        assert np.array_equal(h0, h8), r
        hits.append(h8)
        now = a8.control_plus_batch_work()
        per_row.append([y - x for x, y in zip(before, now)])
        before = now
    _same_everything(a0, a8)
    # one kb_fit_steps call
    out = b.fit_steps(list(range(N)), state.transpose(1, 0, 2), action.transpose(1, 0, 2), labels.transpose(1, 0, 2))
    _same_dictionaries(a8, b)
    m_prev = np.concatenate([np.asarray(sizes)[None], np.stack(out['m'], axis=1)[:-1]])    # [R, N, S]
    f_at, y_at = np.stack(out['f_at'], axis=1), np.stack(out['y_at'], axis=1)
    assert (f_at[m_prev > 0] != 0.0).all()                                                    # no tie draw separates the paths
    assert np.array_equal(np.array(hits), (labels == y_at).astype(np.int32))
    # kb_fit on the augmented samples: the per-sample record
    learners, X, Y = [], [], []
    for e in range(N):
        Xe, Ye = augmented_samples(state[:, e], action[:, e], labels[:, e], DIMS, n_prbs)
        for s in range(S):
            learners.append((e, s))
            X.append(Xe[s])
            Y.append(Ye[s])
    rec = c.fit(learners, X, Y)
    _same_dictionaries(a8, c)
    added = [np.array(h.stats(), dtype=np.int64) - x for h, x in zip((a0, a8, b, c), base)]
    assert added[0].tolist() == added[1].tolist() == added[2].tolist() == added[3].tolist()
    want, insertions = [0] * 8, []
    for e in range(N):
        br = [rec['branch'][e * S + s] for s in range(S)]
        for s in range(S):   # no ties inside the rows either
            mb = np.concatenate([[sizes[e][s]], rec['m'][e * S + s][:-1]])
            assert (rec['f'][e * S + s][mb > 0] != 0.0).all(), (e, s)
        ins = []
        w = bm.expected_work(br, sizes[e], action[:, e], labels[:, e], width, max_landmarks, n_prbs=n_prbs, insertions=ins)
        want = [x + y for x, y in zip(want, w)]
        insertions += [(e,) + t for t in ins]
    got = a8.control_plus_batch_work()
    print('work', got, 'insertions (agent, learner, row, size, position, group):', insertions)
    assert got == want and [sum(col) for col in zip(*per_row)] == got
    assert a0.control_plus_batch_work() == [0] * 8
    for h in (a0, a8, b, c):
        h.close()
    return per_row, want, insertions


SIZES10 = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 320]
SIZES3 = [2, 64, 65, 0, 1, 3, 66, 2, 64, 65, 0, 1, 3, 66, 5]


def test_size_ladder_four_ways():
    """learners of every size at which the walk, the tiles or the prefix store change their path, ten and three state variables;
    rows (control_plus_batch_rows.seam_rows, n_prbs = 41) that insert as the first candidate of a row -- one by one at 0 and 1
    landmarks, entering grouping mid-row at 1 -> 2; inside a group at 64 -> 65, where a new shell appears -- and at position 0,
    3 or 7 of an 8-wide group further into a row"""
    sizes = [[SIZES10[e], SIZES3[e]] for e in range(15)]
    _, work, ins = _four_ways(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, (0, 3, 7)[(e + s) % 3]), 8, 1024)
    seen = {(m, pos, g) for _, _, _, m, pos, g in ins}
    assert (0, -1, -1) in seen and (1, -1, -1) in seen          # one by one: the empty dictionary, 1 -> 2
    rows_1_to_2 = [(e, s, t) for e, s, t, m, pos, g in ins if m == 1]
    assert rows_1_to_2 and work[6] > 0                          # ... and the rest of that row was grouped (41 more candidates)
    assert any(m == 64 and pos >= 0 for m, pos, g in seen)      # 64 -> 65 inside a group: a new shell
    assert {pos for m, pos, g in seen if g == 8} >= {0, 3, 7}   # first, middle and last column of a full group
    assert any(m >= 256 and pos >= 0 for m, pos, g in seen)     # beyond the prefix store


def test_group_edges():
    """n_prbs = 9, width 8: rows of 1, 7, 8, 9 and 10 candidates for both labels (control_plus_batch_rows.edge_rows), on learners
    of 2, 4, 64 and 66 landmarks -- one parity, so that the row that is walked a second time is the same row for all of them.
    Every other row inserts its first candidate (groups of 1, 7 and 8 cut behind their first column, the 9th and 10th candidate
    in a group of their own); the repeated row makes no pass at all: its only candidate has f = 1.0, its one group is skipped"""
    sizes = [[2, 66], [66, 2], [4, 64]]
    where = set()

    def make(m, d, e, s):
        rows, again = rows_of.edge_rows(m, d)
        where.add(again)
        return rows
    per_row, work, ins = _four_ways(sizes, 9, make, 8, 1024)
    assert len(where) == 1 and len(per_row) == 11
    r = where.pop()
    assert per_row[r][2] == 0 and per_row[r][1] == 6 and per_row[r][0] == 6 and per_row[r][6] == 0
    assert all(row[2] > 0 for i, row in enumerate(per_row) if i != r)
    assert len(ins) == 10 * 6 and all(pos == 0 for _, _, _, _, pos, g in ins)
    assert {g for _, _, _, _, pos, g in ins} == {1, 7, 8}
    assert work[1] == 6 and work[6] == 0


def test_the_arenas_limit():
    """max_landmarks = 128: a learner of 128 landmarks is grouped until it inserts, one of 129 goes one by one, one of 127 grows to
    128 in its first row (still grouped) and past it inside its second: grouped up to that insertion, one by one behind it"""
    sizes = [[127, 2], [128, 64], [129, 65]]
    _, work, ins = _four_ways(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, 3), 8, 128)
    by = {(e, s, t): (m, pos) for e, s, t, m, pos, g in ins}
    assert by[(0, 0, 0)] == (127, 0) and by[(0, 0, 1)] == (128, 3)       # grouped, then grouped up to the insertion at position 3
    assert by[(1, 0, 0)] == (128, 0) and by[(1, 0, 1)] == (129, -1)      # grouped; one by one
    assert by[(2, 0, 0)] == (129, -1)
    # one by one: every candidate of the 10-variable learners behind those insertions, and nobody else
    assert work[6] > 0 and work[7] > 0 and work[2] > 0


# ---------------------------------------------------------------------------------------------- 5. the resident paths

def _loop(golden_dir, graph, widths, steps_each, N=24):
    """N agents of scenario 1 in the resident loop, from equal seeds: len(widths) stretches of steps_each steps, the width set in
    front of each -> (dictionaries, control state, histories, sizes)"""
    from ranslice.vec_env import VecRanSlice
    gf = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    cfg = make_config(1, n_envs=N)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    rng = np.random.default_rng(31)
    ia = np.stack([np.concatenate([rng.integers(4, 20, cfg.n_embb), rng.integers(2, 10, cfg.n_mmtc)]) for _ in range(N)]).astype(np.int32)
    sf = np.stack([np.concatenate([rng.integers(2, 8, cfg.n_embb), rng.integers(1, 4, cfg.n_mmtc)]) for _ in range(N)]).astype(np.int32)
    env = VecRanSlice(n_envs=N, cfg=cfg, fading=[gf['t0'], gf['t1'], gf['t2']], seed=19)
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(N, dims, n_prbs, capacity=256, pool_bytes=POOL, algorithm='projectron_plus', control_plus=True)
    ag.reset(ia, sf, seeds=np.arange(N, dtype=np.uint64) + 4)
    env.reset()
    ag.history_begin(steps_each * len(widths))
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    for w in widths:
        ag.set_control_plus_batch(w, 256)
        ag.run_resident(env, steps_each, graph=graph)
    hist = ag.history_fetch()
    assert hist['recorded'] == steps_each * len(widths)
    out = ([ag.learner(r, s, with_kinv=True) for r in range(N) for s in range(len(dims))], ag.control(), hist, ag.dictionary_sizes().copy(),
           env.fetch()['obs'].copy(), ag.control_plus_batch_work())
    env.close()
    ag.close()
    return out


def _same_loops(x, ref):
    assert np.array_equal(x[3], ref[3])
    for la, lb in zip(x[0], ref[0]):
        _same_learner(la, lb)
    for k in ref[1]:
        assert x[1][k].tobytes() == ref[1][k].tobytes(), k
    for k in ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation'):
        assert x[2][k].tobytes() == ref[2][k].tobytes(), k
    assert x[4].tobytes() == ref[4].tobytes()


def test_resident_paths(golden_dir):
    """24 replicas, 10 steps of kb_run_resident, plain and captured, at widths 0 and 8: dictionaries, control state, rewards and
    the other histories as bytes.  Toggling the width between two captured stretches retires the graph: the results stay equal"""
    ref = _loop(golden_dir, False, [0], 10)
    print('sizes after 10 steps: max %d, mean %.1f' % (ref[3].max(), ref[3].mean()))
    assert ref[3].max() > 2 and ref[5] == [0] * 8
    for graph, widths, each in ((False, [8], 10), (True, [0], 10), (True, [8], 10), (True, [8, 0], 5), (True, [0, 8], 5), (False, [8, 4, 2, 0, 8], 2)):
        got = _loop(golden_dir, graph, widths, each)
        _same_loops(got, ref)
        if widths[-1]:
            assert got[5][0] > 0 and got[5][2] > 0, (graph, widths, got[5])


# ---------------------------------------------------------------------------------------------- 6. a checkpoint

def test_checkpoint_taken_at_width_8_continues_at_width_0(golden_dir):
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    a = _handle(1, dims, n_prbs, 8, g=g, seeds=np.zeros(1, dtype=np.uint64))
    b = _handle(1, dims, n_prbs, 0, g=g, seeds=np.zeros(1, dtype=np.uint64))
    P = 45
    for i in range(P):
        a.update_control(state[i][None], action[i][None], labels[i][None])
        a.select_action(state[i + 1][None])
    assert a.dictionary_sizes().max() >= 2
    b.load_state(a.save_state())
    assert b.control_plus_batch == (0, 0, 0) and a.control_plus_batch[0] == 8      # the switch is not in the blob
    for i in range(P, P + 5):
        for h in (a, b):
            h.update_control(state[i][None], action[i][None], labels[i][None])
            h.select_action(state[i + 1][None])
    _same_dictionaries(a, b)
    _same_control(a, b)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 7. the switch

def test_the_switch(golden_dir):
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL
    cfg = make_config(1, n_envs=2)
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    T = 2 * len(dims)
    ag = _handle(2, dims, cfg.n_prbs, capacity=512)
    assert ag.control_plus_batch == (0, 0, 0)
    ag.update_control(np.zeros((2, ag.nv)), np.full((2, len(dims)), 3), np.ones((2, len(dims))))     # (something to deploy)
    for w in (1, 3, 5, 6, 7, 9, 16, -2):
        assert ag.L.kb_set_control_plus_batch(ag.h, w, 128) == _lib.RS_EINVAL, w
        assert '2, 4 or 8' in ag.L.kb_last_error(ag.h).decode()
    for mx in (100, 0, 32, 576, 1024, -64):
        assert ag.L.kb_set_control_plus_batch(ag.h, 8, mx) == _lib.RS_EINVAL, mx
        assert 'multiple of 64' in ag.L.kb_last_error(ag.h).decode()
    assert ag.control_plus_batch == (0, 0, 0)
    assert ag.L.kb_set_control_plus_batch(ag.h, 0, 100) == _lib.RS_OK              # ignored while the width is 0
    for w, mx in ((8, 512), (2, 64), (4, 128)):
        ag.set_control_plus_batch(w, mx)
        assert ag.control_plus_batch == (w, mx, 128 + min(T, 1024) * 2 * w * mx * 8)
        assert ag.control_plus_batch_work() == [0] * 8
    ag.set_control_plus_batch(0)
    assert ag.control_plus_batch == (0, 0, 0) and ag.control_plus_batch_work() == [0] * 8
    # handles on which nothing learns through update_control
    for h, word in ((ag.deploy([0, 1]), 'inference-only'), (ag.deploy([1, 1, 0], by_reference=True), 'by-reference')):
        with pytest.raises(_lib.RanSliceError) as e:
            h.set_control_plus_batch(8, 64)
        assert e.value.code == _lib.RS_ESTATE and word in str(e.value) and 'does not learn through kb_update_control' in str(e.value)
        h.close()
    sh = SharedVecKBRL(2, dims, cfg.n_prbs, capacity=128, pool_bytes=64 << 20)
    assert sh.L.kb_set_control_plus_batch(sh.h, 8, 64) == _lib.RS_ESTATE and 'shared' in sh.L.kb_last_error(sh.h).decode()
    sh.close()
    ag.close()


def test_the_switch_leaves_projectron_alone(golden_dir):
    """width 8 on a Projectron handle (control_plus on as well): 5 resident steps equal, as bytes, to a handle that never set it"""
    from test_gpu_control_plus import _closed_loop, _same_runs
    full = ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation')
    for mode in ('run', 'graph'):
        ref = _closed_loop(golden_dir, mode, 5, algorithm='projectron', control_plus=False)
        got = _closed_loop(golden_dir, mode, 5, algorithm='projectron', control_plus=True, switch=lambda ag: ag.set_control_plus_batch(8, 256))
        _same_runs(got, ref, full)
        assert got[0]['obs'].tobytes() == ref[0]['obs'].tobytes()
