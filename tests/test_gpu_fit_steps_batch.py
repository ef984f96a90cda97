"""One pass over Kinv for a group of a row's candidates in kb_fit_steps, Projectron++ mode (kb_set_fit_steps_batch):
whatever the width, the bytes are those of width 0.  The method throughout: twin handles in Projectron++ mode, pre-grown alike,
take the same fit_steps call at width W and at width 0; then landmarks, coefficients, all of Kinv, sizes and flags, the statistics,
kb_get_repair_work, the control state, the five returned summaries (f_at included) and kb_fit_time_ms's work[0..3] are compared
as bytes.

1. G19 as a log: 300 rows at width 8 (60 at widths 2 and 4) in one call; the counters against expected_work of the recording;
   the dictionaries also against a handle taught the same rows by update_control.
2. The size ladder: line learners of 0 .. 320 landmarks, rows whose insertions fall on the walk's seams; kb_fit on the augmented
   samples says where the insertions fell.  3. Group edges, n_prbs = 9.  4. The arena's limit, max_landmarks = 128.
5. What only a log has: rows of label 0, a learner all of whose rows are 0, an agent listed without rows, agents not listed,
   chunks of 1, 2, 3 rows (a launch boundary between rows: the ticket's reset) and the default, f_at of +1 rows at m == 1 and m >= 2.
6. More learners (1,040) than arenas (1,024), two calls in a row.  7. An exact tie inside a row.  8. The switch."""
import os
import sys

import numpy as np
import pytest

from ranslice.config import make_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_plus_batch_mirror as bm   # noqa: E402
import control_plus_batch_rows as rows_of   # noqa: E402
from test_gpu_control_plus import _load, _same_dictionaries, _same_learner   # noqa: E402
from test_gpu_control_plus_batch import SIZES3, SIZES10, _pregrow, _scenario   # noqa: E402

pytestmark = pytest.mark.gpu
POOL = 256 << 20
DIMS = [10, 3]
SUMMARIES = ('f_at', 'y_at', 'changed', 'grown', 'm')
WORK = ('samples', 'mistakes', 'insertions', 'kernel_evals')


def _handle(n_envs, dims, n_prbs, width=0, max_landmarks=1024, capacity=1024, g=None, seeds=None, **kw):
    from ranslice.kbrl_dev import VecKBRL
    kw.setdefault('algorithm', 'projectron_plus')
    kw.setdefault('control_plus', kw['algorithm'] == 'projectron_plus')
    kw.setdefault('pool_bytes', POOL)
    h = VecKBRL(n_envs, dims, n_prbs, capacity=capacity, fit_steps_batch=width, fit_steps_batch_max=max_landmarks,
                **(dict(accuracy_range=tuple(g['a_range'])) if g is not None else {}), **kw)
    ia = np.tile(g['init_action'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 1)
    sf = np.tile(g['init_sec'], (n_envs, 1)) if g is not None else np.full((n_envs, len(dims)), 1)
    h.reset(ia, sf, seeds=seeds)
    return h


def _same_everything(a, b):
    _same_dictionaries(a, b)
    ca, cb = a.control(), b.control()
    for k in ca:
        assert ca[k].tobytes() == cb[k].tobytes(), k
    assert a.stats() == b.stats()
    assert [int(v) for v in a._repair_raw()] == [int(v) for v in b._repair_raw()]


def _same_call(a, b, agents, state, action, labels, chunk_a=0, chunk_b=0, everything=True):
    """the same fit_steps call on a (grouped) and b (one by one): equal summaries, equal work[0..3], equal handles -> a's summaries"""
    oa = a.fit_steps(agents, state, action, labels, chunk=chunk_a)
    wa = a.fit_time_ms()
    ob = b.fit_steps(agents, state, action, labels, chunk=chunk_b)
    wb = b.fit_time_ms()
    for k in SUMMARIES:
        assert len(oa[k]) == len(ob[k]) == len(agents)
        for i, (x, y) in enumerate(zip(oa[k], ob[k])):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, i)
    assert [wa[k] for k in WORK] == [wb[k] for k in WORK]
    if everything:
        _same_everything(a, b)
    return oa


def _by_agent(state, action, labels):
    """[R, N, ...] as _scenario makes them -> [N, R, ...] as fit_steps takes them"""
    return state.transpose(1, 0, 2), action.transpose(1, 0, 2), labels.transpose(1, 0, 2)


def _record(c, sizes, state, action, labels, n_prbs, width, max_landmarks):
    """kb_fit on the augmented samples of the rows [R, N, ...] on handle c (pre-grown as the twins): the per-sample record ->
    (expected_work, the insertions (agent, learner, row, size, position, group), whether an exact f == 0 met a populated dictionary)"""
    from ranslice.kbrl_dev import augmented_samples
    N, S = len(sizes), len(DIMS)
    learners, X, Y = [], [], []
    for e in range(N):
        Xe, Ye = augmented_samples(state[:, e], action[:, e], labels[:, e], DIMS, n_prbs)
        for s in range(S):
            learners.append((e, s))
            X.append(Xe[s])
            Y.append(Ye[s])
    rec = c.fit(learners, X, Y)
    want, insertions, tie = [0] * 8, [], False
    for e in range(N):
        br = [rec['branch'][e * S + s] for s in range(S)]
        for s in range(S):
            mb = np.concatenate([[sizes[e][s]], rec['m'][e * S + s][:-1]])
            tie = tie or bool((rec['f'][e * S + s][mb > 0] == 0.0).any())
        ins = []
        w = bm.expected_work(br, sizes[e], action[:, e], labels[:, e], width, max_landmarks, n_prbs=n_prbs, insertions=ins)
        want = [x + y for x, y in zip(want, w)]
        insertions += [(e,) + t for t in ins]
    return want, insertions, tie


def _twins_and_record(sizes, n_prbs, make_rows, width, max_landmarks, row_by_row=False):
    """line learners of `sizes`, their rows in ONE fit_steps call (or one call per row) at `width` beside width 0, and kb_fit on
    the augmented samples -> (counters per call, expected_work, insertions)"""
    grow, state, action, labels = _scenario(sizes, n_prbs, make_rows)
    N, R = len(sizes), len(state)
    a, b, c = (_handle(N, DIMS, n_prbs, w, max_landmarks) for w in (width, 0, 0))
    for h in (a, b, c):
        _pregrow(h, grow, sizes)
    st, ac, lb = _by_agent(state, action, labels)
    per_call = []
    for cut in ([slice(r, r + 1) for r in range(R)] if row_by_row else [slice(0, R)]):
        _same_call(a, b, list(range(N)), st[:, cut], ac[:, cut], lb[:, cut], everything=not row_by_row)
        per_call.append(a.fit_steps_batch_work())
        assert b.fit_steps_batch_work() == [0] * 8
    _same_everything(a, b)
    want, insertions, tie = _record(c, sizes, state, action, labels, n_prbs, width, max_landmarks)
    assert not tie                                        # (no draw separates the paths here: test 7 is the one with a tie)
    _same_dictionaries(a, c)
    assert a.stats() == c.stats()
    got = [sum(col) for col in zip(*per_call)]
    print('work', got, 'insertions (agent, learner, row, size, position, group):', insertions)
    assert got == want
    assert a.control_plus_batch_work() == [0] * 8         # (the control loop's counters are another setter's)
    for h in (a, b, c):
        h.close()
    return per_call, want, insertions


# ---------------------------------------------------------------------------------------------- 1. G19 as a log

@pytest.mark.parametrize('width,steps', [(8, 300), (2, 60), (4, 60)])
def test_g19_as_a_log(golden_dir, width, steps):
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    assert len(g['ties']) == 0
    a, b, c = (_handle(1, dims, n_prbs, w, g=g, seeds=np.zeros(1, dtype=np.uint64)) for w in (width, 0, 0))
    assert a.fit_steps_batch == (width, 1024, 128 + 5 * 2 * width * 1024 * 8) and b.fit_steps_batch == (0, 0, 0)
    _same_call(a, b, [0], [state[:steps]], [action[:steps]], [labels[:steps]])
    # the counters, from the recording alone: groups form per row on both surfaces
    counts = np.where(labels[:steps] == 1, n_prbs - action[:steps] + 1, action[:steps] + 1).sum(axis=0)
    br = [g['branch%d' % s][:counts[s]] for s in range(len(dims))]
    want = bm.expected_work(br, [0] * len(dims), action[:steps], labels[:steps], width, 1024, n_prbs=n_prbs)
    got = a.fit_steps_batch_work()
    print('width %d, %d rows: work %s' % (width, steps, got))
    assert got == want and got[2] > 0 and got[1] > 0 and got[5] > 0 and got[6] > 0
    assert b.fit_steps_batch_work() == [0] * 8
    assert int(a._repair_raw()[6]) == 0                   # kb_fit_steps counts no repair work, at either width
    # the same rows through the closed loop's update phase, one by one
    for i in range(steps):
        c.update_control(state[i][None], action[i][None], labels[i][None])
    _same_dictionaries(a, c)
    for h in (a, b, c):
        h.close()


# ---------------------------------------------------------------------------------------------- 2 - 4. hand-made learners and rows

def test_size_ladder():
    """learners of every size at which the walk, the tiles or the prefix store change their path, ten and three state variables;
    rows (control_plus_batch_rows.seam_rows, n_prbs = 41) with insertions at positions 0, 3 and 7: one call at width 8"""
    sizes = [[SIZES10[e], SIZES3[e]] for e in range(15)]
    _, work, ins = _twins_and_record(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, (0, 3, 7)[(e + s) % 3]), 8, 1024)
    seen = {(m, pos, g) for _, _, _, m, pos, g in ins}
    assert (0, -1, -1) in seen and (1, -1, -1) in seen          # one by one: the empty dictionary, 1 -> 2
    assert any(m == 1 for _, _, _, m, pos, g in ins) and work[6] > 0   # ... and the rest of that row was grouped
    assert any(m == 64 and pos >= 0 for m, pos, g in seen)      # 64 -> 65 inside a group: a new shell
    assert {pos for m, pos, g in seen if g == 8} >= {0, 3, 7}   # first, middle and last column of a full group
    assert any(m >= 256 and pos >= 0 for m, pos, g in seen)     # beyond the prefix store (KB_STEPS_PRE)


def test_group_edges():
    """n_prbs = 9, width 8: rows of 1, 7, 8, 9 and 10 candidates for both labels (control_plus_batch_rows.edge_rows) on learners of
    2, 4, 64 and 66 landmarks, one call per row so that the counters are per row: the repeated one-candidate row makes no pass"""
    sizes = [[2, 66], [66, 2], [4, 64]]
    where = set()

    def make(m, d, e, s):
        rows, again = rows_of.edge_rows(m, d)
        where.add(again)
        return rows
    per_row, work, ins = _twins_and_record(sizes, 9, make, 8, 1024, row_by_row=True)
    assert len(where) == 1 and len(per_row) == 11
    r = where.pop()
    assert per_row[r][2] == 0 and per_row[r][1] == 6 and per_row[r][0] == 6 and per_row[r][6] == 0
    assert all(row[2] > 0 for i, row in enumerate(per_row) if i != r)
    assert len(ins) == 10 * 6 and all(pos == 0 for _, _, _, _, pos, g in ins)
    assert {g for _, _, _, _, pos, g in ins} == {1, 7, 8}
    assert work[1] == 6 and work[6] == 0


def test_the_arenas_limit():
    """max_landmarks = 128: a learner of 128 landmarks is grouped until it inserts, one of 129 goes one by one, one of 127 grows to
    128 in its first row (still grouped) and past it inside its second"""
    sizes = [[127, 2], [128, 64], [129, 65]]
    _, work, ins = _twins_and_record(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, 3), 8, 128)
    by = {(e, s, t): (m, pos) for e, s, t, m, pos, g in ins}
    assert by[(0, 0, 0)] == (127, 0) and by[(0, 0, 1)] == (128, 3)
    assert by[(1, 0, 0)] == (128, 0) and by[(1, 0, 1)] == (129, -1)
    assert by[(2, 0, 0)] == (129, -1)
    assert work[6] > 0 and work[7] > 0 and work[2] > 0


# ---------------------------------------------------------------------------------------------- 5. what only a log has

def test_what_only_a_log_has():
    """five agents; listed: 3, 0, 1 and 4 (4 without rows), agent 2 is not.  Every learner's four rows stand in a log of eight: in
    row 2 r learner 1 skips (label 0), in row 2 r + 1 learner 0 does; learner 1 of agent 1 skips all eight.  Learners of one landmark
    open with a +1 row at their landmark's state (f_at in the float32 regime), the others meet seam_rows' +1 row from the midpoint
    as the first member of a group.  Width 8 at chunks 1, 2, 3 and the default against width 0 at the default chunk"""
    n_prbs = 41
    sizes = [[1, 3], [2, 64], [5, 2], [65, 1], [4, 4]]

    def make(m, d, e, s):
        rows = rows_of.seam_rows(m, d, n_prbs, 3)
        return [(rows_of.line_state(0, d), 5, 1)] + rows[:3] if m == 1 else rows
    grow, state, action, labels = _scenario(sizes, n_prbs, make)
    N, S, R = len(sizes), len(DIMS), len(state)
    off = np.concatenate([[0], np.cumsum(DIMS)])
    st = np.zeros((N, 2 * R, int(off[-1])), dtype=np.float32)
    ac, lb = np.zeros((N, 2 * R, S), dtype=np.int64), np.zeros((N, 2 * R, S), dtype=np.int64)
    for s in range(S):
        st[:, s::2, off[s]:off[s + 1]] = state.transpose(1, 0, 2)[:, :, off[s]:off[s + 1]]
        ac[:, s::2, s] = action.transpose(1, 0, 2)[:, :, s]
        lb[:, s::2, s] = labels.transpose(1, 0, 2)[:, :, s]
    lb[1, :, 1] = 0
    ac[lb == 0] = -7                                            # (an action is not looked at where the label is 0)
    listed = [3, 0, 1, 4]
    log = ([st[e] if e != 4 else st[e][:0] for e in listed], [ac[e] if e != 4 else ac[e][:0] for e in listed],
           [lb[e] if e != 4 else lb[e][:0] for e in listed])
    b = _handle(N, DIMS, n_prbs, 0)
    _pregrow(b, grow, sizes)
    ref = None
    for chunk in (1, 2, 3, 0):
        a = _handle(N, DIMS, n_prbs, 8)
        _pregrow(a, grow, sizes)
        before = {(e, s): a.learner(e, s, with_kinv=True) for e, s in ((1, 1), (2, 0), (2, 1), (4, 0), (4, 1))}
        stats0 = a.stats()
        if ref is None:
            out = ref = _same_call(a, b, listed, *log, chunk_a=chunk)
        else:                                                   # (b has been taught: the later chunks against the first one's results)
            out = a.fit_steps(listed, *log, chunk=chunk)
            for k in SUMMARIES:
                assert all(x.tobytes() == y.tobytes() for x, y in zip(out[k], ref[k])), (chunk, k)
            _same_everything(a, b)
        work = a.fit_steps_batch_work()
        print('chunk %d: work %s' % (chunk, work))
        assert work[2] > 0 and work[6] > 0
        # the learner all of whose rows are 0, the agent without rows and the agent not listed: not touched at all
        for (e, s), was in before.items():
            _same_learner(a.learner(e, s, with_kinv=True), was, (e, s))
        assert a.stats()[0] > stats0[0]
        # skipped entries report 0, 0, 0, 0 and the current size
        assert all((out[k][2][:, 1] == 0).all() for k in ('f_at', 'y_at', 'changed', 'grown')) and (out['m'][2][:, 1] == 64).all()
        assert out['m'][3].shape == (0, S)
        a.close()
    # f_at of a +1 row: at m == 1 (one by one, float32) and at m >= 2 (the first member of a group), nonzero and the twin's
    seen = set()
    for i, e in enumerate(listed[:3]):
        for s in range(S):
            m_before = np.concatenate([[sizes[e][s]], ref['m'][i][:-1, s]])
            for r in np.nonzero(lb[e][:, s] == 1)[0]:
                assert ref['f_at'][i][r, s] != 0.0 and ref['y_at'][i][r, s] != 0
                seen.add(min(int(m_before[r]), 2))
    assert seen == {1, 2}
    b.close()


# ---------------------------------------------------------------------------------------------- 6. more learners than arenas

def test_more_learners_than_arenas():
    """520 agents x 2 slices = 1,040 learners for 1,024 arenas, n_prbs = 9: four fresh rows each from the empty dictionary (the
    first two insert one by one, the rest is grouped and every learner makes a pass), then two more in a second call, which finds
    the ticket back at zero"""
    N, n_prbs, S = 520, 9, len(DIMS)
    a, b = (_handle(N, DIMS, n_prbs, w, 64, capacity=64) for w in (8, 0))
    assert a.fit_steps_batch == (8, 64, 128 + 1024 * 2 * 8 * 64 * 8)
    off = np.concatenate([[0], np.cumsum(DIMS)])

    def rows(i0, i1):
        st = np.zeros((N, i1 - i0, int(off[-1])), dtype=np.float32)
        ac, lb = np.zeros((N, i1 - i0, S), dtype=np.int64), np.zeros((N, i1 - i0, S), dtype=np.int64)
        for s, d in enumerate(DIMS):
            for i in range(i0, i1):
                x, act, lab = rows_of.fresh_row(i, d, n_prbs, rows_of.last_sign(i), 2)
                st[:, i - i0, off[s]:off[s + 1]], ac[:, i - i0, s], lb[:, i - i0, s] = x, act, lab
        return st, ac, lb
    out = _same_call(a, b, list(range(N)), *rows(0, 4), everything=False)
    work = a.fit_steps_batch_work()
    print('1,040 learners, four rows: work', work)
    assert all((m[-1] >= 2).all() for m in out['m'])
    assert work[2] >= N * S and work[6] > 0
    out = _same_call(a, b, list(range(N)), *rows(4, 6), everything=False)
    work = a.fit_steps_batch_work()
    print('two more rows: work', work)
    assert work[2] >= N * S and work[6] == 0 and all((m[-1] == 6).all() for m in out['m'])
    _same_everything(a, b)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 7. a tie inside a group

def test_a_tie_inside_a_row():
    """n_prbs = 10, line learners of exactly two landmarks (+1 at allocation 0, -1 at allocation 1, 3.5 away from the midpoint on
    either side), the midpoint row labelled +1 from allocation 0: at a = 5 the two kernel values are the same double and f = k - k
    is exactly 0 against a populated dictionary, so fit_decide draws from the learner's stream -- as a member of a group.  The
    record of kb_fit on the augmented samples must show that f; the twins, reset with equal seeds, must agree in every byte, the
    stream's position included"""
    n_prbs, sizes = 10, [[2, 2]]
    grow, state, action, labels = _scenario(sizes, n_prbs, lambda m, d, e, s: [(rows_of.line_state(0.5, d), 0, 1)])
    seeds = np.array([11], dtype=np.uint64)
    a, b, c = (_handle(1, DIMS, n_prbs, w, seeds=seeds) for w in (8, 0, 0))
    for h in (a, b, c):
        _pregrow(h, grow, sizes)
    _same_call(a, b, [0], *_by_agent(state, action, labels))
    work = a.fit_steps_batch_work()
    print('work', work)
    assert work[0] > 0 and work[2] > 0 and work[6] == 0         # every candidate was a member of a group
    from ranslice.kbrl_dev import augmented_samples
    X, Y = augmented_samples(state[:, 0], action[:, 0], labels[:, 0], DIMS, n_prbs)
    rec = c.fit([(0, 0), (0, 1)], X, Y)
    for i in range(2):
        print('learner %d: f %s branch %s' % (i, rec['f'][i].tolist(), rec['branch'][i].tolist()))
        assert rec['f'][i][5] == 0.0 and (rec['m'][i][:5] == 2).all(), i     # an exact 0 at a = 5, against two landmarks
    _same_everything(a, c)
    # the draw moved the stream of all three alike: the counters as an agent file carries them, and the next draws
    from ranslice import agent_file as af
    ctr = [af.unpack(h.export_agents(np.arange(1)))['agents'][0]['tie_ctr'].tolist() for h in (a, b, c)]
    print('tie counters', ctr)
    assert ctr[0] == ctr[1] == ctr[2] and all(v > 0 for v in ctr[0])
    for s, d in enumerate(DIMS):
        far = np.array([7e4] * (d + 1))
        draws = [tuple(h.predict(0, s, far) for h in (a, b, c)) for _ in range(6)]
        assert all(u == v == w and u[1] == 0.0 and u[0] in (1, -1) for u, v, w in draws), draws
    for h in (a, b, c):
        h.close()


# ---------------------------------------------------------------------------------------------- 8. the switch

def _short_log(dims, n_prbs, rows=3):
    rng = np.random.default_rng(5)
    st = rng.random((2, rows, int(sum(dims)))).astype(np.float32)
    ac = rng.integers(1, n_prbs, (2, rows, len(dims)))
    lb = rng.choice([-1, 1], (2, rows, len(dims)))
    return st, ac, lb


def test_the_switch():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL
    cfg = make_config(1, n_envs=2)
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    T = 2 * len(dims)
    ag = _handle(2, dims, cfg.n_prbs, capacity=512)
    assert ag.fit_steps_batch == (0, 0, 0) and ag.fit_steps_batch_work() == [0] * 8
    ag.fit_steps([0, 1], *_short_log(dims, cfg.n_prbs))          # (something to deploy)
    for w in (1, 3, 16, 5, -2):
        assert ag.L.kb_set_fit_steps_batch(ag.h, w, 128) == _lib.RS_EINVAL, w
        assert '2, 4 or 8' in ag.L.kb_last_error(ag.h).decode()
    for mx in (0, 63, 512 + 64, 100, -64):
        assert ag.L.kb_set_fit_steps_batch(ag.h, 8, mx) == _lib.RS_EINVAL, mx
        assert 'multiple of 64' in ag.L.kb_last_error(ag.h).decode()
    assert ag.fit_steps_batch == (0, 0, 0)
    assert ag.L.kb_set_fit_steps_batch(ag.h, 0, 100) == _lib.RS_OK            # ignored while the width is 0
    for w, mx in ((8, 512), (2, 64), (4, 128)):
        ag.set_fit_steps_batch(w, mx)
        assert ag.fit_steps_batch == (w, mx, 128 + min(T, 1024) * 2 * w * mx * 8)
        assert ag.fit_steps_batch_work() == [0] * 8
        assert ag.control_plus_batch == (0, 0, 0)                             # the other setter's report is its own
    ag.set_control_plus_batch(2, 64)
    assert ag.fit_steps_batch == (4, 128, 128 + T * 2 * 4 * 128 * 8) and ag.control_plus_batch == (2, 64, 128 + T * 2 * 2 * 64 * 8)
    ag.set_fit_steps_batch(0)
    assert ag.fit_steps_batch == (0, 0, 0) and ag.fit_steps_batch_work() == [0] * 8
    assert ag.control_plus_batch == (2, 64, 128 + T * 2 * 2 * 64 * 8)
    ag.set_control_plus_batch(0)
    # handles on which nothing learns through fit_steps
    for h, word in ((ag.deploy([0, 1]), 'inference-only'), (ag.deploy([1, 1, 0], by_reference=True), 'by-reference')):
        with pytest.raises(_lib.RanSliceError) as e:
            h.set_fit_steps_batch(8, 64)
        assert e.value.code == _lib.RS_ESTATE and word in str(e.value) and 'does not learn through kb_fit_steps' in str(e.value)
        h.close()
    sh = SharedVecKBRL(2, dims, cfg.n_prbs, capacity=128, pool_bytes=64 << 20)
    assert sh.L.kb_set_fit_steps_batch(sh.h, 8, 64) == _lib.RS_ESTATE and 'shared' in sh.L.kb_last_error(sh.h).decode()
    sh.close()
    ag.close()


def test_the_switch_leaves_projectron_alone_and_toggles(golden_dir):
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    z = np.zeros(1, dtype=np.uint64)
    # Projectron mode: width 8 set, bytes of a handle that never set it, and the info reads zeros
    a, b = (_handle(1, dims, n_prbs, w, g=g, seeds=z, algorithm='projectron') for w in (8, 0))
    assert a.fit_steps_batch[0] == 8
    _same_call(a, b, [0], [state[:40]], [action[:40]], [labels[:40]])
    assert a.fit_steps_batch_work() == [0] * 8 and a.dictionary_sizes().max() >= 2
    a.close()
    b.close()
    # Projectron++ mode: 8 -> 0 -> 4 between calls, beside a handle at 0 throughout
    a, b = (_handle(1, dims, n_prbs, w, g=g, seeds=z) for w in (8, 0))
    for i, w in enumerate((8, 0, 4)):
        a.set_fit_steps_batch(w)
        cut = slice(30 * i, 30 * i + 30)
        _same_call(a, b, [0], [state[cut]], [action[cut]], [labels[cut]])
        work = a.fit_steps_batch_work()
        assert (work[0] > 0) == (w > 0) and (w == 0) == (work == [0] * 8), (w, work)
    a.close()
    b.close()
