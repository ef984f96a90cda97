"""The closed loop's Projectron++ update phase with the large learners' passes over Kinv spread over the chip
(kb_set_control_plus_wide): whatever min_landmarks, max_landmarks and rounds, the bytes are those of the same
batch width with the switch off.  Every case runs a wide handle beside a twin of the same width.

1. G19 teacher-forced at width 8, 100 steps at (min 2, rounds 1) and (min 2, rounds 32), 160 at (min 64, rounds 4): every step's hits,
   actions, adjusted, margins, security factors and sizes; at the end all bytes, the statistics, kb_get_repair_work and the eight
   batch counters (the twin's, and expected_work of the recording); kb_control_plus_wide_info shows what the rounds did.
2. The size ladder (tests/control_plus_batch_rows.py): learners of 2 .. 320 landmarks, insertions at the first, a middle and the
   last column of a group, 64 -> 65 inside a row; widths 2 and 8; against width 0 too.
3. Group edges (n_prbs = 9).  4. rounds = 1, 2 and 256.  5. The bounds: min_landmarks above every size; max_landmarks = 128;
the batch setting's max_landmarks and this one's apart, in both directions.
6. More heavy learners (1,030) than slots (1,024).  7. An exact f == 0 tie inside a spread group.  8. The resident paths, plain and
captured, the switch toggled between stretches.  9. A checkpoint.  10. The setter.  11. A Projectron handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from ranslice.config import make_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import control_plus_batch_mirror as bm   # noqa: E402
import control_plus_batch_rows as rows_of   # noqa: E402
from test_gpu_control_plus import _load   # noqa: E402
from test_gpu_control_plus_batch import DIMS, POOL, _handle, _loop, _pregrow, _same_everything, _same_loops, _scenario   # noqa: E402

pytestmark = pytest.mark.gpu
SLOTS, REC, HEAD = 1024, 256, 128


def _scratch(T, max_landmarks):
    slots = min(T, SLOTS)
    return HEAD + slots * REC + 2 * (slots + 1) * 8 + 8 * ((T + 1) // 2) + slots * 2 * 8 * max_landmarks * 8


# ---------------------------------------------------------------------------------------------- 1. G19, teacher-forced

@pytest.mark.parametrize('min_m,rounds,steps', [(2, 1, 100), (2, 32, 100), (64, 4, 160)])
def test_g19_teacher_forced_beside_the_width_alone(golden_dir, min_m, rounds, steps):
    """(the recording's largest learner holds 51 landmarks after 100 steps and reaches 64 at step 128: the run at min 64 goes on to
    step 160, so that it becomes heavy, and inserts as a heavy learner, inside the run)"""
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    width = 8
    assert len(g['ties']) == 0
    a = _handle(1, dims, n_prbs, width, g=g, seeds=np.zeros(1, dtype=np.uint64), control_plus_wide=min_m, control_plus_wide_max=1024,
                control_plus_wide_rounds=rounds)
    b = _handle(1, dims, n_prbs, width, g=g, seeds=np.zeros(1, dtype=np.uint64))
    assert a.control_plus_wide == (min_m, 1024, rounds, _scratch(len(dims), 1024)) and b.control_plus_wide == (0, 0, 0, 0)
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
    counts = np.where(labels[:steps] == 1, n_prbs - action[:steps] + 1, action[:steps] + 1).sum(axis=0)
    br = [g['branch%d' % s][:counts[s]] for s in range(len(dims))]
    want = bm.expected_work(br, [0] * len(dims), action[:steps], labels[:steps], width, 1024, n_prbs=n_prbs)
    got, info = a.control_plus_batch_work(), a.control_plus_wide_work()
    print('min %d, rounds %d: sizes %s, batch work %s, wide work %s' % (min_m, rounds, a.dictionary_sizes()[0].tolist(), got, info))
    assert got == want == b.control_plus_batch_work()
    # (a learner that begins a row below min_landmarks walks it on the batch kernel's row, so the rounds' passes and tiles are
    # part of the batch counters', all of them once every learner is heavy and no row reaches the finisher)
    assert info[7] == steps and info[0] > 0 and info[1] == 0 and 0 < info[2] <= got[2] and info[2] <= info[3] <= got[3] and info[4] > 0
    assert info[3] == info[2] or a.dictionary_sizes().max() > 64       # one tile per pass while every heavy dictionary fits one
    if rounds == 1:
        assert info[5] > 0 and info[6] >= info[5]
    assert b.control_plus_wide_work() == [0] * 8
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 2 - 7. hand-made learners and rows

def _tiles(m):
    nb = (m + 63) // 64
    return nb * (nb + 1) // 2


def _all_in_the_rounds(info, work, units):
    """every learner heavy from its row's start and no row left to the finisher: the rounds made every pass of the batch counters,
    read their tiles, and spread the rank-1 units of every insertion"""
    assert info[5] == 0 and info[6] == 0
    assert info[2] == work[2] and info[3] == work[3] and info[4] == units


def _twins(sizes, n_prbs, make_rows, width, wide, max_landmarks=1024, with_zero=False, seeds=None, keep=False):
    """the rows on a wide handle (wide = (min_landmarks, max_landmarks, rounds)), a twin of the same width and, with_zero, one of
    width 0: equal hits row by row, equal bytes, equal batch counters -> (kb_control_plus_wide_info, the batch counters, handles)"""
    grow, state, action, labels = _scenario(sizes, n_prbs, make_rows)
    N = len(sizes)
    hs = [_handle(N, DIMS, n_prbs, w, max_landmarks, seeds=seeds) for w in ((width, width, 0) if with_zero else (width, width))]
    hs[0].set_control_plus_wide(*wide)
    assert hs[0].control_plus_wide == tuple(wide) + (_scratch(N * len(DIMS), wide[1]),)
    for h in hs:
        _pregrow(h, grow, sizes)
    units = 0      # the rank-1 units of every insertion of the rows: 4 per tile of the grown triangle, n_b (n_b + 1) / 2 tiles
    for r in range(len(state)):
        before = hs[1].dictionary_sizes().copy()
        hits = [h.update_control(state[r], action[r], labels[r]) for h in hs]
        assert all(np.array_equal(hits[0], x) for x in hits[1:]), r
        for m0, m1 in zip(before.ravel(), hs[1].dictionary_sizes().ravel()):
            units += sum(_tiles(j + 1) * 4 for j in range(int(m0), int(m1)))
    for h in hs[1:]:
        _same_everything(hs[0], h)
    info, work = hs[0].control_plus_wide_work(), hs[0].control_plus_batch_work()
    assert work == hs[1].control_plus_batch_work()
    assert info[7] == len(state) and hs[1].control_plus_wide_work() == [0] * 8
    print('wide', wide, 'width', width, 'wide work', info, 'batch work', work)
    if keep:
        return info, work, units, hs
    for h in hs:
        h.close()
    return info, work, units


LADDER10 = [2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 320]
LADDER3 = [64, 2, 65, 3, 66, 2, 64, 65, 2, 3, 66, 5, 2]


@pytest.mark.parametrize('width', [8, 2])
def test_size_ladder(width):
    """learners of every size at which the pass, the tiles or the prefix store change their path; rows that insert their first
    candidate (64 -> 65: a new shell and a new output block inside a row) and, at the midpoint rows, the first, a middle and the
    last column of a group further into the row; all of them heavy (min 2), 32 rounds; against the width alone and width 0"""
    sizes = [[LADDER10[e], LADDER3[e]] for e in range(len(LADDER10))]
    pos = (0, 3, 7) if width == 8 else (0, 1, 3)
    info, work, units = _twins(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, pos[(e + s) % 3]), width, (2, 1024, 32), with_zero=True)
    T = 2 * len(sizes)
    _all_in_the_rounds(info, work, units)
    assert info[0] == 4 * T and info[1] == 0 and info[2] > 0 and info[4] > 0 and info[5] == 0 and work[5] > 0 and work[6] == 0


def test_group_edges():
    """n_prbs = 9, width 8: rows of 1, 7, 8, 9 and 10 candidates for both labels, and the row whose one group is skipped"""
    sizes = [[2, 66], [66, 2], [4, 64]]
    info, work, units = _twins(sizes, 9, lambda m, d, e, s: rows_of.edge_rows(m, d)[0], 8, (2, 1024, 32), with_zero=True)
    _all_in_the_rounds(info, work, units)
    assert info[0] == 11 * 6 and info[2] > 0 and info[5] == 0 and work[1] == 6 and work[6] == 0


def test_rounds_do_not_change_a_byte():
    """the same rows at 1, 2 and 256 rounds: each equal to the width alone, hence to each other; what one round leaves open reaches
    the finisher, 256 rounds leave nothing"""
    sizes = [[2, 64], [65, 3], [128, 2], [193, 66]]
    infos = {r: _twins(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, (0, 3, 7)[(e + s) % 3]), 8, (2, 1024, r)) for r in (1, 2, 256)}
    works = [infos[r][1] for r in (1, 2, 256)]
    _all_in_the_rounds(*infos[256])
    assert infos[1][0][4] <= infos[2][0][4] <= infos[256][0][4] == infos[256][2]      # (the finisher's insertions are not spread)
    assert works[0] == works[1] == works[2]
    assert infos[1][0][5] > 0 and infos[1][0][6] > 0 and infos[256][0][5] == 0 and infos[256][0][6] == 0
    assert infos[1][0][0] == infos[2][0][0] == infos[256][0][0] == 4 * 8


def test_bounds():
    """min_landmarks above every size: nobody is listed.  max_landmarks = 128 (the twin's arena holds 128 as well): a learner of
    129 stays on the batch kernel's row, one by one; those of 127 and 128 are heavy, and the one whose row takes it to 129 is left
    to the finisher, one by one there"""
    sizes = [[127, 2], [128, 64], [129, 65]]
    make = lambda m, d, e, s: rows_of.seam_rows(m, d, 41, 3)   # noqa: E731
    info, work, _ = _twins(sizes, 41, make, 8, (512, 1024, 8))
    assert info[:7] == [0] * 7
    info, work, _ = _twins(sizes, 41, make, 8, (2, 128, 8), max_landmarks=128, with_zero=True)
    # per row: learner (2, 0) is never listed; (0, 0) holds 129 from its second row's insertion on, (1, 0) from its first row's
    assert info[0] == HEAVY_ROWS_128 and info[5] > 0 and info[6] > 0 and work[6] > 0 and work[7] > 0 and work[2] > 0


HEAVY_ROWS_128 = 4 * 6 - 4 - 2 - 3


def test_the_two_maxima_apart():
    """the rounds take and keep a learner up to the SMALLER of kb_set_control_plus_batch's and kb_set_control_plus_wide's
    max_landmarks, and the finisher groups by the batch setting's alone: with the maxima apart in either direction every learner is
    grouped or taken one by one where the twin of the same width does it, so all eight batch counters are the twin's (_twins asserts
    it).  The learners of test_bounds.  Batch 1,024, wide 128: the twin groups everybody; the learner of 129 is not listed and is
    grouped on the batch kernel's row, the one an insertion takes to 129 goes to the finisher and is grouped there -- nobody goes
    one by one.  Batch 128, wide 1,024: the limit is 128 again, and 129 landmarks go one by one on either handle"""
    sizes = [[127, 2], [128, 64], [129, 65]]
    make = lambda m, d, e, s: rows_of.seam_rows(m, d, 41, 3)   # noqa: E731
    info, work, _ = _twins(sizes, 41, make, 8, (2, 128, 8), max_landmarks=1024, with_zero=True)
    assert info[0] == HEAVY_ROWS_128 and info[5] > 0 and info[6] > 0 and work[6] == 0 and work[7] == 0 and work[2] > 0
    wide_small = work
    info, work, _ = _twins(sizes, 41, make, 8, (2, 1024, 8), max_landmarks=128, with_zero=True)
    assert info[0] == HEAVY_ROWS_128 and info[5] > 0 and info[6] > 0 and work[6] > 0 and work[7] > 0 and work[2] > 0
    assert wide_small[4] > work[4]          # (what goes one by one here was a column of a group there)


def test_more_heavy_learners_than_slots():
    """1,030 learners of two landmarks, min 2: the first 1,024 in task order take the slots, six are turned away to the batch
    kernel's row; equal bytes"""
    N = 515
    sizes = [[2, 2]] * N
    info, work, _ = _twins(sizes, 41, lambda m, d, e, s: rows_of.seam_rows(m, d, 41, 3)[:2], 8, (2, 64, 4), max_landmarks=64)
    assert info[0] == 2 * 1024 and info[1] == 2 * 6 and info[2] > 0


def test_a_tie_inside_a_spread_group():
    """n_prbs = 10, line learners of exactly two landmarks, the midpoint row labelled +1 from allocation 0: at a = 5 f = k - k is
    exactly 0 against a populated dictionary and fit_decide draws from the learner's stream -- as a member of a group whose d* a
    spread pass formed.  The twins, reset with equal seeds, agree in every byte, the stream's position included"""
    from ranslice import agent_file as af
    n_prbs, sizes = 10, [[2, 2]]
    info, work, units, hs = _twins(sizes, n_prbs, lambda m, d, e, s: [(rows_of.line_state(0.5, d), 0, 1)], 8, (2, 1024, 32), with_zero=True,
                            seeds=np.array([11], dtype=np.uint64), keep=True)
    assert info[0] == 2 and info[2] >= 2 and work[6] == 0
    _all_in_the_rounds(info, work, units)
    ctr = [af.unpack(h.export_agents(np.arange(1)))['agents'][0]['tie_ctr'].tolist() for h in hs]
    print('tie counters', ctr)
    assert ctr[0] == ctr[1] == ctr[2] and all(v > 0 for v in ctr[0])
    for s, d in enumerate(DIMS):
        far = np.array([7e4] * (d + 1))
        draws = [tuple(h.predict(0, s, far) for h in hs) for _ in range(6)]
        assert all(u == v == w and u[1] == 0.0 and u[0] in (1, -1) for u, v, w in draws), draws
    for h in hs:
        h.close()


# ---------------------------------------------------------------------------------------------- 8. the resident paths

def _wide_loop(golden_dir, graph, settings, steps_each, N=24):
    """test_gpu_control_plus_batch._loop with width 8 and the wide switch set in front of each stretch: settings = [(min_landmarks,
    rounds), ..], min_landmarks 0 = off"""
    from ranslice.kbrl_dev import VecKBRL
    from ranslice.vec_env import VecRanSlice
    gf = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    cfg = make_config(1, n_envs=N)
    dims, n_prbs = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs
    rng = np.random.default_rng(31)
    ia = np.stack([np.concatenate([rng.integers(4, 20, cfg.n_embb), rng.integers(2, 10, cfg.n_mmtc)]) for _ in range(N)]).astype(np.int32)
    sf = np.stack([np.concatenate([rng.integers(2, 8, cfg.n_embb), rng.integers(1, 4, cfg.n_mmtc)]) for _ in range(N)]).astype(np.int32)
    env = VecRanSlice(n_envs=N, cfg=cfg, fading=[gf['t0'], gf['t1'], gf['t2']], seed=19)
    ag = VecKBRL(N, dims, n_prbs, capacity=256, pool_bytes=POOL, algorithm='projectron_plus', control_plus=True, control_plus_batch=8,
                 control_plus_batch_max=256)
    ag.reset(ia, sf, seeds=np.arange(N, dtype=np.uint64) + 4)
    env.reset()
    ag.history_begin(steps_each * len(settings))
    env._check(env.L.rs_step(env.h, ia.ctypes.data_as(C.POINTER(C.c_int32)), None, None, None, None))
    for min_m, rounds in settings:
        ag.set_control_plus_wide(min_m, 256, rounds)
        ag.run_resident(env, steps_each, graph=graph)
    hist = ag.history_fetch()
    assert hist['recorded'] == steps_each * len(settings)
    out = ([ag.learner(r, s, with_kinv=True) for r in range(N) for s in range(len(dims))], ag.control(), hist, ag.dictionary_sizes().copy(),
           env.fetch()['obs'].copy(), ag.control_plus_batch_work(), ag.control_plus_wide_work())
    env.close()
    ag.close()
    return out


def test_resident_paths(golden_dir):
    """24 replicas, 10 steps of kb_run_resident, plain and captured, the switch toggled between stretches (which retires the graph):
    dictionaries, control state, rewards and the other histories as bytes, against the width-only loop"""
    ref = _loop(golden_dir, False, [8], 10)
    assert ref[3].max() > 2
    for graph, settings, each in ((False, [(2, 4)], 10), (True, [(2, 4)], 10), (True, [(2, 1), (0, 0)], 5), (True, [(0, 0), (2, 32)], 5),
                                  (False, [(2, 2), (0, 0), (3, 8), (2, 1), (0, 0)], 2)):
        got = _wide_loop(golden_dir, graph, settings, each)
        _same_loops(got, ref)
        print(graph, settings, 'wide work', got[6])
        if settings[-1][0]:
            assert got[6][0] > 0 and got[6][2] > 0 and got[6][7] > 0, (graph, settings, got[6])
            if len(settings) == 1:
                assert got[5] == ref[5] and got[6][7] == each


# ---------------------------------------------------------------------------------------------- 9. a checkpoint

def test_checkpoint_taken_with_the_switch_on_continues_with_it_off(golden_dir):
    g, dims, n_prbs, (state, action, labels) = _load(golden_dir, 'g19_control_plus')
    a = _handle(1, dims, n_prbs, 8, g=g, seeds=np.zeros(1, dtype=np.uint64), control_plus_wide=2, control_plus_wide_max=1024)
    b = _handle(1, dims, n_prbs, 8, g=g, seeds=np.zeros(1, dtype=np.uint64))
    P = 45
    for i in range(P):
        a.update_control(state[i][None], action[i][None], labels[i][None])
        a.select_action(state[i + 1][None])
    assert a.dictionary_sizes().max() >= 2 and a.control_plus_wide_work()[2] > 0
    b.load_state(a.save_state())
    assert b.control_plus_wide == (0, 0, 0, 0) and a.control_plus_wide[:3] == (2, 1024, 32)      # the switch is not in the blob
    for i in range(P, P + 5):
        for h in (a, b):
            h.update_control(state[i][None], action[i][None], labels[i][None])
            h.select_action(state[i + 1][None])
    _same_everything(a, b)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------- 10. the setter

def test_the_setter():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL
    cfg = make_config(1, n_envs=2)
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    T = 2 * len(dims)
    ag = _handle(2, dims, cfg.n_prbs, capacity=512)
    assert ag.control_plus_wide == (0, 0, 0, 0) and ag.control_plus_wide_work() == [0] * 8
    ag.update_control(np.zeros((2, ag.nv)), np.full((2, len(dims)), 3), np.ones((2, len(dims))))     # (something to deploy)
    for mn, mx, r in ((1, 128, 4), (-2, 128, 4), (129, 128, 4), (2, 100, 4), (2, 0, 4), (2, 32, 4), (2, 576, 4), (2, 1024, 4), (2, -64, 4),
                      (2, 128, 0), (2, 128, 257), (2, 128, -1)):
        assert ag.L.kb_set_control_plus_wide(ag.h, mn, mx, r) == _lib.RS_EINVAL, (mn, mx, r)
        assert 'kb_set_control_plus_wide' in ag.L.kb_last_error(ag.h).decode()
    assert ag.control_plus_wide == (0, 0, 0, 0)
    assert ag.L.kb_set_control_plus_wide(ag.h, 0, 100, 999) == _lib.RS_OK              # ignored while min_landmarks is 0
    for mn, mx, r in ((2, 512, 32), (64, 64, 1), (100, 128, 256)):     # (without a batch width it is kept, and has no effect)
        ag.set_control_plus_wide(mn, mx, r)
        assert ag.control_plus_wide == (mn, mx, r, _scratch(T, mx))
        assert ag.control_plus_wide_work() == [0] * 8
    ag.update_control(np.zeros((2, ag.nv)), np.full((2, len(dims)), 3), np.ones((2, len(dims))))
    assert ag.control_plus_wide_work() == [0] * 8                       # width 0: control_plus_kernel's launch
    ag.set_control_plus_wide(0)
    assert ag.control_plus_wide == (0, 0, 0, 0)
    for h, word in ((ag.deploy([0, 1]), 'inference-only'), (ag.deploy([1, 1, 0], by_reference=True), 'by-reference')):
        with pytest.raises(_lib.RanSliceError) as e:
            h.set_control_plus_wide(2, 64, 4)
        assert e.value.code == _lib.RS_ESTATE and word in str(e.value) and 'does not learn through kb_update_control' in str(e.value)
        h.close()
    sh = SharedVecKBRL(2, dims, cfg.n_prbs, capacity=128, pool_bytes=64 << 20)
    assert sh.L.kb_set_control_plus_wide(sh.h, 2, 64, 4) == _lib.RS_ESTATE and 'shared' in sh.L.kb_last_error(sh.h).decode()
    with pytest.raises(_lib.RanSliceError) as e:
        sh.set_control_plus_wide(2, 64, 4)
    assert e.value.code == _lib.RS_ESTATE
    sh.close()
    ag.close()


# ---------------------------------------------------------------------------------------------- 11. Projectron

def test_the_switch_leaves_projectron_alone(golden_dir):
    """the switch (and width 8, and control_plus) on a Projectron handle: 5 resident steps equal, as bytes, to a handle that never set it"""
    from test_gpu_control_plus import _closed_loop, _same_runs
    full = ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation')

    def switch(ag):
        ag.set_control_plus_batch(8, 256)
        ag.set_control_plus_wide(2, 256, 4)
    for mode in ('run', 'graph'):
        ref = _closed_loop(golden_dir, mode, 5, algorithm='projectron', control_plus=False)
        got = _closed_loop(golden_dir, mode, 5, algorithm='projectron', control_plus=True, switch=switch)
        _same_runs(got, ref, full)
        assert got[0]['obs'].tobytes() == ref[0]['obs'].tobytes()
