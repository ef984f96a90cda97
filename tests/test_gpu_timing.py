"""The accounting of the kernel timing (rs_set_kernel_timing, kb_set_kernel_timing): which launches get an event pair, how the
pairs are counted per kind, and that reading them starts the count over.  Counts and ordering only -- a duration is never held
against a threshold, only against zero and against the other durations of the same report."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_prune import _random_stream   # noqa: E402
from ranslice.config import make_config   # noqa: E402

pytestmark = pytest.mark.gpu

N = 8


@pytest.fixture(scope='module')
def fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


def _even_actions(env):
    return np.full((N, env.n_slices), env.n_prbs // (env.n_slices + 1), dtype=np.int32)


def _expect_spans(env, launches):
    """`launches` pairs with 0 < min <= mean <= max, and nothing left behind for the next reader"""
    (mean, mn, mx), n = env.kernel_time_stats_ms()
    print('launches %d: mean %.4f min %.4f max %.4f ms' % (n, mean, mn, mx))
    assert n == launches
    if launches:
        assert 0.0 < mn <= mean <= mx
    else:
        assert (mean, mn, mx) == (0.0, 0.0, 0.0)
    assert env.kernel_time_ms() == (0.0, 0)


@pytest.mark.parametrize('mux', [False, True])
def test_simulator_counts_one_pair_per_step(fading, mux):
    """scenario 0, per-slice and multiplexed L1: three rs_step give three pairs; four steps of rs_run_random with use_graph are
    enqueued one by one while timing is on, so four pairs; switching the timing on again in the middle of a run discards the
    pairs taken so far"""
    from ranslice.vec_env import VecRanSlice
    cfg = make_config(0, n_envs=N, L1_level=False) if mux else make_config(0, n_envs=N)
    env = VecRanSlice(n_envs=N, cfg=cfg, fading=fading, seed=3)
    assert env.multiplexed == mux
    env.reset()
    acts = _even_actions(env)
    env.step(acts)                       # untimed: no pair
    env.set_kernel_timing(True)
    for _ in range(3):
        env.step(acts)
    _expect_spans(env, 3)
    env.run_random(11, 0, 4, graph=True)
    _expect_spans(env, 4)
    env.step(acts)
    env.step(acts)
    env.set_kernel_timing(True)          # (again: the two pairs are dropped)
    env.step(acts)
    _expect_spans(env, 1)
    env.set_kernel_timing(False)
    env.step(acts)
    _expect_spans(env, 0)
    env.close()


def test_simulator_without_embb_tasks_takes_no_pair():
    """mMTC slices only: the pair brackets the eMBB step launches, and there are none"""
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=N, cfg=make_config(None, n_envs=N, n_prbs=256, n_embb=0, n_mmtc=2), fading=None, seed=1)
    env.reset()
    env.set_kernel_timing(True)
    for _ in range(3):
        env.step(np.full((N, 2), 5, dtype=np.int32))
    _expect_spans(env, 0)
    env.close()


def _agent(fading):
    from ranslice.kbrl_dev import VecKBRL
    cfg0 = make_config(0)
    dims = [10] * cfg0.n_embb + [3] * cfg0.n_mmtc
    ag = VecKBRL(N, dims, cfg0.n_prbs, capacity=1024, pool_bytes=256 << 20)
    ia = np.tile(np.array([10 if d == 10 else 5 for d in dims], dtype=np.int32), (N, 1))
    sf = np.tile(np.array([3 if d == 10 else 2 for d in dims], dtype=np.int32), (N, 1))
    ag.reset(ia, sf, seeds=np.arange(N, dtype=np.uint64) + 5)
    return ag, ia


def _drive(ag, rng, steps):
    for _ in range(steps):
        st = rng.random((N, ag.nv)).astype(np.float32)
        act = rng.integers(0, ag.n_prbs + 1, size=(N, ag.S)).astype(np.int32)
        lab = rng.choice([-1, 1], size=(N, ag.S)).astype(np.int32)
        ag.update_control(st, act, lab)
        ag.select_action(st)


PER_LAUNCH = (('update_small_launch_ms', 'n_update_small'), ('select_bin_launch_ms', 'n_select_bin'),
              ('select_gemm_launch_ms', 'n_select_gemm'), ('matvec_launch_ms', 'n_matvec'), ('rank1_launch_ms', 'n_rank1'),
              ('finish_launch_ms', 'n_finish'))


def test_agent_counts_per_phase_and_per_kernel(fading):
    """Per-replica agents of a few landmarks, production library, two identically driven handles.  Three (update_control,
    select_action): three pairs around each phase and around each of update_small / select_bin / select_gemm, none around the
    chip-wide rounds (they are enqueued from 200 queued tiles on, dictionaries of 320+ landmarks); a second reading finds
    nothing.  Two more steps read through kb_kernel_time_ms: four phase pairs, and their mean is the count-weighted mean of
    the two phase means that the same reading left behind for kb_kernel_times_ms."""
    for _ in range(2):
        ag, _ia = _agent(fading)
        rng = np.random.default_rng(9)
        ag.set_kernel_timing(True)
        _drive(ag, rng, 3)
        ph = ag.phase_times_ms()
        print(ph)
        assert ph['n_update'] == 3 and ph['n_select'] == 3
        assert ph['n_update_small'] == ph['n_select_bin'] == ph['n_select_gemm'] == 3
        assert ph['n_matvec'] == ph['n_rank1'] == ph['n_finish'] == 0
        assert ph['update_ms'] > 0 and ph['select_ms'] > 0
        for ms, n in PER_LAUNCH:
            assert (ph[ms] > 0) if ph[n] else (ph[ms] == 0.0), ms
        again = ag.phase_times_ms()
        assert all(again[k] == 0 for k in again), again
        _drive(ag, rng, 2)
        mean, launches = ag.kernel_time_ms()
        km, kn = (C.c_double * 8)(), (C.c_int64 * 8)()
        assert ag.L.kb_kernel_times_ms(ag.h, km, kn) == 0
        assert launches == 4 and kn[0] == 2 and kn[1] == 2
        # (the library forms the same expression in float64: equal but for the last rounding)
        assert mean == pytest.approx((km[0] * kn[0] + km[1] * kn[1]) / (kn[0] + kn[1]), rel=1e-12) and mean > 0
        assert ag.kernel_time_ms() == (0.0, 0)
        ag.close()


def test_agent_in_inference_mode_times_the_select_phase_only(fading):
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=N, cfg=make_config(0, n_envs=N), fading=fading, seed=41)
    ag, ia = _agent(fading)
    env.reset()
    env.step(ia)
    ag.set_learning(False)
    ag.set_kernel_timing(True)
    for _ in range(2):
        ag.step_resident(env)
        env.step_resident()
    ag.synchronize()
    ph = ag.phase_times_ms()
    assert ph['n_update'] == 0 and ph['n_select'] == 2 and ph['update_ms'] == 0.0 and ph['select_ms'] > 0
    assert ph['n_update_small'] == 0 and ph['n_select_bin'] == ph['n_select_gemm'] == 2
    ag.close()
    env.close()


def test_prune_counts_one_pair_per_phase_and_round():
    """Two agents grown past 64 landmarks by teacher-forced updates, one further than the other; prune(64) with timing on: the
    three phases are launched once per round, the rounds of a call are as many as the landmarks removed from the dictionary that
    loses most (one removal per listed dictionary and round; observed on the commit before the timing code was shared), the
    three times are sums and positive, and a second reading finds nothing."""
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(2, [10], 200, capacity=1024, pool_bytes=64 << 20)
    ag.reset([[10]] * 2, [[3]] * 2)
    rng = np.random.default_rng(31)
    for e, cnt in enumerate((200, 160)):   # (a sample becomes a landmark when it is misclassified: about every second one)
        xs, ys = _random_stream(rng, 11, cnt, spread=3.0)
        for i in range(cnt):
            ag.predict(e, 0, xs[i])
            ag.update(e, 0, xs[i], int(ys[i]))
    sizes = ag.dictionary_sizes()[:, 0]
    print('sizes before the prune', sizes)
    assert sizes.min() > 64 and sizes[0] != sizes[1]
    ag.set_kernel_timing(True)
    assert ag.prune(64) == (sizes - 64).sum()
    t = ag.prune_times_ms()
    print(t)
    assert t['n_choose'] == t['n_downdate'] == t['n_move'] >= 1
    assert t['n_choose'] == ag.pruned().max() == sizes.max() - 64
    assert t['choose_ms'] > 0 and t['downdate_ms'] > 0 and t['move_ms'] > 0
    again = ag.prune_times_ms()
    assert (again['choose_ms'], again['downdate_ms'], again['move_ms']) == (0.0, 0.0, 0.0)
    assert again['n_choose'] == again['n_downdate'] == again['n_move'] == 0
    ag.close()
