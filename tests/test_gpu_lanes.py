"""Lanes of the step loop (rs_set_lanes): a handle whose replica ranges are stepped on streams of their own, not joined between
steps, against a twin at rs_set_lanes(1) with the same seeds and the same script.  Everything is compared bit for bit: what
fetch() returns, the counters, the reception statistics, the info sums and the saved state.

The saved state is compared whole but for two of its regions that differ between any two handles, single-lane twins
included: the table of device pointers to the state arrays (struct RsState, addresses of the handle's own allocations, which
rs_load_state does not restore either) and the four pace words of the step kernel (sums of cycle counts of the waves, read
from the device's clock).  On a handle without mMTC slices they are the third last and the last region; the run words
between them are compared.  Every other byte -- the header, the constants, the simulator state, the outputs, the counters and
the launch-order scratch -- must be equal.  The batches are one wave of tasks (at most 64), where the ranks the ordering
kernels take by atomics are taken in lane order.

None of these sizes engages lanes by itself, so they are forced; 16 lanes per task is set because the handles that engage
lanes by themselves run that instance (small batches default to 32)."""
import os
import re

import numpy as np
import pytest

from oracle import pyoracle as po
from ranslice.config import make_config
from ranslice.sharding import replica_seed

pytestmark = pytest.mark.gpu

SEED = 77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_BYTES = PACE_BYTES = 32


def _pointer_table_bytes():
    """sizeof(struct RsState): pointers only"""
    text = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'rs_device.h')).read()
    body = re.search(r'struct RsState \{(.*?)\n\};', text, flags=re.S).group(1)
    fields = [ln for ln in re.sub(r'//[^\n]*', '', body).split(';') if ln.strip()]
    assert fields and all(re.match(r'^\s*\w+\*\s+\w+$', f) for f in fields), fields
    return 8 * len(fields)


def _comparable(blob):
    """the saved state without the pointer table and the pace words"""
    st = _pointer_table_bytes()
    assert blob.size > st + RUN_BYTES + PACE_BYTES
    return blob[:-(st + RUN_BYTES + PACE_BYTES)].tobytes() + blob[-(RUN_BYTES + PACE_BYTES):-PACE_BYTES].tobytes()


@pytest.fixture(scope='module')
def fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


def _cfg(n, crowd=False):
    """scenario 0 with per-slice L1 and traffic that makes arrivals, departures and bursts fire within a few steps"""
    c = make_config(0, n_envs=n)
    c.cbr_lambda, c.cbr_t_mean = 2.0 / 1.2, 0.6
    c.vbr_lambda, c.vbr_t_mean = 5.0 / 1.2, 0.6
    c.vbr_b_size, c.vbr_b_rate = 40, 12
    if crowd:                                    # most slices beyond 8 UEs
        c.cbr_lambda, c.vbr_lambda, c.cbr_t_mean, c.vbr_t_mean = 8.0, 18.0, 0.8, 0.8
    return c


def _env(n, fading, lanes, group=16, crowd=False, seed=11, reset=True):
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=n, cfg=_cfg(n, crowd), fading=fading, seed=seed)
    env.set_group_size(group)
    env.set_lanes(lanes)
    if reset:
        env.reset()
    return env


def _run(env, k, i0=0):
    for i in range(i0, i0 + k):
        env.random_actions(SEED, i)
        env.step_resident()
    return i0 + k


def _snapshot(env):
    out = {k: v.tobytes() for k, v in env.fetch().items()}
    assert sorted(out) == ['actions', 'labels', 'obs', 'reward', 'violations']
    out['counters'] = tuple(env.counters())
    out['rx_stats'] = tuple(env.rx_stats())
    out['info'] = env.l1_info().tobytes()
    blob = env.save_state()
    out['state'] = _comparable(blob)
    out['state_bytes'] = blob.size
    return out


def _assert_same(a, b, what='', skip=()):
    sa, sb = _snapshot(a), _snapshot(b)
    for k in sa:
        assert k in skip or sa[k] == sb[k], '%s differs %s' % (k, what)


@pytest.mark.parametrize('n,lanes,in_use', [(7, 2, 2), (6, 4, 4), (8, 2, 2), (2, 4, 2)])
def test_uneven_ranges_and_wave_boundaries(fading, n, lanes, in_use):
    """task counts per lane 20 / 15, 10 / 10 / 5 / 5 and 20 / 20: lanes shorter than a wave, counts that are no multiple of the
    four tasks of a wave (the heavy + light pairing falls back), and more lanes asked for than there are replicas (clamped to
    one replica per lane: no launch without a task)"""
    a, t = _env(n, fading, lanes), _env(n, fading, 1)
    assert a.lane_info()[0] == in_use and t.lane_info()[0] == 1
    _run(a, 40)
    _run(t, 40)
    _assert_same(a, t)
    assert a.counters()[3] > 0
    a.close()
    t.close()


def test_lanes_are_refused_where_the_mode_has_none(fading):
    from ranslice import _lib
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=4, cfg=make_config(1, n_envs=4), fading=fading, seed=1)   # three eMBB and two mMTC slices
    with pytest.raises(_lib.RanSliceError) as e:
        env.set_lanes(2)
    assert e.value.code == _lib.RS_EINVAL
    env.set_lanes(1)
    env.set_lanes(0)
    assert env.lane_info()[0] == 1
    env.close()


def test_replay_inside_a_lane(fading):
    """8 lanes per task and crowded slices: tasks raise their redo flag in the primary launch and the 32-lane replay of the
    lane takes them"""
    n, steps = 7, 20
    a, t = _env(n, fading, 2, group=8, crowd=True), _env(n, fading, 1, group=8, crowd=True)
    _run(a, steps)
    _run(t, steps)
    _assert_same(a, t)
    # UE-slots per (slot, task): beyond 8 on average, so tasks outgrew the 8-lane instance and were replayed
    assert a.counters()[3] / float(steps * a.cfg.slots_per_step * n * 5) > 8.0
    a.close()
    t.close()


def _host_actions(rng, n):
    return rng.multinomial(200, [1 / 6.0] * 6, size=n)[:, :5].astype(np.int32)


def test_consumers_in_the_middle(fading):
    """after every fifth step one of the entry points that need the whole batch, on both handles; then laned steps again"""
    n = 8
    a, t = _env(n, fading, 2), _env(n, fading, 1)
    spare = {id(a): _env(n, fading, 1), id(t): _env(n, fading, 1)}
    rng = np.random.default_rng(5)
    ident = np.arange(n, dtype=np.int32)
    i = 0
    for block in range(8):
        i = _run(a, 5, i)
        _run(t, 5, i - 5)
        kind = block % 7
        acts = _host_actions(rng, n)
        got = []
        for env in (a, t):
            if kind == 0:
                got.append({k: v.tobytes() for k, v in env.fetch().items()})
            elif kind == 1:
                got.append(env.counters())
            elif kind == 2:
                got.append(_comparable(env.save_state()))
            elif kind == 3:
                obs, rew, _, info = env.step(acts)
                got.append((obs.tobytes(), rew.tobytes(), info['violations'].tobytes()))
            elif kind == 4:
                view = env.device_view()
                env.step_device(view['in_prbs'].set(acts))
                got.append(view['obs'].get().tobytes())
            elif kind == 5:
                # rs_fork refuses a handle as its own source: out to a spare handle and back, the identity both ways (the
                # laned handle is the source of one fork and the destination of the other)
                spare[id(env)].fork_from(env, ident)
                env.fork_from(spare[id(env)], ident)
                got.append(None)
            else:
                env.set_kernel_timing(True)
                env.set_kernel_timing(False)
                got.append(None)
        assert got[0] == got[1], 'consumer %d' % kind
    assert a.lane_info()[0] == 2
    _assert_same(a, t)
    for env in (a, t) + tuple(spare.values()):
        env.close()


def test_run_random(fading):
    """6 steps of rs_run_random without a graph on lanes = 6 call pairs; with a graph the loop is the single-lane one, as
    before, and equal.  (rs_run_random leaves the script's seed in the run words, call pairs do not: the saved state is
    compared with a single-lane twin that calls rs_run_random too, everything else with the call pairs as well.)"""
    n = 7
    a, t, p = _env(n, fading, 2), _env(n, fading, 1), _env(n, fading, 1)
    a.run_random(SEED, 0, 6)
    t.run_random(SEED, 0, 6)
    _run(p, 6)
    _assert_same(a, t, 'after run_random without a graph')
    _assert_same(a, p, 'after run_random without a graph (call pairs)', skip=('state',))
    a.run_random(SEED, 6, 6, graph=True)
    t.run_random(SEED, 6, 6, graph=True)
    _run(p, 6, 6)
    _assert_same(a, t, 'after run_random with a graph')
    _assert_same(a, p, 'after run_random with a graph (call pairs)', skip=('state',))
    a.run_random(SEED, 12, 5)          # (and on lanes again behind a graph: an odd count, the parity of the counters moves)
    t.run_random(SEED, 12, 5)
    _run(p, 5, 12)
    _assert_same(a, t, 'after run_random behind the graph')
    _assert_same(a, p, 'after run_random behind the graph (call pairs)', skip=('state',))
    for env in (a, t, p):
        env.close()


def test_checkpoint_while_open(fading):
    n = 7
    a, t = _env(n, fading, 2), _env(n, fading, 1)
    _run(a, 10)
    blob = a.save_state()                                  # (the handle is open here)
    b = _env(n, fading, 2)
    b.load_state(blob)
    _run(b, 10, 10)
    _run(a, 10, 10)
    _run(t, 20)
    _assert_same(b, t, '(restored)')
    _assert_same(a, t, '(saved from)')
    for env in (a, b, t):
        env.close()


def test_timing_with_lanes(fading):
    """one sample per step, the sum over the step's lanes; no duration is held against a threshold"""
    n, lanes = 8, 2
    a = _env(n, fading, lanes)
    _run(a, 3)
    a.set_kernel_timing(True)
    a.run_random(SEED, 3, 4)
    (mean, mn, mx), launches = a.kernel_time_stats_ms()
    assert launches == 4
    assert 0.0 < mn <= mean <= mx
    in_use, total, union, hidden = a.lane_info()
    assert in_use == lanes
    assert 0.0 < union <= total
    assert 0.0 <= hidden < 1.0
    # the same pairs, once as differences of float32 timestamps against the reference event (well below a second: half an ulp
    # is under 3e-5 ms), once as the pairs' own elapsed times
    assert abs(total - mean) <= 1e-3
    a.set_kernel_timing(False)
    a.close()


def test_lanes_against_the_oracle(fading):
    """one replica of each lane of the (7, 2) case against the CPU oracle over the same action script"""
    n, steps, seed0 = 7, 40, 11
    a = _env(n, fading, 2, seed=seed0)
    reps = (1, 5)
    oracles = []
    for r in reps:
        o = po.OracleEnv(_cfg(1), fading)
        o.set_seed(replica_seed(seed0, r))
        o.reset()
        oracles.append(o)
    for i0 in range(0, steps, 8):
        _run(a, 8, i0)
        got = a.fetch()
        l1 = a.l1_info()
        for r, o in zip(reps, oracles):
            for i in range(i0, i0 + 8):
                acts = po.random_actions(a.cfg, SEED, i, r)
                out = o.step(acts)
            assert (got['actions'][r] == acts).all()
            assert got['obs'][r].tobytes() == out['obs'].tobytes(), 'obs bits differ: step %d replica %d' % (i0 + 7, r)
            assert got['reward'][r] == out['reward']
            assert (got['labels'][r] == out['labels']).all() and (got['violations'][r] == out['violations']).all()
            assert l1[r].tobytes() == out['info'].tobytes()
    a.close()
