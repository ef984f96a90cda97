"""The step kernel's launch constants, instance by instance, against the oracle bit for bit.

The plain instances keep what they need of the three fading traces (length, column / element / valid-byte offsets) in an LDS
table indexed by a UE's trace type, the BLOCK, tracing and 32-lane instances select among twelve launch constants; the PF share's reciprocal form is a template argument of every instance, picked at launch; the rest of the
boolean configuration (NaN columns present, reception test by guard band, estimates from prefix sums) is read once per launch.
A wrong table row, a wrong instance or a stale flag shows at the smallest shapes -- 8 replicas, 5 eMBB slices, 3 steps -- if the three traces differ in length and
offset, one of them has a NaN column, and the walkers leave their traces within the run:

* traces of 64, 96 and 128 time samples (the second with a NaN column): a walker reflects within 150 slots, so the estimate
  prologue's non-`straight` branch and the `fad_valid` offsets are used;
* arrival rates high enough that every task holds UEs of all three trace types (about twenty UEs per slice by the third step: the
  chance that some trace type is missing among the >= 60 UEs the reference check below asks for is below 1e-10) and that some
  task outgrows 16 lanes, which sends it to the 32-lane replay;
* one slice of at least 24 RB pairs per step, for the BLOCK instance's block rounds.

The inputs are prepared and run through the oracle alone first (no replica may raise); every GPU case compares with that one
reference: obs as float32 bits, reward, labels, violations, the ten info sums per slice as float64 bits, and -- tracing instance --
every UE's allocation record in every slot.

The split step's 8-lane instance behind the cost ranking needs 4096 tasks (rs_api.hip: launch_step); at this size it is reached
only as the primary instance (set_group_size(8)), which is run here; the split itself is covered by the full-size tests.
"""
import numpy as np
import pytest

from oracle import pyoracle as po
from ranslice.config import make_config
from ranslice.fading import synth_fading
from ranslice.sharding import replica_seed

pytestmark = pytest.mark.gpu

N_ENVS, STEPS, SEED = 8, 3, 2718
# slice 0, then 1, then 4 holds >= 24 RB pairs (PF granularity 2); small and empty slices beside them
ACTIONS = np.array([[100, 40, 30, 20, 10], [20, 120, 20, 20, 20], [13, 7, 1, 0, 179]], dtype=np.int32)


def _cfg(n):
    c = make_config(0, n_envs=n)
    c.cbr_lambda, c.cbr_t_mean = 40.0, 5.0
    c.vbr_lambda, c.vbr_t_mean = 100.0, 5.0
    c.vbr_b_size, c.vbr_b_rate = 40, 12
    return c


@pytest.fixture(scope='module')
def fading():
    f = [synth_fading(0, 64), synth_fading(1, 96, nan_cols=(40,)), synth_fading(2, 128)]
    assert [t.shape[1] for t in f] == [64, 96, 128] and np.isnan(f[1]).any() and not np.isnan(f[0]).any()
    return f


@pytest.fixture(scope='module')
def reference(fading):
    """the oracle alone, once: per step and replica obs, reward, labels, violations, info and the allocation trace"""
    ref = []
    oracles = []
    for r in range(N_ENVS):
        o = po.OracleEnv(_cfg(1), fading)
        o.set_seed(replica_seed(SEED, r))
        o.reset()
        oracles.append(o)
    for i in range(STEPS):
        ref.append([o.step(ACTIONS[i], trace=True) for o in oracles])   # (an overflow or any other flag raises OracleError)
    # what the cases below rely on, checked on the CPU: enough UEs for all three trace types, and a task wider than 16 lanes
    last = np.stack([out['trace'] for out in ref[-1]])                  # [replica][slice][slot][UE]
    held = (last['prbs'] != 0) | (last['queue'] != 0) | (last['th'] != 0) | (last['serial'] != 0)
    per_task = held.sum(axis=-1).max(axis=-1)                           # most UEs a task held in a slot of the last step
    assert per_task.sum() >= 60, per_task
    assert per_task.max() > 16, per_task
    assert per_task.max() <= 32, per_task
    return ref


def _compare(env, reference, trace=False):
    for i in range(STEPS):
        acts = np.ascontiguousarray(np.broadcast_to(ACTIONS[i], (N_ENVS, 5)), dtype=np.int32)
        obs, rew, _, info = env.step(acts)
        l1 = env.l1_info()
        tr = env.alloc_trace() if trace else None
        for r, out in enumerate(reference[i]):
            assert obs[r].tobytes() == out['obs'].tobytes(), ('obs', i, r)
            assert rew[r] == out['reward'], ('reward', i, r)
            assert (info['SLA_labels'][r] == out['labels']).all(), ('labels', i, r)
            assert (info['violations'][r] == out['violations']).all(), ('violations', i, r)
            assert l1[r].tobytes() == out['info'].tobytes(), ('info', i, r)
            if trace:
                a, b = tr[r], out['trace']
                for f in ('serial', 'type', 'e_snr', 'prbs', 'bits'):
                    assert (a[f] == b[f]).all(), (f, i, r)
                for f in ('queue', 'th', 'p'):
                    assert a[f].tobytes() == b[f].tobytes(), (f, i, r)
    env.close()


def _env(fading, group=None, hint=None, trace=False):
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=N_ENVS, cfg=_cfg(N_ENVS), fading=fading, seed=SEED)
    if group:
        env.set_group_size(group)
    if hint is not None:
        env.set_schedule_hint(hint)
    if trace:
        env.set_alloc_trace(True)
    env.reset()
    return env


def test_plain_16_lane_instance_and_its_32_lane_replay(fading, reference):
    """embb_step_kernel<16, false, false, FDIV>; the tasks that outgrow 16 lanes are replayed by <32, false, true, FDIV>"""
    _compare(_env(fading, group=16, hint=0), reference)


def test_block_instance(fading, reference):
    """embb_step_kernel<16, false, true, FDIV> through rs_set_schedule_hint: every step has a slice of >= 24 RB pairs"""
    _compare(_env(fading, group=16, hint=1), reference)


def test_32_lane_instance(fading, reference):
    """embb_step_kernel<32, false, true, FDIV> as the primary instance"""
    _compare(_env(fading, group=32), reference)


def test_8_lane_instance(fading, reference):
    """embb_step_kernel<8, false, false, FDIV> as the primary instance (most tasks go on to the 32-lane replay)"""
    _compare(_env(fading, group=8, hint=0), reference)


@pytest.mark.parametrize('group', [16, 32])
def test_tracing_instances(fading, reference, group):
    """embb_step_kernel<G, true, true, FDIV>: the estimates by the pairwise sum, every probability exact, and every UE's
    allocation record in every slot"""
    _compare(_env(fading, group=group, trace=True), reference, trace=True)


@pytest.mark.parametrize('hint', [0, 1])
def test_every_flag_off(fading, reference, hint, monkeypatch):
    """The other value of every flag (the NaN flag is on throughout this file; the smoke run's traces have no NaN): the FDIV = false
    instances (the PF share by the IEEE divide), the reception probability exact for every UE and every estimate by the pairwise
    sum.  No slot length was found for which rs_create rejects the reciprocal form by itself (1e-3 and some 150 others between
    2e-4 and 2e-3 pass its check for every `bits` up to 12,000), so the test build's switch that forces the same RsDev.pf_div_fast = 0
    is used."""
    monkeypatch.setenv('RANSLICE_DEV_BUILD', '1')   # knobs are read by the test build only (ranslice._lib)
    monkeypatch.setenv('RANSLICE_EXACT_DIV', '1')
    monkeypatch.setenv('RANSLICE_RX_EXACT', '1')
    monkeypatch.setenv('RANSLICE_EST_EXACT', '1')
    _compare(_env(fading, group=16, hint=hint), reference)
