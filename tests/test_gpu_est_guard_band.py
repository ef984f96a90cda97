"""The channel estimate by guard band on the device (rs_embb.hip: the est_fast block; rs_api.hip: upload_fading), on fading tables
whose column means sit at half-integers (tests/est_adversarial.py; the CPU side and the census of these inputs are in
tests/test_est_guard_band.py).

With prop_A = prop_B = 0 the path loss is the FSPL floor and about a tenth of the UEs carry the clamped nominal SINR 61.0; on the
families' columns every estimate of theirs is a rounding at a half-integer, where the mean formed from two prefix-sum entries and
numpy's pairwise sum of the samples land on different sides often enough (the census: 118 of 19,968 spans of family A, 160 of
13,824 of family B, not counting those where the fast mean is an exact tie).  One wrong rounding changes the UE's MCS, hence its
bits, hence the observations -- and the mean e_snr is an observation itself.

  * the production band, on every instance of the step kernel (8, 16 and 32 lanes per task; at 16 the plain and the BLOCK
    instance, and once on two lanes of the step loop): observations, rewards, labels, violations and the info sums equal the
    oracle's bit for bit for every replica and step;
  * RANSLICE_EST_EXACT=1 (every estimate by the pairwise sum) and RANSLICE_EST_BAND=0.2: the same bytes;
  * the control: RANSLICE_EST_BAND=1e-300 leaves only exact ties to the pairwise sum, and the device must then DIFFER from the
    oracle -- the run reaches estimates that the band alone decides correctly.  A wrong answer on purpose, nothing else;
  * samples of exactly +-1000.0 (family B) do not switch the short paths off, and family B runs the float32 reception test at
    the largest sample magnitude its band was derived for.

Allocation tracing stays off: the tracing instances form every estimate by the pairwise sum.  The oracle's trajectories are
computed once per family and shared.  The lanes of the step loop are stepped by the device's own action script only (rs_set_lanes),
so that case follows po.random_actions; every other case takes the families' scripts, rows in rotation.

Measured on the MI355X (python -m pytest tests/test_gpu_est_guard_band.py -q -m gpu -s): under the band of 1e-300, 41 of the 384
(step, replica) observation rows differ from the oracle on family A and 95 on family B, the first at step 0; rx_stats under the
production band (tests, exact, available): (96018, 29, True) on A, (108615, 31, True) on B.  Each case takes under a second.
"""
import numpy as np
import pytest

import est_adversarial as ea
from oracle import pyoracle as po
from ranslice.sharding import replica_seed

pytestmark = pytest.mark.gpu

N, STEPS, SEED, ACT_SEED = 48, 8, 5, 77
KNOBS = ('RANSLICE_RX_EXACT', 'RANSLICE_RX_BAND_SCALE', 'RANSLICE_EST_EXACT', 'RANSLICE_EST_BAND')
KEYS = ('obs', 'reward', 'labels', 'violations', 'info')


class _Family:
    def __init__(self, name):
        self.name = name
        self.tables = ea.family_a() if name == 'A' else ea.family_b()
        self.script = ea.SCRIPT_A if name == 'A' else ea.SCRIPT_B
        self._ref = {}

    def cfg(self, n):
        if self.name == 'A':
            return ea.floor_config(0, n_envs=n)                                      # 200 PRBs, 5 eMBB slices
        return ea.floor_config(None, n_envs=n, n_prbs=256, n_embb=5, n_mmtc=0)       # the build's widest carrier

    def actions(self, scripted, step):
        if scripted:
            return ea.rotation(self.script, N, step)
        return np.array([po.random_actions(self.cfg(N), ACT_SEED, step, r) for r in range(N)], dtype=np.int32)

    def oracle(self, scripted):
        """{key: [STEPS][N]...} of the oracle over the scripted / the random actions, computed once"""
        if scripted not in self._ref:
            out = {k: [] for k in KEYS}
            acts = [self.actions(scripted, i) for i in range(STEPS)]
            rows = []
            for r in range(N):
                o = po.OracleEnv(self.cfg(1), self.tables)
                o.set_seed(replica_seed(SEED, r))
                o.reset()
                rows.append([o.step(acts[i][r]) for i in range(STEPS)])
            for k in KEYS:
                out[k] = np.array([[rows[r][i][k] for r in range(N)] for i in range(STEPS)])
                out[k].setflags(write=False)
            self._ref[scripted] = out
        return self._ref[scripted]


@pytest.fixture(scope='module', params=['A', 'B'])
def fam(request):
    return _Family(request.param)


def _device(fam, monkeypatch, group=16, hint=None, lanes=None, knob=None):
    """-> ({key: [STEPS][N]...}, rx_stats) of one handle over the family's script (the random script on lanes)"""
    from ranslice.vec_env import VecRanSlice
    monkeypatch.setenv('RANSLICE_DEV_BUILD', '1')        # the knobs are read by the test build only (ranslice._lib)
    for v in KNOBS:
        monkeypatch.delenv(v, raising=False)
    if knob:
        monkeypatch.setenv(*knob)
    env = VecRanSlice(n_envs=N, cfg=fam.cfg(N), fading=fam.tables, seed=SEED)
    env.set_group_size(group)
    if hint is not None:
        env.set_schedule_hint(hint)
    if lanes:
        env.set_lanes(lanes)
    env.reset()
    out = {k: [] for k in KEYS}
    for i in range(STEPS):
        if lanes:
            env.random_actions(ACT_SEED, i)
            env.step_resident()
            if i == 0:
                assert env.lane_info()[0] == lanes
            f = env.fetch()
            assert (f['actions'] == fam.actions(False, i)).all()
        else:
            obs, rew, _, info = env.step(fam.actions(True, i))
            f = dict(obs=obs, reward=rew, labels=info['SLA_labels'], violations=info['violations'])
        for k in KEYS[:-1]:
            out[k].append(f[k])
        out['info'].append(env.l1_info())
    stats = env.rx_stats()
    env.close()
    return {k: np.array(v) for k, v in out.items()}, stats


def _differing(got, ref):
    """(step, replica) pairs whose observations differ in any bit, and the first key and place at which anything differs"""
    first = None
    for k in KEYS:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
        for i in range(STEPS):
            for r in range(N):
                if first is None and got[k][i, r].tobytes() != ref[k][i, r].tobytes():
                    first = (k, i, r)
    obs = sum(got['obs'][i, r].tobytes() != ref['obs'][i, r].tobytes() for i in range(STEPS) for r in range(N))
    return obs, first


def _check_stats(stats):
    tests, exact, avail = stats
    assert avail == 1, stats               # samples of exactly +-1000.0 keep the short paths
    assert 0 < exact < tests, stats


@pytest.mark.parametrize('group,hint,lanes', [(8, None, None), (16, 0, None), (16, 1, None), (32, None, None), (16, None, 2)],
                         ids=['g8', 'g16-plain', 'g16-block', 'g32', 'g16-lanes2'])
def test_production_band_equals_the_oracle_on_every_instance(fam, monkeypatch, group, hint, lanes):
    got, stats = _device(fam, monkeypatch, group=group, hint=hint, lanes=lanes)
    n_obs, first = _differing(got, fam.oracle(not lanes))
    print('family %s group %d hint %s lanes %s: rx_stats %r' % (fam.name, group, hint, lanes, stats))
    assert first is None and n_obs == 0, 'family %s: %d observations differ, first difference (key, step, replica) %r' % (
        fam.name, n_obs, first)
    _check_stats(stats)


@pytest.mark.parametrize('knob', [('RANSLICE_EST_EXACT', '1'), ('RANSLICE_EST_BAND', '0.2')], ids=['exact', 'band0.2'])
def test_other_band_settings_give_the_same_bytes(fam, monkeypatch, knob):
    got, stats = _device(fam, monkeypatch, knob=knob)
    n_obs, first = _differing(got, fam.oracle(True))
    assert first is None and n_obs == 0, (fam.name, knob, n_obs, first)
    _check_stats(stats)


def test_without_the_band_the_device_differs(fam, monkeypatch):
    """the control: a band of 1e-300 (0.5 - 1e-300 == 0.5, so only an exact tie still falls back) must get roundings wrong"""
    got, stats = _device(fam, monkeypatch, knob=('RANSLICE_EST_BAND', '1e-300'))
    n_obs, first = _differing(got, fam.oracle(True))
    print('family %s, band 1e-300: %d of %d observations differ from the oracle, first difference %r' % (fam.name, n_obs, N * STEPS, first))
    assert n_obs >= 1 and first is not None, 'the inputs do not reach a decision that the band takes'
