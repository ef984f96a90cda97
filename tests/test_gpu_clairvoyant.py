"""rs_step_clairvoyant / VecRanSlice.step_clairvoyant: the clairvoyant allocation rule, checked against the independent CPU
oracle.  For every step, replica, slice s and candidate k <= R_s an oracle replica with the same seed is replayed through
the chosen actions so far and stepped once with (a_0 .. a_{s-1}, k, 0 .. 0); the device's a_s must be the candidate that
minimises (violations[s], k).  The trajectory itself must be the oracle's under the chosen actions, bit for bit."""
import os

import numpy as np
import pytest

from oracle import pyoracle as po
from ranslice.config import make_config
from ranslice.sharding import replica_seed

pytestmark = pytest.mark.gpu


def _fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


def _churn(cfg):
    cfg.cbr_lambda, cfg.cbr_t_mean = 2.0 / 1.2, 0.6
    cfg.vbr_lambda, cfg.vbr_t_mean = 5.0 / 1.2, 0.6
    cfg.vbr_b_size, cfg.vbr_b_rate = 40, 12
    return cfg


def _heavy(cfg):
    # some nine UEs at a time and short holding times: slices that a few PRBs cannot serve
    cfg.cbr_lambda, cfg.cbr_t_mean = 10.0, 0.3
    cfg.vbr_lambda, cfg.vbr_t_mean = 20.0, 0.3
    cfg.vbr_b_size, cfg.vbr_b_rate = 40, 12
    return cfg


def _oracle(cfgf, fading, seed, r, history):
    o = po.OracleEnv(cfgf(1), fading)
    o.set_seed(replica_seed(seed, r))
    o.reset()
    for a in history:
        o.step(a)
    return o


def _check_rule(golden_dir, cfgf, n, steps, seed, fallback='cheapest'):
    """runs the clairvoyant env and checks every choice (a), the trajectory (b) and exactness (c); returns the number of
    slices without a feasible candidate"""
    from ranslice.vec_env import VecRanSlice
    fading = _fading(golden_dir)
    env = VecRanSlice(n_envs=n, cfg=cfgf(n), fading=fading, seed=seed)
    env.reset()
    env.set_clairvoyant_fallback(fallback)
    S, P = env.n_slices, env.n_prbs
    history = [[] for _ in range(n)]
    mains = [_oracle(cfgf, fading, seed, r, []) for r in range(n)]
    infeasible = 0
    for t in range(steps):
        acts, obs, rew, lab, viol = env.step_clairvoyant()
        for r in range(n):
            prefix = np.zeros(S, dtype=np.int32)
            for s in range(S):
                R = P - int(prefix[:s].sum())
                vs = []
                for k in range(R + 1):
                    cand = prefix.copy()
                    cand[s] = k
                    vs.append(int(_oracle(cfgf, fading, seed, r, history[r]).step(cand)['violations'][s]))
                vmin = min(vs)
                ks = [k for k, v in enumerate(vs) if v == vmin]
                best = (vmin, ks[-1] if (fallback == 'widest' and vmin > 0) else ks[0])
                assert acts[r, s] == best[1], ('rule', t, r, s, acts[r], best)
                prefix[s] = best[1]
                # (c) the final step reproduces the label the search saw: feasible slices end with +1
                assert viol[r, s] == best[0], ('exactness', t, r, s)
                if best[0] == 0:
                    assert lab[r, s] == 1, ('feasible slice violated', t, r, s)
                else:
                    infeasible += 1
            # (b) the real step is the oracle's under the chosen action
            out = mains[r].step(acts[r])
            assert obs[r].tobytes() == out['obs'].tobytes(), ('obs', t, r)
            assert rew[r] == out['reward'] and (lab[r] == out['labels']).all() and (viol[r] == out['violations']).all(), \
                ('outputs', t, r)
            history[r].append(acts[r].copy())
    env.close()
    return infeasible


@pytest.mark.parametrize('traffic', ['scenario', 'churn', 'heavy'])
def test_choices_follow_the_rule_against_the_oracle(golden_dir, traffic):
    """(a) + (b) + (c) on scenario 3 (70 PRBs, one eMBB and one mMTC slice), 4 replicas, 12 steps: with the scenario's
    traffic, with churn, and with heavy churn"""
    shape = {'scenario': lambda c: c, 'churn': _churn, 'heavy': _heavy}[traffic]
    _check_rule(golden_dir, lambda n: shape(make_config(3, n_envs=n)), n=4, steps=12, seed=2024)


@pytest.mark.parametrize('fallback', ['cheapest', 'widest'])
def test_infeasible_slices_follow_the_fallback(golden_dir, fallback):
    """(e) a 6-PRB carrier under heavy churn: slices that no candidate satisfies take the cheapest (default) or the widest
    (rs_set_clairvoyant_fallback(h, 1)) of the least-violating candidates"""
    infeasible = _check_rule(golden_dir, lambda n: _heavy(make_config(3, n_envs=n, n_prbs=6)), n=4, steps=12, seed=77,
                             fallback=fallback)
    assert infeasible > 0


def test_widest_fallback_against_the_oracle(golden_dir):
    """the widest fallback on scenario 3 under heavy churn: feasible slices still take the smallest feasible k"""
    _check_rule(golden_dir, lambda n: _heavy(make_config(3, n_envs=n)), n=4, steps=12, seed=31, fallback='widest')


def test_chunking_does_not_change_the_choices(golden_dir):
    """(d) 256 replicas searched 1, 14 or all 256 at a time (max_branches 71, 1000, 300,000) choose the same actions"""
    from ranslice.vec_env import VecRanSlice
    fading = _fading(golden_dir)
    runs = []
    for mb in (71, 1000, 300000):
        env = VecRanSlice(n_envs=256, cfg=_churn(make_config(3, n_envs=256)), fading=fading, seed=5)
        env.set_lookahead(mb)
        env.reset()
        out = [env.step_clairvoyant() for _ in range(5)]
        runs.append(out)
        env.close()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            for x, y in zip(a, b):
                assert x.tobytes() == y.tobytes()


def test_lookahead_capacity_checks(golden_dir):
    from ranslice import _lib
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice(n_envs=4, cfg=make_config(3, n_envs=4), fading=_fading(golden_dir), seed=1)
    with pytest.raises(_lib.RanSliceError) as e:
        env.set_lookahead(70)           # fewer than the n_prbs + 1 candidates of one replica
    assert e.value.code == _lib.RS_EINVAL
    env.reset()
    env.set_lookahead(0)                # no capacity: the library refuses instead of searching
    with pytest.raises(_lib.RanSliceError) as e:
        env._check(env.L.rs_step_clairvoyant(env.h, None, None, None, None, None))
    assert e.value.code == _lib.RS_ESTATE
    env.set_lookahead(71)
    acts = env.step_clairvoyant()[0]
    assert acts.shape == (4, 2) and (acts.sum(axis=1) <= 70).all()
    env.close()
