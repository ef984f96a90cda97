"""rs_fork / VecRanSlice.fork_from: a device-side gather of replicas into another handle.  A forked replica must continue
exactly as its source does under the same actions -- observations (f32 bits), rewards, labels, violations, the info
accumulators (f64 bits) and every traced UE record -- whatever index array built the fork (repeats, a reversed range, a
permutation), in eMBB + mMTC scenarios with churn and with the L1 slices multiplexed."""
import os

import numpy as np
import pytest

from ranslice import _lib
from ranslice.config import make_config
from ranslice.fading import synth_fading

pytestmark = pytest.mark.gpu


def _fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


def _churn(cfg):
    cfg.cbr_lambda, cfg.cbr_t_mean = 2.0 / 1.2, 0.6
    cfg.vbr_lambda, cfg.vbr_t_mean = 5.0 / 1.2, 0.6
    cfg.vbr_b_size, cfg.vbr_b_rate = 40, 12
    return cfg


CONFIGS = {
    's1': lambda n: _churn(make_config(1, n_envs=n)),
    's3': lambda n: _churn(make_config(3, n_envs=n)),
    'mux': lambda n: _churn(make_config(1, n_envs=n, L1_level=False)),
}


def _actions(rng, n, n_slices, n_prbs):
    return rng.multinomial(n_prbs, [1.0 / (n_slices + 1)] * (n_slices + 1), size=n)[:, :n_slices].astype(np.int32)


def _env(cfgf, n, fading, seed):
    from ranslice.vec_env import VecRanSlice
    return VecRanSlice(n_envs=n, cfg=cfgf(n), fading=fading, seed=seed)


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize('name', sorted(CONFIGS))
def test_forked_replicas_continue_as_their_sources(golden_dir, name):
    cfgf, fading = CONFIGS[name], _fading(golden_dir)
    rng = np.random.default_rng(7)
    src = _env(cfgf, 64, fading, seed=901)
    src.set_alloc_trace(True)
    src.reset()
    for _ in range(20):
        src.step(_actions(rng, 64, src.n_slices, src.n_prbs))
    index = np.concatenate([[5, 5, 5, 0, 63, 63], np.arange(63, -1, -1), rng.permutation(64)]).astype(np.int32)
    dst = _env(cfgf, len(index), fading, seed=12345)   # never reset: the fork makes it so
    dst.set_alloc_trace(True)
    dst.fork_from(src, index)
    # the outputs of the last step travel with the replica
    assert _bits(dst.l1_info()) == _bits(src.l1_info()[index])
    for step in range(10):
        A = _actions(rng, 64, src.n_slices, src.n_prbs)
        o_s, r_s, _, i_s = src.step(A)
        o_d, r_d, _, i_d = dst.step(A[index])
        assert _bits(o_d) == _bits(o_s[index]), (name, step)
        assert _bits(r_d) == _bits(r_s[index]), (name, step)
        assert (i_d['SLA_labels'] == i_s['SLA_labels'][index]).all(), (name, step)
        assert (i_d['violations'] == i_s['violations'][index]).all(), (name, step)
        assert _bits(dst.l1_info()) == _bits(src.l1_info()[index]), (name, step)
        assert _bits(dst.alloc_trace()) == _bits(src.alloc_trace()[index]), (name, step)
    # the fork took the source's clock: env-steps count the source's twenty steps and the ten since
    assert dst.counters()[1] == (20 + 10) * len(index)
    src.close()
    dst.close()


def test_fork_refusals(golden_dir):
    fading = _fading(golden_dir)
    cfgf = CONFIGS['s3']
    src = _env(cfgf, 8, fading, seed=3)
    idx = np.arange(8, dtype=np.int32)
    # a source that was never reset
    dst = _env(cfgf, 8, fading, seed=4)
    with pytest.raises(_lib.RanSliceError) as e:
        dst.fork_from(src, idx)
    assert e.value.code == _lib.RS_ESTATE
    src.reset()
    src.step(np.full((8, 2), 10, dtype=np.int32))
    # index out of range, either side
    for bad in (8, -1):
        j = idx.copy()
        j[3] = bad
        with pytest.raises(_lib.RanSliceError) as e:
            dst.fork_from(src, j)
        assert e.value.code == _lib.RS_EINVAL
    # configurations that differ beyond n_envs
    other = _env(lambda n: _churn(make_config(3, n_envs=n, n_prbs=60)), 8, fading, seed=4)
    with pytest.raises(_lib.RanSliceError) as e:
        other.fork_from(src, idx)
    assert e.value.code == _lib.RS_EINVAL
    # different fading tables
    alien = _env(cfgf, 8, [synth_fading(t, 256, seed=99) for t in range(3)], seed=4)
    with pytest.raises(_lib.RanSliceError) as e:
        alien.fork_from(src, idx)
    assert e.value.code == _lib.RS_ESTATE
    # and the good fork still works after the refusals
    dst.fork_from(src, idx[::-1].copy())
    a = np.full((8, 2), 12, dtype=np.int32)
    o_s, r_s, _, _ = src.step(a)
    o_d, r_d, _, _ = dst.step(a)
    assert _bits(o_d) == _bits(o_s[::-1]) and _bits(r_d) == _bits(r_s[::-1])
    for env in (src, dst, other, alien):
        env.close()


def test_fork_4096_into_eight_copies(golden_dir):
    """4096 replicas of scenario 1 forked into 4096 x 8 (every replica eight times, shuffled); a sample of the copies checked"""
    fading = _fading(golden_dir)
    cfgf = CONFIGS['s1']
    rng = np.random.default_rng(11)
    n = 4096
    src = _env(cfgf, n, fading, seed=77)
    src.reset()
    for _ in range(6):
        src.step(_actions(rng, n, src.n_slices, src.n_prbs))
    index = rng.permutation(np.tile(np.arange(n, dtype=np.int32), 8)).astype(np.int32)
    dst = _env(cfgf, 8 * n, fading, seed=78)
    dst.fork_from(src, index)
    sample = rng.choice(8 * n, size=512, replace=False)
    for step in range(4):
        A = _actions(rng, n, src.n_slices, src.n_prbs)
        o_s, r_s, _, i_s = src.step(A)
        o_d, r_d, _, i_d = dst.step(A[index])
        assert _bits(o_d[sample]) == _bits(o_s[index[sample]]), step
        assert _bits(r_d[sample]) == _bits(r_s[index[sample]]), step
        assert (i_d['violations'][sample] == i_s['violations'][index[sample]]).all(), step
    src.close()
    dst.close()
