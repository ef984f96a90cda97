"""Device-resident policy interface on the GPU (csrc/rs_policy_io.hip): rs_step_device against the host step on twin
environments, bit for bit -- PRB rows, ReportWrapper's simplex, table rows; refusals; stream ordering against a second
stream; torch tensors over the view; the example script."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


class Hip:
    """the few HIP runtime calls the tests make themselves, resolved through libranslice.so's own dependency (so they
    land in the runtime the library uses)"""

    def __init__(self):
        from ranslice import _lib
        L = _lib.load()
        vp = C.c_void_p
        self.malloc = L.hipMalloc
        self.malloc.argtypes = [C.POINTER(vp), C.c_size_t]
        self.free = L.hipFree
        self.free.argtypes = [vp]
        self.memcpy = L.hipMemcpy
        self.memcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        self.memcpy_async = L.hipMemcpyAsync
        self.memcpy_async.argtypes = [vp, vp, C.c_size_t, C.c_int, vp]
        self.memset_async = L.hipMemsetAsync
        self.memset_async.argtypes = [vp, C.c_int, C.c_size_t, vp]
        self.stream_create = L.hipStreamCreateWithFlags
        self.stream_create.argtypes = [C.POINTER(vp), C.c_uint]
        self.stream_sync = L.hipStreamSynchronize
        self.stream_sync.argtypes = [vp]
        self.stream_destroy = L.hipStreamDestroy
        self.stream_destroy.argtypes = [vp]
        for f in (self.malloc, self.free, self.memcpy, self.memcpy_async, self.memset_async, self.stream_create,
                  self.stream_sync, self.stream_destroy):
            f.restype = C.c_int

    def buffer(self, nbytes):
        p = C.c_void_p()
        assert self.malloc(C.byref(p), nbytes) == 0
        return p

    def upload(self, p, a):
        a = np.ascontiguousarray(a)
        assert self.memcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice


def _valid_actions(rng, n, n_prbs, S):
    return rng.multinomial(n_prbs, [1.0 / (S + 1)] * (S + 1), size=n)[:, :S].astype(np.int32)


def _read(env, view):
    out = {k: view[k].get() for k in ('obs', 'reward', 'labels', 'violations', 'total_violations', 'actions', 'resources',
                                      'obs_norm')}
    out['l1_info'] = env.l1_info()
    return out


def _same(host, dev, acts):
    obs, rew, done, info = host
    assert dev['obs'].tobytes() == obs.tobytes()
    assert dev['reward'].tobytes() == rew.tobytes()
    assert (dev['labels'] == info['SLA_labels']).all() and (dev['violations'] == info['violations']).all()
    assert dev['total_violations'].dtype == np.int32 and (dev['total_violations'] == info['total_violations']).all()
    assert (dev['actions'] == acts).all() and (dev['resources'] == acts.sum(axis=1)).all()


@pytest.mark.parametrize('scenario,l1', [(0, True), (2, True), (1, False)])
def test_prbs_step_matches_host_step(fading, scenario, l1):
    from oracle import pyoracle as po
    from ranslice import _lib
    from ranslice.config import make_config
    from ranslice.device_io import DeviceArray
    from ranslice.report import normalise_obs
    from ranslice.sharding import replica_seed
    from ranslice.vec_env import VecRanSlice
    hip = Hip()
    n, steps, seed = 64, 12, 4100 + scenario
    mk = lambda n_envs: make_config(scenario, n_envs=n_envs, L1_level=l1)
    a = VecRanSlice(n_envs=n, cfg=mk(n), fading=fading, seed=seed)
    b = VecRanSlice(n_envs=n, cfg=mk(n), fading=fading, seed=seed)
    a.reset()
    b.reset()
    view = b.device_view()
    assert view['obs'].shape == (n, b.n_variables) and view['in_shares'].shape == (n, b.n_slices + 1)
    oracles = []
    for r in range(4):
        o = po.OracleEnv(mk(1), fading)
        o.set_seed(replica_seed(seed, r))
        o.reset()
        oracles.append(o)
    own = hip.buffer(n * b.n_slices * 4)
    rng = np.random.default_rng(17 + scenario)
    for i in range(steps):
        acts = _valid_actions(rng, n, a.n_prbs, a.n_slices)
        host = a.step(acts)
        if i % 2 == 0:
            b.step_device(view['in_prbs'].set(acts))                           # kind inferred: int32 [n, S]
        else:
            hip.upload(own, acts)
            b.step_device(DeviceArray(own.value, acts.shape, np.int32), kind=_lib.RS_ACT_PRBS)
        dev = _read(b, view)
        _same(host, dev, acts)
        assert dev['l1_info'].tobytes() == a.l1_info().tobytes()
        assert dev['obs_norm'].tobytes() == normalise_obs(host[0]).tobytes()
        for r, o in enumerate(oracles):
            out = o.step(acts[r])
            assert dev['obs'][r].tobytes() == out['obs'].tobytes(), (i, r)
            assert dev['reward'][r] == out['reward'] and (dev['violations'][r] == out['violations']).all()
    assert b.rejected_rows() == 0
    b.synchronize()
    assert hip.free(own) == 0
    a.close()
    b.close()


def _shares(rng, n, W, n_prbs, i):
    s = (rng.random((n, W)) - 0.2).astype(np.float32)       # rows with negatives: abs() is taken
    s[0] = 0.0                                              # the all-zero row: t = 1
    counts = rng.multinomial(n_prbs, [1.0 / W] * W, size=4).astype(np.float32)
    s[1:5] = counts * np.float32(0.37 + 0.01 * i)           # exact-boundary rows: n_prbs * a_i / t sits on an integer
    s[5] = counts[0]
    s[6, :-1] = 0.0                                         # everything unused
    s[7, 1:] = 0.0                                          # the whole carrier to slice 0
    return s


@pytest.mark.parametrize('n_embb', [5, 7])
def test_device_report_wrapper_matches_host_wrapper(fading, tmp_path, n_embb):
    from ranslice.config import make_config
    from ranslice.device_io import DeviceArray
    from ranslice.report import DeviceReportWrapper, VecReportWrapper
    from ranslice.vec_env import VecRanSlice
    n, steps, seed = 64, 10, 930 + n_embb
    mk = lambda: make_config(0, n_envs=n, n_embb=n_embb)
    a = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    b = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    pa, pb = str(tmp_path) + '/host/', str(tmp_path) + '/dev/'
    wa = VecReportWrapper(a, steps=steps, control_steps=5, env_id=2, path=pa)
    wb = DeviceReportWrapper(b, steps=steps, control_steps=5, env_id=2, path=pb)
    oa, ob = wa.reset(), wb.reset()
    assert isinstance(ob, DeviceArray) and ob.get().tobytes() == oa.tobytes()
    view = b.device_view()
    rng = np.random.default_rng(5 + n_embb)

    def one(i):
        s = _shares(rng, n, n_embb + 1, a.n_prbs, i)
        obs, rew, done, info = wa.step(s)
        dobs, drew, ddone, dinfo = wb.step(view['in_shares'].set(s))
        assert isinstance(dobs, DeviceArray) and isinstance(drew, DeviceArray) and dinfo == {0: 0} and not ddone.any()
        got = dobs.get()
        assert got.dtype == obs.dtype == np.float32 and got.tobytes() == obs.tobytes(), i
        assert drew.get().tobytes() == rew.tobytes(), i
    for i in range(steps):
        one(i)
    f, g = np.load(pa + 'history_2.npz'), np.load(pb + 'history_2.npz')

    def same_npz(f, g, cols):
        assert sorted(g.files) == sorted(f.files) == ['resources', 'reward', 'violation']
        for k in f.files:
            assert g[k].dtype == f[k].dtype and g[k].shape == f[k].shape == (n, cols), k
            assert g[k].tobytes() == f[k].tobytes(), k
    same_npz(f, g, steps)
    assert f['resources'].any() and f['reward'].any()
    wa.set_evaluation(4, change_name=True)
    wb.set_evaluation(4, change_name=True)
    assert wb.steps == wa.steps == steps + 4 and wb.step_counter == wa.step_counter == steps
    for i in range(steps, steps + 4):
        one(i)
    wa.save_results()
    wb.save_results()
    same_npz(np.load(pa + 'evaluation_2.npz'), np.load(pb + 'evaluation_2.npz'), steps + 4)
    v, r, res, n_rec = wb.histories()
    assert n_rec == steps + 4
    assert v.tobytes() == wa.violation_history.tobytes() and r.tobytes() == wa.reward_history.tobytes()
    assert res.tobytes() == wa.action_history.tobytes()
    assert b.rejected_rows() == 0
    a.close()
    b.close()


def test_index_step_matches_table_rows(fading):
    from ranslice.config import make_config
    from ranslice.report import dqn_action_table
    from ranslice.vec_env import VecRanSlice
    n, seed = 64, 77
    a = VecRanSlice(n_envs=n, cfg=make_config(3, n_envs=n), fading=fading, seed=seed)
    b = VecRanSlice(n_envs=n, cfg=make_config(3, n_envs=n), fading=fading, seed=seed)
    a.reset()
    b.reset()
    view = b.device_view()
    from ranslice._lib import RanSliceError, RS_ESTATE
    with pytest.raises(RanSliceError) as e:
        b.step_device(view['in_index'])                     # no table yet
    assert e.value.code == RS_ESTATE
    table = dqn_action_table(70, 2)
    with pytest.raises(ValueError):
        b.set_action_table(table[:, :1])
    b.set_action_table(table)
    rng = np.random.default_rng(3)
    for i in range(8):
        idx = rng.integers(0, len(table), size=n).astype(np.int64)
        host = a.step(table[idx])
        b.step_device(view['in_index'].set(idx))
        _same(host, _read(b, view), table[idx])
    assert b.rejected_rows() == 0
    a.close()
    b.close()


def test_refused_rows_step_with_zeros_and_are_counted(fading):
    from ranslice import _lib
    from ranslice.config import make_config
    from ranslice.report import dqn_action_table
    from ranslice.vec_env import VecRanSlice
    n, seed = 64, 505
    mk = lambda: make_config(3, n_envs=n)
    a = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    b = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    a.reset()
    b.reset()
    view = b.device_view()
    table = dqn_action_table(70, 2)
    b.set_action_table(table)
    rng = np.random.default_rng(8)
    refused = 0
    for i in range(6):
        acts = _valid_actions(rng, n, 70, 2)
        bad = acts.copy()
        bad[3] = [-1, 10]                                    # a negative entry
        bad[10] = [35, 36]                                   # sum = n_prbs + 1
        bad[11] = [70, 0]                                    # sum = n_prbs: fine
        ref = bad.copy()
        ref[3] = 0
        ref[10] = 0
        host = a.step(ref)
        b.step_device(view['in_prbs'].set(bad), kind=_lib.RS_ACT_PRBS)
        refused += 2
        _same(host, _read(b, view), ref)
        assert b.rejected_rows() == refused
        idx = rng.integers(0, len(table), size=n).astype(np.int64)
        bad_idx = idx.copy()
        bad_idx[5] = -1
        bad_idx[6] = len(table)
        bad_idx[7] = len(table) - 1
        ref = table[np.clip(bad_idx, 0, len(table) - 1)].copy()
        ref[5] = 0
        ref[6] = 0
        host = a.step(ref)
        b.step_device(view['in_index'].set(bad_idx))
        refused += 2
        _same(host, _read(b, view), ref)
        assert b.rejected_rows() == refused
    with pytest.raises(_lib.RanSliceError) as e:
        b._check(b.L.rs_step_device(b.h, 7, C.c_void_p(view['in_prbs'].ptr), None))
    assert e.value.code == _lib.RS_EINVAL
    b.reset()
    assert b.rejected_rows() == 0                            # "since rs_reset"
    c = VecRanSlice(n_envs=4, cfg=make_config(3, n_envs=4), fading=fading, seed=1)
    with pytest.raises(_lib.RanSliceError) as e:
        c.step_device(c.device_view()['in_prbs'])            # before reset
    assert e.value.code == _lib.RS_ESTATE
    for env in (a, b, c):
        env.close()


def test_checkpoint_and_fork_are_unchanged_by_the_view(fading):
    """the new buffers are no region of the saved state: a handle that used the device path saves and loads blobs of the
    size a fresh handle does, and rs_fork between such handles still works"""
    from ranslice.config import make_config
    from ranslice.vec_env import VecRanSlice
    n = 16
    a = VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=fading, seed=9)
    b = VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=fading, seed=9)
    a.reset()
    b.reset()
    size0 = a.save_state().size
    view = a.device_view()
    acts = _valid_actions(np.random.default_rng(1), n, 200, 5)
    a.step_device(view['in_prbs'].set(acts))
    blob = a.save_state()
    assert blob.size == size0
    b.load_state(blob)                                       # b never created its view
    acts2 = _valid_actions(np.random.default_rng(2), n, 200, 5)
    ha, hb = a.step(acts2), b.step(acts2)
    assert ha[0].tobytes() == hb[0].tobytes() and ha[1].tobytes() == hb[1].tobytes()
    b.fork_from(a, np.arange(n, dtype=np.int32)[::-1].copy())
    a.step_device(view['in_prbs'].set(acts))
    hb = b.step(acts[::-1].copy())
    assert view['obs'].get()[::-1].tobytes() == hb[0].tobytes()
    a.close()
    b.close()


def test_stream_ordering_against_a_second_stream(fading):
    """the actions are produced on a second stream (behind a long fill, so that they are late) and the outputs are read on
    it; nothing waits in between -- the two events of rs_step_device are the only ordering"""
    from ranslice import _lib
    from ranslice.config import make_config
    from ranslice.vec_env import VecRanSlice
    hip = Hip()
    n, steps, seed = 64, 3, 61
    mk = lambda: make_config(2, n_envs=n)                    # mMTC slices: the step forks to its side stream
    a = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    b = VecRanSlice(n_envs=n, cfg=mk(), fading=fading, seed=seed)
    a.reset()
    b.reset()
    view = b.device_view()
    S, V = b.n_slices, b.n_variables
    s2 = C.c_void_p()
    assert hip.stream_create(C.byref(s2), 1) == 0            # hipStreamNonBlocking
    rng = np.random.default_rng(23)
    acts = [_valid_actions(rng, n, a.n_prbs, S) for _ in range(steps)]
    staged = [hip.buffer(n * S * 4) for _ in range(steps)]
    for p, x in zip(staged, acts):
        hip.upload(p, x)
    own = hip.buffer(n * S * 4)
    hip.upload(own, np.full((n, S), -1, dtype=np.int32))     # rows that would be refused if the step ran early
    big_bytes = 512 << 20
    big = hip.buffer(big_bytes)
    obs = [np.zeros((n, V), dtype=np.float32) for _ in range(steps)]
    rew = [np.zeros(n, dtype=np.float64) for _ in range(steps)]
    for i in range(steps):
        assert hip.memset_async(big, i, big_bytes, s2) == 0
        assert hip.memcpy_async(own, staged[i], n * S * 4, 3, s2) == 0          # device to device, by a kernel on s2
        b.step_device(own.value, kind=_lib.RS_ACT_PRBS, stream=s2.value)
        assert hip.memcpy_async(obs[i].ctypes.data_as(C.c_void_p), C.c_void_p(view['obs'].ptr), obs[i].nbytes, 2, s2) == 0
        assert hip.memcpy_async(rew[i].ctypes.data_as(C.c_void_p), C.c_void_p(view['reward'].ptr), rew[i].nbytes, 2, s2) == 0
        assert hip.memset_async(own, 0xff, n * S * 4, s2) == 0                  # spoil the buffer again (-1 everywhere)
    assert hip.stream_sync(s2) == 0
    for i in range(steps):
        o, r, _, _ = a.step(acts[i])
        assert obs[i].tobytes() == o.tobytes(), i
        assert rew[i].tobytes() == r.tobytes(), i
    assert b.rejected_rows() == 0
    b.stream_join(s2.value)
    assert hip.stream_sync(s2) == 0
    b.synchronize()
    for p in staged + [own, big]:
        assert hip.free(p) == 0
    assert hip.stream_destroy(s2) == 0
    a.close()
    b.close()


def _need_torch():
    # (found, not imported: torch brings a HIP runtime of its own, which has to be the first one a process loads --
    # the torch cases therefore run in a child process that imports torch before the library)
    if importlib.util.find_spec('torch') is None:
        pytest.skip('torch is not installed')


TORCH_CASE = r'''
import os, sys
import torch
import numpy as np
sys.path[:0] = [%(root)r, os.path.join(%(root)r, 'network-slicing_amd')]
from ranslice.config import make_config
from ranslice.report import DeviceReportWrapper, VecReportWrapper
from ranslice.vec_env import VecRanSlice
g = np.load(os.path.join(%(root)r, 'tests', 'golden', 'fading_small.npz'))
fading = [g['t0'], g['t1'], g['t2']]
n = 64
a = VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=fading, seed=31)
b = VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=fading, seed=31)
wa = VecReportWrapper(a, steps=8, control_steps=1000, path=%(tmp)r + '/h/')
wb = DeviceReportWrapper(b, steps=8, control_steps=1000, path=%(tmp)r + '/d/')
wa.reset()
view = b.device_view()
obs_t = torch.as_tensor(wb.reset(), device='cuda')
assert obs_t.data_ptr() == view['obs_norm'].ptr, (obs_t.data_ptr(), view['obs_norm'].ptr)
assert obs_t.shape == (n, 50) and obs_t.dtype == torch.float32
rew_t = torch.as_tensor(view['reward'], device='cuda')
assert rew_t.data_ptr() == view['reward'].ptr and rew_t.dtype == torch.float64
gen = torch.Generator(device='cuda').manual_seed(5)
for i in range(8):
    shares = torch.rand((n, 6), device='cuda', generator=gen) - 0.2
    wb.step(shares)
    o = obs_t.cpu().numpy()                                  # on torch's stream, which the step made wait
    r = rew_t.cpu().numpy()
    ho, hr, _, _ = wa.step(shares.cpu().numpy())
    assert o.tobytes() == ho.tobytes(), i
    assert r.tobytes() == hr.tobytes(), i
v, r, res, n_rec = wb.histories()
assert n_rec == 8 and r.tobytes() == wa.reward_history.tobytes() and res.tobytes() == wa.action_history.tobytes()
a.close(); b.close()
print('torch case ok')
'''


def test_torch_tensor_over_the_view(tmp_path):
    _need_torch()
    script = tmp_path / 'torch_case.py'
    script.write_text(TORCH_CASE % dict(root=ROOT, tmp=str(tmp_path)))
    p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert 'torch case ok' in p.stdout


def test_example_torch_device_policy(tmp_path):
    _need_torch()
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'torch_device_policy.py'), '--envs', '64', '--steps',
                        '20', '--check', '20', '--fading', os.path.join(ROOT, 'tests', 'golden', 'fading_small.npz'),
                        '--path', str(tmp_path) + '/'], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    f = np.load(str(tmp_path) + '/history_1.npz')
    assert f['reward'].shape == (64, 20) and f['violation'].dtype == np.int16
