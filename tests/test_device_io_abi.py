"""Device-resident policy interface, the parts that need no GPU: the C ABI and its ctypes binding, DeviceArray's
__cuda_array_interface__, the DQN action table, and the simplex rule of rs_step_device (csrc/rs_policy_io.hip) in a
pure-Python mirror -- same operations, same order, scalar float64 -- against ranslice.report.simplex_to_prbs.  The mirror
is how numpy's summation order for 8- and 9-entry rows is pinned without a GPU."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = (
    'int rs_get_device_view(rs_handle* h, rs_device_view* out);',
    'int rs_step_device(rs_handle* h, int kind, const void* actions_device, void* caller_stream);',
    'int rs_stream_join(rs_handle* h, void* caller_stream);',
    'int rs_set_action_table(rs_handle* h, const int32_t* table /* host [n_actions][n_slices] */, int32_t n_actions);',
    'int rs_report_begin(rs_handle* h, int32_t steps);',
    'int rs_report_extend(rs_handle* h, int32_t eval_steps);',
    'int rs_report_fetch(rs_handle* h, int16_t* violation, double* reward, int16_t* resources, int32_t* n_recorded);',
    'int rs_device_copy(rs_handle* h, void* dst, const void* src, uint64_t bytes, int to_device);',
)
NAMES = [re.search(r'(rs_[a-z_]+)\(', p).group(1) for p in PROTOTYPES]


def _header():
    return open(os.path.join(ROOT, 'include', 'ranslice.h')).read()


def test_prototypes_are_declared_and_listed():
    from ranslice import _lib
    text = _header()
    flat = re.sub(r'\s+', ' ', text)
    for p in PROTOTYPES:
        assert re.sub(r'\s+', ' ', p) in flat, p
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    for name, val in (('RS_ACT_PRBS', 0), ('RS_ACT_SHARES', 1), ('RS_ACT_INDEX', 2)):
        assert re.search(r'#define %s\s+%d\b' % (name, val), text), name
        assert getattr(_lib, name) == val
    # the header says what is not checkpointed or forked, and that the host waits for nothing
    assert 'NOT part of a checkpoint' in text and 'NOT copied by rs_fork' in text
    assert 'THE HOST WAITS FOR NOTHING' in text


def test_exports_are_bound_with_the_stated_argtypes():
    from ranslice import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libranslice.so not built (python __graft_entry__.py build)')
    L = _lib.load()
    vp, ip = C.c_void_p, C.POINTER(C.c_int32)
    sp, dp = C.POINTER(C.c_int16), C.POINTER(C.c_double)
    want = {
        'rs_get_device_view': [vp, C.POINTER(_lib.RsDeviceView)],
        'rs_step_device': [vp, C.c_int, vp, vp],
        'rs_stream_join': [vp, vp],
        'rs_set_action_table': [vp, ip, C.c_int32],
        'rs_report_begin': [vp, C.c_int32],
        'rs_report_extend': [vp, C.c_int32],
        'rs_report_fetch': [vp, sp, dp, sp, ip],
        'rs_device_copy': [vp, vp, vp, C.c_uint64, C.c_int],
    }
    for n in NAMES:
        f = getattr(L, n)
        assert list(f.argtypes) == want[n], n
        assert f.restype is C.c_int, n


def test_device_view_struct_matches_header():
    from ranslice._lib import RsDeviceView
    body = re.search(r'typedef struct rs_device_view \{(.*?)\} rs_device_view;', _header(), flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names, kinds = [], []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r'^(int32_t|int64_t|double|float|void)\s*(\*?)\s*(.*)$', decl)
        assert m, decl
        for name in m.group(3).split(','):
            names.append(name.strip())
            kinds.append('ptr' if m.group(2) else m.group(1))
    assert names == [f[0] for f in RsDeviceView._fields_]
    for (fname, ftype), kind in zip(RsDeviceView._fields_, kinds):
        assert ftype is (C.c_void_p if kind == 'ptr' else C.c_int32), fname
    assert C.sizeof(RsDeviceView) == 16 + 13 * C.sizeof(C.c_void_p)


def test_device_array_cuda_array_interface():
    from ranslice.device_io import DeviceArray
    import ranslice.device_io as dio
    assert 'import torch' not in open(dio.__file__).read()
    for dt, ts in ((np.float32, '<f4'), (np.int32, '<i4'), (np.int64, '<i8'), (np.float64, '<f8')):
        a = DeviceArray(0x7f0012340000, (64, 5), dt)
        cai = a.__cuda_array_interface__
        assert cai['shape'] == (64, 5) and cai['typestr'] == ts and cai['version'] == 3
        assert cai['data'] == (0x7f0012340000, False)        # read-write
        assert 'stream' not in cai and cai.get('strides') is None
        assert a.nbytes == 64 * 5 * np.dtype(dt).itemsize and a.data_ptr() == 0x7f0012340000
    with pytest.raises(ValueError):
        DeviceArray(16, (2,), np.float32).get()            # no owner handle to copy through


def test_dqn_action_table():
    from ranslice.report import dqn_action_table
    n_prbs = 70
    actions = []                                             # wrapper.py:143-149
    a = list(range(0, 51, 2))
    for (a1, a2) in itertools.product(a, a):
        if a1 + a2 <= n_prbs:
            actions.append(np.array([a1, a2], dtype=np.int16))
    t = dqn_action_table(70, 2)
    assert t.dtype == np.int32 and t.shape == (len(actions), 2)
    assert (t == np.array(actions)).all()
    full = [p for p in itertools.product(a, a)]
    t40 = dqn_action_table(40, 2)
    assert [tuple(r) for r in t40] == [p for p in full if p[0] + p[1] <= 40]
    assert len(full) - len(t40) == sum(1 for p in full if p[0] + p[1] > 40) > 0
    t3 = dqn_action_table(30, 3, granularity=10, max_prbs=31)
    assert [tuple(r) for r in t3] == [p for p in itertools.product(range(0, 31, 10), repeat=3) if sum(p) <= 30]


# ---- the device's simplex rule, operation for operation (rs_policy_io.hip: policy_front_kernel, RS_ACT_SHARES)

def mirror_sum(v, pairwise=True):
    W = len(v)
    if W < 8 or not pairwise:
        t = 0.0
        for x in v:
            t = t + x
    else:
        t = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
        for x in v[8:]:
            t = t + x
    return t


def mirror_row(row, n_prbs, n_slices, pairwise=True):
    v = [abs(float(x)) for x in row]                        # float32 -> float64 is exact
    t = mirror_sum(v, pairwise)
    if t == 0.0:
        t = 1.0
    return [int(math.floor((float(n_prbs) * v[s]) / t)) for s in range(n_slices)]


def mirror(a32, n_prbs, n_slices, pairwise=True):
    assert a32.dtype == np.float32
    return np.array([mirror_row(r, n_prbs, n_slices, pairwise) for r in a32.tolist()], dtype=np.int32)


def _mismatches(a32, n_prbs, pairwise=True):
    from ranslice.report import simplex_to_prbs
    S = a32.shape[1] - 1
    want = simplex_to_prbs(np.ascontiguousarray(a32), n_prbs, S)
    assert want.dtype == np.int32 and want.shape == (a32.shape[0], S)
    return int((mirror(a32, n_prbs, S, pairwise) != want).any(axis=1).sum())


def test_shares_rule_on_the_g12_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g12_report_wrapper.npz'))
    a32 = g['action'].astype(np.float32)
    assert a32.shape[1] == 6
    assert _mismatches(a32, 200) == 0


@pytest.mark.parametrize('width', [3, 6, 8, 9])
def test_shares_rule_random_rows(width):
    rng = np.random.default_rng(100 + width)
    n = 100000
    a32 = (rng.random((n, width)) - 0.2).astype(np.float32)   # negative entries: abs() is taken
    a32[:7] = 0.0                                             # t = 0 -> 1
    a32[7:14, 1:] = 0.0
    assert _mismatches(a32, 200) == 0
    assert _mismatches(a32, 70) == 0


@pytest.mark.parametrize('width', [3, 6, 8, 9])
def test_shares_rule_adversarial_rows(width):
    """integer counts that sum to n_prbs, times a random float32 scale: n_prbs * a_i / t sits on an integer, so one ulp
    in the row sum flips a floor"""
    rng = np.random.default_rng(200 + width)
    n = 100000
    for n_prbs in (200, 70):
        counts = rng.multinomial(n_prbs, [1.0 / width] * width, size=n).astype(np.float32)
        scale = rng.random((n, 1)).astype(np.float32) + np.float32(1e-3)
        a32 = (counts * scale).astype(np.float32)
        a32 *= rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=a32.shape)
        assert _mismatches(a32, n_prbs) == 0


@pytest.mark.parametrize('width', [8, 9])
def test_shares_rule_pins_the_summation_order(width):
    """rows whose entries span sixty binary orders of magnitude: the sum of the widened float32 values is no longer exact
    and depends on the order.  The mirror's order (numpy's for a contiguous axis) gives numpy's row sum in every row and
    the same PRBs; the plain left-to-right sum gives another sum in some rows -- so these rows tell the two apart, and the
    former is what the kernel must do."""
    rng = np.random.default_rng(300 + width)
    n = 100000
    a32 = (rng.standard_normal((n, width)) * np.exp2(rng.integers(-30, 30, (n, width)))).astype(np.float32)
    assert _mismatches(a32, 200) == 0
    a = np.abs(a32.astype(np.float64))
    t = a.sum(axis=-1, keepdims=True)[:, 0]
    rows = a.tolist()
    assert sum(1 for r, want in zip(rows, t.tolist()) if mirror_sum(r) != want) == 0
    assert sum(1 for r, want in zip(rows, t.tolist()) if mirror_sum(r, pairwise=False) != want) > 100


@pytest.mark.parametrize('width', [3, 6, 7])
def test_shares_rule_wide_range_narrow_rows(width):
    rng = np.random.default_rng(400 + width)
    a32 = (rng.standard_normal((50000, width)) * np.exp2(rng.integers(-30, 30, (50000, width)))).astype(np.float32)
    assert _mismatches(a32, 200) == 0


def test_vec_env_infers_the_action_kind():
    """dtype / shape -> kind, and the refusals, on an object that never touches the library"""
    from ranslice import _lib
    from ranslice.device_io import DeviceArray, describe
    from ranslice.vec_env import VecRanSlice
    env = VecRanSlice.__new__(VecRanSlice)
    env.n_envs, env.n_slices, env.h = 64, 5, None
    assert env._action_kind((64, 5), np.dtype(np.int32)) == _lib.RS_ACT_PRBS
    assert env._action_kind((64, 6), np.dtype(np.float32)) == _lib.RS_ACT_SHARES
    assert env._action_kind((64,), np.dtype(np.int64)) == _lib.RS_ACT_INDEX
    for shape, dt in (((64, 6), np.int32), ((64, 5), np.float32), ((64, 6), np.float64), ((63,), np.int64)):
        with pytest.raises(ValueError):
            env._action_kind(shape, np.dtype(dt))

    class Strided:
        __cuda_array_interface__ = {'shape': (64, 6), 'typestr': '<f4', 'data': (4096, False), 'version': 3,
                                    'strides': (48, 4)}
    with pytest.raises(ValueError):
        describe(Strided())
    Strided.__cuda_array_interface__['strides'] = (24, 4)
    assert describe(Strided()) == (4096, (64, 6), np.dtype(np.float32))
    assert describe(DeviceArray(8192, (64,), np.int64)) == (8192, (64,), np.dtype(np.int64))
    with pytest.raises(ValueError):
        env.step_device(Strided(), kind=_lib.RS_ACT_PRBS)    # float32 [64, 6] is not the PRB layout
    with pytest.raises(ValueError):
        env.step_device(12345)                               # a bare pointer needs a kind
