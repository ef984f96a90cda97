"""Lanes of the step loop, the parts that need no GPU: the two functions of the C ABI, their ctypes binding and the
wrappers of VecRanSlice."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = (
    'int rs_set_lanes(rs_handle* h, int n);',
    'int rs_get_lane_info(rs_handle* h, double out[4]);',
)
NAMES = [re.search(r'(rs_[a-z_]+)\(', p).group(1) for p in PROTOTYPES]


def test_prototypes_are_declared_and_listed():
    from ranslice import _lib
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    flat = re.sub(r'\s+', ' ', text)
    for p in PROTOTYPES:
        assert p in flat, p
    for n in NAMES:
        assert n in _lib.EXPORTS, n
    # the header says what a step's timing sample is with lanes, and what the four numbers are
    assert 'SUM of its lanes' in text and '1 - union / sum' in text


def test_exports_are_bound_with_the_stated_argtypes():
    from ranslice import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libranslice.so not built (python __graft_entry__.py build)')
    L = _lib.load()
    want = {'rs_set_lanes': [C.c_void_p, C.c_int], 'rs_get_lane_info': [C.c_void_p, C.POINTER(C.c_double)]}
    for n in NAMES:
        f = getattr(L, n)
        assert list(f.argtypes) == want[n], n
        assert f.restype is C.c_int, n


def test_null_handle_and_bad_count_are_refused():
    """both functions check their arguments before they touch the device"""
    from ranslice import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libranslice.so not built (python __graft_entry__.py build)')
    L = _lib.load()
    out = (C.c_double * 4)()
    assert L.rs_set_lanes(None, 2) == _lib.RS_EINVAL
    assert L.rs_get_lane_info(None, out) == _lib.RS_EINVAL


def test_vec_env_wraps_both():
    from ranslice.vec_env import VecRanSlice

    class Lib:
        def __init__(self):
            self.calls = []

        def rs_set_lanes(self, h, n):
            self.calls.append(('set', n))
            return 0

        def rs_get_lane_info(self, h, out):
            out[0], out[1], out[2], out[3] = 2.0, 0.9, 0.6, 1.0 - 0.6 / 0.9
            return 0

    env = VecRanSlice.__new__(VecRanSlice)
    env.L, env.h = Lib(), None
    env.set_lanes(4)
    assert env.L.calls == [('set', 4)]
    lanes, total, union, hidden = env.lane_info()
    assert lanes == 2 and isinstance(lanes, int) and (total, union) == (0.9, 0.6) and abs(hidden - (1.0 - 0.6 / 0.9)) < 1e-15
