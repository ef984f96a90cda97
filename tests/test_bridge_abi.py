"""kb_unshare / kb_share / kb_bridge_time_ms at the C ABI and on the Python classes (no GPU needed): the symbols are declared
with the signatures that are bound, exported by both builds of the library, and shared_pool_bytes is the storage formula of
kb_kbrl.hip ("Storage") for dictionaries that keep both block triangles of Kinv."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_unshare', 'kb_share', 'kb_bridge_time_ms')


def _header():
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_declared_in_the_header():
    text = _header()
    assert re.search(r'int kb_unshare\(kb_handle\* dst, kb_handle\* src, const int32_t\* src_index\);', text)
    assert re.search(r'int kb_share\(kb_handle\* dst, kb_handle\* src, int32_t dict_agent, const int32_t\* ctl_index\);', text)
    assert re.search(r'int kb_bridge_time_ms\(kb_handle\* k, double\* ms, uint64_t bytes\[2\]\);', text)


def test_exported_by_both_builds_and_bound():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
    for path in (_lib.LIB_PATH, _lib.DEV_LIB_PATH):
        assert os.path.exists(path), '%s not built (python __graft_entry__.py build)' % os.path.basename(path)
        raw = C.CDLL(path)
        for n in NEW:
            assert hasattr(raw, n), (path, n)
    for L in (_lib.load(), _lib.load(dev=True)):
        assert [t.__name__ for t in L.kb_unshare.argtypes] == ['c_void_p', 'c_void_p', 'LP_c_int']
        assert [t.__name__ for t in L.kb_share.argtypes] == ['c_void_p', 'c_void_p', 'c_int', 'LP_c_int']
        assert [t.__name__ for t in L.kb_bridge_time_ms.argtypes] == ['c_void_p', 'LP_c_double', 'LP_c_ulong']
        for n in NEW:
            assert getattr(L, n).restype is C.c_int
    # the existing fork keeps its own entry point
    assert _lib.load().kb_fork is not _lib.load().kb_unshare


def test_python_surface():
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    p = inspect.signature(SharedVecKBRL.to_agents).parameters
    assert list(p) == ['self', 'index', 'capacity', 'pool_bytes', 'device']
    assert p['capacity'].default is None and p['pool_bytes'].default is None and p['device'].default is None
    p = inspect.signature(VecKBRL.to_shared).parameters
    assert list(p) == ['self', 'agent', 'n_envs', 'ctl_index', 'budget', 'max_rounds', 'first_env', 'pool_bytes']
    assert (p['ctl_index'].default, p['budget'].default, p['max_rounds'].default, p['first_env'].default, p['pool_bytes'].default) == \
        (None, 64, 4, 0, None)


@pytest.mark.parametrize('m', [0, 1, 64, 65, 129, 1024])
def test_shared_pool_bytes_is_the_storage_formula(m):
    """shell b of a shared dictionary = one vector page (30 rows x 64 doubles) + 2 b + 1 tiles of 64 x 64 doubles; the pool starts
    with 64 unused doubles.  Summed shell by shell here, in closed form in the helper."""
    from ranslice.kbrl_dev import fork_pool_bytes, shared_pool_bytes
    shells = (m + 63) // 64
    want = 64 * 8 + sum(30 * 64 * 8 + (2 * b + 1) * 64 * 64 * 8 for b in range(shells))
    assert shared_pool_bytes([m]) == want
    assert shared_pool_bytes(np.array([[m, 0], [m, m]])) == 64 * 8 + 3 * (want - 64 * 8)
    # against the triangle's helper: both hold the pages and the lower tiles; one adds the upper tiles, the other 1 KB per tile
    tiles_lo = shells * (shells + 1) // 2
    assert shared_pool_bytes([m]) - 32768 * (shells * shells - tiles_lo) == fork_pool_bytes([m]) - 1024 * tiles_lo
