"""kb_prune at the C ABI, on VecKBRL and in the tools (no GPU needed): declared, exported, bound; the evaluators' defaults are
what they were."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_prune', 'kb_get_pruned', 'kb_prune_time_ms', 'kb_get_prune_work')


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    assert re.search(r'int kb_prune\(kb_handle\* k, int32_t target, uint64_t\* removed_total\);', text)
    assert re.search(r'int kb_get_pruned\(kb_handle\* k, int64_t\* removed\s*\);', text)
    assert re.search(r'int kb_prune_time_ms\(kb_handle\* k, double ms\[3\], int64_t n\[3\]\);', text)
    assert re.search(r'int kb_get_prune_work\(kb_handle\* k, uint64_t work\[2\]\);', text)


def test_listed_among_the_exports():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS


def test_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_prune.argtypes] == ['c_void_p', 'c_int', 'LP_c_ulong']
    assert [t.__name__ for t in L.kb_get_pruned.argtypes] == ['c_void_p', 'LP_c_long']
    assert [t.__name__ for t in L.kb_prune_time_ms.argtypes] == ['c_void_p', 'LP_c_double', 'LP_c_long']
    assert [t.__name__ for t in L.kb_get_prune_work.argtypes] == ['c_void_p', 'LP_c_ulong']


def test_python_surface_and_defaults(tmp_path):
    from ranslice.kbrl_dev import VecKBRL
    import experiments_kbrl as ek
    for m in ('prune', 'pruned', 'prune_times_ms'):
        assert callable(getattr(VecKBRL, m))
    for f in (ek.BatchedEvaluator.__init__, ek.evaluate_grid):
        p = inspect.signature(f).parameters
        assert p['prune_to'].default is None and p['prune_every'].default is None
    with pytest.raises(ValueError):
        ek.BatchedEvaluator(0, [0.97, 0.99], steps=10, out_dir=str(tmp_path), prune_to=128)
