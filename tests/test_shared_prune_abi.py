"""kb_shared_prune at the C ABI and on SharedVecKBRL (no GPU needed): declared, exported, bound; prune() is still the
per-replica call, which refuses shared handles."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    assert re.search(r'int kb_shared_prune\(kb_handle\* k, int32_t target, uint64_t\* removed_total\);', text)


def test_listed_among_the_exports():
    from ranslice import _lib
    assert 'kb_shared_prune' in _lib.EXPORTS and 'kb_shared_prune' in _lib.KB_EXPORTS


def test_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, 'kb_shared_prune')
    L = _lib.load()
    assert [t.__name__ for t in L.kb_shared_prune.argtypes] == ['c_void_p', 'c_int', 'LP_c_ulong']
    assert L.kb_shared_prune.restype is C.c_int


def test_python_surface():
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    assert callable(SharedVecKBRL.shrink) and 'shrink' in vars(SharedVecKBRL) and not hasattr(VecKBRL, 'shrink')
    assert SharedVecKBRL.prune is VecKBRL.prune
    for m in ('pruned', 'prune_times_ms'):
        assert getattr(SharedVecKBRL, m) is getattr(VecKBRL, m)
