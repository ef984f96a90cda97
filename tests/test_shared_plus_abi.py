"""The shared-dictionary rounds' Projectron++ switch at the C ABI and on the Python class (no GPU needed):
kb_set_shared_plus / kb_get_shared_plus are declared, exported by both builds and bound; SharedVecKBRL has the keyword (default
False), the method and the property; algorithm='projectron_plus' keeps raising."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_shared_plus', 'kb_get_shared_plus')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_shared_plus(kb_handle* k, int32_t on);' in text
    assert 'int kb_get_shared_plus(kb_handle* k, int32_t* on);' in text
    flat = re.sub(r'\s+', ' ', raw)
    assert re.search(r'kb_set_shared_plus\(k, on\).{0,60}on = 0 \(the default\)', flat)
    # the header says that kb_get_algorithm does not name the fleet's rule, and that the ranks must agree on the switch
    assert re.search(r'kb_get_algorithm keeps answering KB_ALG_PROJECTRON on a shared handle', flat)
    assert re.search(r'Every rank of a group must have set the same kb_set_shared_plus value', flat)


def test_listed_exported_by_both_builds_and_bound():
    """the built libraries (build() of __graft_entry__.py makes them: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    for path in (_lib.LIB_PATH, os.path.join(os.path.dirname(_lib.LIB_PATH), 'libranslice_dev.so')):
        raw = C.CDLL(path)
        for n in NEW:
            assert hasattr(raw, n), (path, n)
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
    L = _lib.load()
    assert [t.__name__ for t in L.kb_set_shared_plus.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.kb_get_shared_plus.argtypes] == ['c_void_p', 'LP_c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_shared_plus(None, 1) == _lib.RS_EINVAL
    assert L.kb_get_shared_plus(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    assert inspect.signature(SharedVecKBRL.__init__).parameters['shared_plus'].default is False
    assert list(inspect.signature(SharedVecKBRL.set_shared_plus).parameters) == ['self', 'on']
    assert inspect.signature(SharedVecKBRL.set_shared_plus).parameters['on'].default is True
    assert isinstance(SharedVecKBRL.shared_plus, property)
    assert 'shared_plus' in SharedVecKBRL.__doc__ and 'y f < 1' in SharedVecKBRL.__doc__
    # the per-replica class has no such switch: its loop learns by the margin rule behind set_control_plus
    assert not hasattr(VecKBRL, 'set_shared_plus') and not hasattr(VecKBRL, 'shared_plus')
    # the algorithm keyword keeps raising, before any handle exists, and now names the switch
    with pytest.raises(ValueError, match='projectron_plus') as e:
        SharedVecKBRL(1, [3], 200, algorithm='projectron_plus')
    assert 'shared_plus=True' in str(e.value)
