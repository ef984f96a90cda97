"""kb_fit's wide path at the C ABI and on the Python classes (no GPU needed): kb_set_fit_wide / kb_get_fit_wide / kb_fit_wide_info are
declared, exported and bound; VecKBRL.set_fit_wide, fit_wide, fit_wide_info and Projectron.fit(..., wide=) exist; the
shared-dictionary class refuses the setter before it touches the library."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_fit_wide', 'kb_get_fit_wide', 'kb_fit_wide_info')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_fit_wide(kb_handle* k, int32_t min_landmarks, int32_t window);' in text
    assert 'int kb_get_fit_wide(kb_handle* k, int32_t* min_landmarks, int32_t* window);' in text
    assert 'int kb_fit_wide_info(kb_handle* k, uint64_t work[4]);' in text
    # kb_fit's own signature and kb_fit_time_ms's are what they were
    assert ('int kb_fit(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, const int8_t* y, '
            'int32_t chunk, int32_t* y_pred, double* f, int32_t* branch, double* delta, int32_t* m_after);') in text
    assert 'int kb_fit_time_ms(kb_handle* k, double ms[2], uint64_t work[4]);' in text
    # the header says that Projectron++ stays narrow
    assert re.search(r'Projectron\+\+ mode.{0,80}narrow path', re.sub(r'\s+', ' ', raw))


def test_listed_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_set_fit_wide.argtypes] == ['c_void_p', 'c_int', 'c_int']
    assert [t.__name__ for t in L.kb_get_fit_wide.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_int']
    assert [t.__name__ for t in L.kb_fit_wide_info.argtypes] == ['c_void_p', 'LP_c_ulong']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_fit_wide(None, 2, 0) == _lib.RS_EINVAL
    assert L.kb_get_fit_wide(None, None, None) == _lib.RS_EINVAL
    assert L.kb_fit_wide_info(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    from algorithms.projectron import Projectron, ProjectronPlus
    assert list(inspect.signature(VecKBRL.set_fit_wide).parameters) == ['self', 'min_landmarks', 'window']
    assert inspect.signature(VecKBRL.set_fit_wide).parameters['window'].default == 0
    assert isinstance(VecKBRL.fit_wide, property) and callable(VecKBRL.fit_wide_info)
    assert list(inspect.signature(Projectron.fit).parameters) == ['self', 'X', 'y', 'wide']
    assert inspect.signature(Projectron.fit).parameters['wide'].default is None
    assert ProjectronPlus.fit is Projectron.fit
    assert list(inspect.signature(VecKBRL.fit).parameters) == ['self', 'learners', 'X', 'y', 'chunk']
    # the shared-dictionary class refuses by itself, as the library does: no handle is needed to learn that
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_fit_wide(object.__new__(SharedVecKBRL), 64)
    assert e.value.code == _lib.RS_ESTATE
