"""kb_fit / kb_score at the C ABI, on VecKBRL and on Projectron (no GPU needed): declared, exported, bound; the methods exist."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_fit', 'kb_score', 'kb_fit_time_ms')


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    text = re.sub(r'\s+', ' ', text)
    assert ('int kb_fit(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, const int8_t* y, '
            'int32_t chunk, int32_t* y_pred, double* f, int32_t* branch, double* delta, int32_t* m_after);') in text
    assert ('int kb_score(kb_handle* k, const int32_t* task, int32_t n, const int64_t* first, const double* x, double* f, '
            'int32_t* y_pred);') in text
    assert 'int kb_fit_time_ms(kb_handle* k, double ms[2], uint64_t work[4]);' in text


def test_listed_among_the_exports():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS


def test_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_fit.argtypes] == ['c_void_p', 'LP_c_int', 'c_int', 'LP_c_long', 'LP_c_double', 'LP_c_byte', 'c_int',
                                                       'LP_c_int', 'LP_c_double', 'LP_c_int', 'LP_c_double', 'LP_c_int']
    assert [t.__name__ for t in L.kb_score.argtypes] == ['c_void_p', 'LP_c_int', 'c_int', 'LP_c_long', 'LP_c_double', 'LP_c_double',
                                                         'LP_c_int']
    assert [t.__name__ for t in L.kb_fit_time_ms.argtypes] == ['c_void_p', 'LP_c_double', 'LP_c_ulong']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int


def test_python_surface():
    from ranslice import kbrl_dev
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    from algorithms.projectron import Projectron
    for m in ('fit', 'score', 'fit_time_ms'):
        assert callable(getattr(VecKBRL, m))
    assert list(inspect.signature(VecKBRL.fit).parameters) == ['self', 'learners', 'X', 'y', 'chunk']
    assert inspect.signature(VecKBRL.fit).parameters['chunk'].default == 0
    assert list(inspect.signature(VecKBRL.score).parameters) == ['self', 'learners', 'X']
    # shared dictionaries: score is the inherited one, fit is refused before anything reaches the device
    assert SharedVecKBRL.score is VecKBRL.score and SharedVecKBRL.fit is not VecKBRL.fit
    from ranslice import _lib
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.fit(object.__new__(SharedVecKBRL), [(0, 0)], [[[0.0] * 4]], [[1]])
    assert e.value.code == _lib.RS_ESTATE
    assert callable(kbrl_dev.augmented_samples)
    assert list(inspect.signature(kbrl_dev.augmented_samples).parameters) == ['state', 'action', 'labels', 'dims', 'n_prbs']
    for m in ('fit', 'decision_function'):
        assert callable(getattr(Projectron, m))
        assert 'BUILD-DEFINED' in getattr(Projectron, m).__doc__
    for m in ('predict', 'update'):   # the reference's surface is what it was
        assert callable(getattr(Projectron, m))
    assert list(inspect.signature(Projectron.update).parameters) == ['self', 'x', 'y']
