"""kb_fit's wide path for Projectron++ at the C ABI and on the Python classes (no GPU needed): kb_set_fit_wide_plus /
kb_get_fit_wide_plus are declared, exported and bound; VecKBRL.set_fit_wide_plus and fit_wide_plus exist; a ProjectronPlus carries
the plain attribute wide_plus; the shared-dictionary class refuses the setter before it touches the library."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_fit_wide_plus', 'kb_get_fit_wide_plus')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_fit_wide_plus(kb_handle* k, int32_t on);' in text
    assert 'int kb_get_fit_wide_plus(kb_handle* k, int32_t* on);' in text
    # kb_set_fit_wide keeps its signature and its meaning: the new mode has a switch of its own
    assert 'int kb_set_fit_wide(kb_handle* k, int32_t min_landmarks, int32_t window);' in text
    flat = re.sub(r'\s+', ' ', raw)
    assert re.search(r'kb_set_fit_wide_plus\(k, on\).{0,400}on = 0 \(the default\)', flat)
    assert 'whatever the setting -- nearly every sample' not in flat   # the sentence that said "narrow always" is gone


def test_listed_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_set_fit_wide_plus.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.kb_get_fit_wide_plus.argtypes] == ['c_void_p', 'LP_c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_fit_wide_plus(None, 1) == _lib.RS_EINVAL
    assert L.kb_get_fit_wide_plus(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import Projectron, ProjectronPlus, SVvariable
    assert list(inspect.signature(VecKBRL.set_fit_wide_plus).parameters) == ['self', 'on']
    assert inspect.signature(VecKBRL.set_fit_wide_plus).parameters['on'].default is True
    assert isinstance(VecKBRL.fit_wide_plus, property)
    # what the existing surface pins stays
    assert list(inspect.signature(VecKBRL.set_fit_wide).parameters) == ['self', 'min_landmarks', 'window']
    assert list(inspect.signature(Projectron.fit).parameters) == ['self', 'X', 'y', 'wide']
    assert ProjectronPlus.fit is Projectron.fit
    # the attribute: on a ProjectronPlus object, off by default; a Projectron has none (no device is touched by the constructors)
    p = ProjectronPlus(GaussianKernel(SVvariable(), 1.0))
    assert p.wide_plus is False and 'wide_plus' in vars(p)
    assert not hasattr(Projectron(GaussianKernel(SVvariable(), 1.0)), 'wide_plus')
    # the shared-dictionary class refuses by itself, as the library does: no handle is needed to learn that
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_fit_wide_plus(object.__new__(SharedVecKBRL), True)
    assert e.value.code == _lib.RS_ESTATE
