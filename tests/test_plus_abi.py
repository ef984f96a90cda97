"""Projectron++ at the C ABI and on the Python classes (no GPU needed): kb_set_algorithm / kb_get_algorithm are declared, exported
and bound; ProjectronPlus and VecKBRL.set_algorithm exist; KBRL_Control refuses ProjectronPlus learners before it touches a device."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_algorithm', 'kb_get_algorithm')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_algorithm(kb_handle* k, int32_t alg);' in text
    assert 'int kb_get_algorithm(kb_handle* k, int32_t* alg);' in text
    assert re.search(r'#define KB_ALG_PROJECTRON 0\b', text) and re.search(r'#define KB_ALG_PROJECTRON_PLUS 1\b', text)
    # the signatures the branch codes 3 and 4 arrive through are what they were
    assert 'int kb_update(kb_handle* k, int e, int s, const double* x, int32_t y, int32_t* branch, double* delta);' in text


def test_listed_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_set_algorithm.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.kb_get_algorithm.argtypes] == ['c_void_p', 'LP_c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_algorithm(None, 1) == _lib.RS_EINVAL and L.kb_get_algorithm(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import kbrl_dev
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    from algorithms.projectron import Projectron, ProjectronPlus
    assert kbrl_dev.ALGORITHMS == {'projectron': 0, 'projectron_plus': 1}
    assert callable(VecKBRL.set_algorithm) and isinstance(VecKBRL.algorithm, property)
    assert list(inspect.signature(VecKBRL.set_algorithm).parameters) == ['self', 'algorithm']
    assert inspect.signature(VecKBRL.__init__).parameters['algorithm'].default == 'projectron'
    for m in ('update', 'fit'):
        assert 'margin update' in getattr(VecKBRL, m).__doc__
    # an unknown name never reaches the library; the shared-dictionary class refuses Projectron++ by name
    with pytest.raises(ValueError):
        VecKBRL(1, [3], 200, algorithm='perceptron')
    with pytest.raises(ValueError):
        VecKBRL.set_algorithm(object.__new__(VecKBRL), 'perceptron')
    with pytest.raises(ValueError, match='projectron_plus'):
        SharedVecKBRL(1, [3], 200, algorithm='projectron_plus')
    # the reference's surface (projectron.py:66-107): a Projectron whose update is the margin rule
    assert issubclass(ProjectronPlus, Projectron)
    assert Projectron.ALGORITHM == 'projectron' and ProjectronPlus.ALGORITHM == 'projectron_plus'
    assert list(inspect.signature(ProjectronPlus.__init__).parameters)[:3] == ['self', 'kernel', 'eta']
    for m in ('predict', 'update', 'fit', 'decision_function', 'get_set_size'):
        assert getattr(ProjectronPlus, m) is getattr(Projectron, m)
    assert isinstance(ProjectronPlus.Kinv, property)


def test_kbrl_control_refuses_projectron_plus_learners():
    """neither trained silently as Projectron nor failing deep inside: a ValueError that names the supported route, raised before
    any device handle exists"""
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import Projectron, ProjectronPlus, SVvariable
    from kbrl_control import KBRL_Control, Learner
    learners = [Learner(Projectron(GaussianKernel(SVvariable(), 1.0)), slice(0, 10), 100, 3),
                Learner(ProjectronPlus(GaussianKernel(SVvariable(), 1.0)), slice(10, 13), 100, 3)]
    with pytest.raises(ValueError) as e:
        KBRL_Control(learners, 200)
    msg = str(e.value)
    assert 'ProjectronPlus' in msg and 'VecKBRL.fit' in msg and 'augmented_samples' in msg and '[1]' in msg
    assert all(not h.algorithm._bound() for h in learners)
