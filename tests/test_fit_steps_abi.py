"""kb_fit_steps at the C ABI and on VecKBRL (no GPU needed): declared, exported, bound; the host checks of fit_steps refuse bad logs
before any handle exists."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    text = re.sub(r'\s+', ' ', text)
    assert ('int kb_fit_steps(kb_handle* k, const int32_t* agent, int32_t n, const int64_t* first , const float* state , '
            'const int32_t* action , const int32_t* labels , int32_t chunk, double* f_at, int32_t* y_at, int32_t* changed, '
            'int32_t* grown, int32_t* m_after);') in text


def test_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    assert 'kb_fit_steps' in _lib.EXPORTS and 'kb_fit_steps' in _lib.KB_EXPORTS
    assert hasattr(C.CDLL(_lib.LIB_PATH), 'kb_fit_steps')
    L = _lib.load()
    assert [t.__name__ for t in L.kb_fit_steps.argtypes] == ['c_void_p', 'LP_c_int', 'c_int', 'LP_c_long', 'LP_c_float', 'LP_c_int',
                                                             'LP_c_int', 'c_int', 'LP_c_double', 'LP_c_int', 'LP_c_int', 'LP_c_int',
                                                             'LP_c_int']
    assert L.kb_fit_steps.restype is C.c_int


def _no_handle(cls):
    """an object of the class that never met the library: fit_steps' checks need the shapes only"""
    from ranslice import kbrl_dev
    h = object.__new__(getattr(kbrl_dev, cls))
    h.n_envs, h.S, h.n_prbs, h.dims, h.nv, h.h = 3, 2, 6, [10, 3], 13, None
    return h


def test_bad_logs_are_refused_before_the_library_is_touched():
    from ranslice.kbrl_dev import VecKBRL
    assert list(inspect.signature(VecKBRL.fit_steps).parameters) == ['self', 'agents', 'state', 'action', 'labels', 'chunk']
    assert inspect.signature(VecKBRL.fit_steps).parameters['chunk'].default == 0
    h = _no_handle('VecKBRL')
    st, ac, lb = np.zeros((4, 13), dtype=np.float32), np.full((4, 2), 3), np.ones((4, 2), dtype=int)
    bad = [
        ([0], [st], [ac[:3]], [lb]),                      # ragged: 4 states, 3 actions
        ([0], [st], [ac], [lb[:, :1]]),                   # labels of one learner only
        ([0], [st[:, :12]], [ac], [lb]),                  # 12 state variables
        ([0, 1], [st], [ac], [lb]),                       # two agents, one log
        ([3], [st], [ac], [lb]),                          # no such agent
        ([0], [st], [ac], [np.where(np.eye(4, 2) > 0, 2, 1)]),        # a label of 2
        ([0], [st], [np.where(np.eye(4, 2) > 0, 7, 3)], [lb]),        # an action of n_prbs + 1
        ([0], [st], [np.where(np.eye(4, 2) > 0, -1, 3)], [lb]),       # a negative action
        (np.array([0, 1]), np.zeros((2, 4, 13)), np.full((2, 4, 2), 3), np.full((2, 4, 2), 2)),   # the [n, T, ...] form
    ]
    for args in bad:
        with pytest.raises(ValueError):
            h.fit_steps(*args)
    # an action off the grid is nobody's business where the label is 0: the checks pass, and the library is reached (there is none)
    with pytest.raises(AttributeError):
        h.fit_steps([0], [st], [np.where(np.eye(4, 2) > 0, 7, 3)], [np.where(np.eye(4, 2) > 0, 0, 1)])


def test_shared_dictionaries_refuse():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    assert SharedVecKBRL.fit_steps is not VecKBRL.fit_steps
    h = _no_handle('SharedVecKBRL')
    with pytest.raises(_lib.RanSliceError) as e:
        h.fit_steps([0], [np.zeros((1, 13))], [np.zeros((1, 2))], [np.ones((1, 2))])
    assert e.value.code == _lib.RS_ESTATE


def test_augmented_samples_points_to_fit_steps():
    from ranslice.kbrl_dev import augmented_samples
    assert 'fit_steps' in augmented_samples.__doc__
