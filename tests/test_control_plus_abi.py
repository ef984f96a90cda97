"""The closed control loop's Projectron++ switch at the C ABI and on the Python classes (no GPU needed): kb_set_control_plus /
kb_get_control_plus are declared, exported by both builds and bound; VecKBRL.set_control_plus, the control_plus property and the
constructor's default exist; a ProjectronPlus carries the plain attribute control_plus; KBRL_Control accepts a list of
ProjectronPlus learners that all opted in and refuses every other list that holds one with the message it always gave."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_control_plus', 'kb_get_control_plus')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_control_plus(kb_handle* k, int32_t on);' in text
    assert 'int kb_get_control_plus(kb_handle* k, int32_t* on);' in text
    flat = re.sub(r'\s+', ' ', raw)
    assert re.search(r'kb_set_control_plus\(k, on\).{0,200}on = 0 \(the default\)', flat)
    # declared beside kb_set_fit_wide_plus' family, after kb_fit_steps
    assert text.index('int kb_fit_steps(') < text.index('int kb_set_control_plus(')


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
    assert [t.__name__ for t in L.kb_set_control_plus.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.kb_get_control_plus.argtypes] == ['c_void_p', 'LP_c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_control_plus(None, 1) == _lib.RS_EINVAL
    assert L.kb_get_control_plus(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import Projectron, ProjectronPlus, SVvariable
    assert list(inspect.signature(VecKBRL.set_control_plus).parameters) == ['self', 'on']
    assert inspect.signature(VecKBRL.set_control_plus).parameters['on'].default is True
    assert isinstance(VecKBRL.control_plus, property)
    assert inspect.signature(VecKBRL.__init__).parameters['control_plus'].default is False
    assert inspect.signature(VecKBRL.__init__).parameters['algorithm'].default == 'projectron'
    # the attribute: on the class and on every object, off by default; a Projectron has none
    assert ProjectronPlus.control_plus is False
    p = ProjectronPlus(GaussianKernel(SVvariable(), 1.0))
    assert p.control_plus is False and p.wide_plus is False
    assert not hasattr(Projectron(GaussianKernel(SVvariable(), 1.0)), 'control_plus')
    # the shared-dictionary class refuses by itself, as the library does: no handle is needed to learn that
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_control_plus(object.__new__(SharedVecKBRL), True)
    assert e.value.code == _lib.RS_ESTATE


def _learners(kinds, opted):
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import Projectron, ProjectronPlus, SVvariable
    from kbrl_control import Learner
    out, at = [], 0
    for kind, on in zip(kinds, opted):
        alg = (ProjectronPlus if kind == '+' else Projectron)(GaussianKernel(SVvariable(), 1.0))
        if kind == '+':
            alg.control_plus = on
        out.append(Learner(alg, slice(at, at + 3), 100, 3))
        at += 3
    return out


def test_kbrl_control_accepts_a_list_that_opted_in(monkeypatch):
    """every learner a ProjectronPlus with control_plus true: the constructor gets past its check and asks for ONE handle in
    Projectron++ mode with the switch on.  No device is needed to see that: the handle class is replaced by a recorder, so
    nothing is created and no learner is bound to a device learner"""
    import kbrl_control
    asked = []

    class Recorder:
        algorithm = 'projectron_plus'

        def __init__(self, *a, **kw):
            asked.append((a, kw))

        def reset(self, *a, **kw):
            pass

    monkeypatch.setattr(kbrl_control, 'VecKBRL', Recorder)
    learners = _learners('++', [True, True])
    ctl = kbrl_control.KBRL_Control(learners, 200)
    assert len(asked) == 1 and asked[0][1]['algorithm'] == 'projectron_plus' and asked[0][1]['control_plus'] is True
    assert asked[0][0][:3] == (1, [3, 3], 200)
    assert all(h.algorithm._agent is ctl._dev for h in learners)
    # a list of Projectron learners asks for what it always asked for
    asked.clear()
    kbrl_control.KBRL_Control(_learners('..', [None, None]), 200)
    assert 'algorithm' not in asked[0][1] and 'control_plus' not in asked[0][1]


@pytest.mark.parametrize('kinds,opted,named', [('.+', [None, True], '[1]'), ('+.', [True, None], '[0]'), ('++', [True, False], '[0, 1]'),
                                               ('++', [False, False], '[0, 1]'), ('++', [1, True], '[0, 1]')])
def test_kbrl_control_refuses_every_other_list(kinds, opted, named):
    """a Projectron among them, or a ProjectronPlus that did not opt in (control_plus must be True itself): the parent's ValueError,
    word for word, before any device handle exists"""
    from kbrl_control import KBRL_Control
    learners = _learners(kinds, opted)
    with pytest.raises(ValueError) as e:
        KBRL_Control(learners, 200)
    assert str(e.value) == ('KBRL_Control: learner(s) %s are ProjectronPlus; the closed control loop (update_control, run) '
                            'implements the Projectron rule only.  Supported route: log the control steps, turn them into sample '
                            "lists with ranslice.kbrl_dev.augmented_samples, and VecKBRL.fit them on a handle created with "
                            "algorithm='projectron_plus' (then deploy / select_action / export_agents as usual)" % named)
    assert all(not h.algorithm._bound() for h in learners)
