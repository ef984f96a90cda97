"""kb_set_control_plus_batch / kb_get_control_plus_batch / kb_control_plus_batch_info at the C ABI and on the Python classes (no GPU
needed): declared, exported by both builds and bound; a NULL handle is an argument error; VecKBRL carries the defaults (width
0, max_landmarks 1024); the tools take the width."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_control_plus_batch', 'kb_get_control_plus_batch', 'kb_control_plus_batch_info')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_control_plus_batch(kb_handle* k, int32_t width, int32_t max_landmarks);' in text
    assert 'int kb_get_control_plus_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes);' in text
    assert 'int kb_control_plus_batch_info(kb_handle* k, uint64_t work[8]);' in text
    assert text.index('int kb_get_control_plus(') < text.index('int kb_set_control_plus_batch(')
    # the scratch formula stands in the header comment, and the kernel file's constants are the ones it names
    flat = re.sub(r'\s+', ' ', raw)
    assert 'scratch_bytes = 128 + min(n_envs * n_slices, 1024) * 2 * width * max_landmarks * 8' in flat
    src = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'kb_control_plus_batch.hip')).read()
    assert re.search(r'#define KB_CPB_ARENAS 1024\b', src) and re.search(r'#define KB_CPB_HEAD 128\b', src)


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
    assert [t.__name__ for t in L.kb_set_control_plus_batch.argtypes] == ['c_void_p', 'c_int', 'c_int']
    assert [t.__name__ for t in L.kb_get_control_plus_batch.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_int', 'LP_c_ulong']
    assert [t.__name__ for t in L.kb_control_plus_batch_info.argtypes] == ['c_void_p', 'LP_c_ulong']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_control_plus_batch(None, 8, 1024) == _lib.RS_EINVAL
    assert L.kb_get_control_plus_batch(None, None, None, None) == _lib.RS_EINVAL
    assert L.kb_control_plus_batch_info(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    sig = inspect.signature(VecKBRL.__init__).parameters
    assert sig['control_plus_batch'].default == 0 and sig['control_plus_batch_max'].default == 1024
    assert sig['control_plus'].default is False
    sig = inspect.signature(VecKBRL.set_control_plus_batch).parameters
    assert list(sig) == ['self', 'width', 'max_landmarks'] and sig['max_landmarks'].default == 1024
    assert sig['width'].default is inspect.Parameter.empty
    assert isinstance(VecKBRL.control_plus_batch, property)
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_control_plus_batch(object.__new__(SharedVecKBRL), 8)
    assert e.value.code == _lib.RS_ESTATE


def test_the_tools_take_the_width():
    import experiments_kbrl
    assert inspect.signature(experiments_kbrl.BatchedEvaluator.__init__).parameters['control_plus_batch'].default == 0
    for path in (os.path.join(ROOT, 'network-slicing_amd', 'experiments_kbrl.py'), os.path.join(ROOT, 'network-slicing_amd', 'experiments_trained.py')):
        assert "'--control-plus-batch'" in open(path).read(), path
    assert "'--batch'" in open(os.path.join(ROOT, 'tools', 'control_plus_record.py')).read()
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    assert sorted(cr.CTL_BATCH) == ['control_plus_batch_kernelILi%dE' % w for w in (2, 4, 8)]
    assert cr.CTL_BATCH['control_plus_batch_kernelILi2E'][2] == 0 and cr.CTL_BATCH['control_plus_batch_kernelILi4E'][2] == 0
