"""kb_set_control_plus_wide / kb_get_control_plus_wide / kb_control_plus_wide_info at the C ABI and on the Python classes (no GPU
needed): declared, exported by both builds and bound; a NULL handle is an argument error; VecKBRL carries the defaults
(min_landmarks 0, max_landmarks 2048, 32 rounds); the scripts and the tools take the switch."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_control_plus_wide', 'kb_get_control_plus_wide', 'kb_control_plus_wide_info')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    decls = ('int kb_set_control_plus_wide(kb_handle* k, int32_t min_landmarks, int32_t max_landmarks, int32_t rounds);',
             'int kb_get_control_plus_wide(kb_handle* k, int32_t* min_landmarks, int32_t* max_landmarks, int32_t* rounds, uint64_t* scratch_bytes);',
             'int kb_control_plus_wide_info(kb_handle* k, uint64_t work[8]);')
    at = [text.index(d) for d in decls]
    assert text.index('int kb_control_plus_batch_info(') < at[0] < at[1] < at[2] < text.index('int kb_set_fit_steps_batch(')
    # the scratch formula stands in the header comment, and the kernel file's constants are the ones it names
    flat = re.sub(r'\s+', ' ', re.sub(r'\n \*(?!/)', ' ', raw))      # (the comment's lines joined, without their leading stars)
    assert 'slots = min(T, 1024)' in flat and 'T = n_envs * n_slices' in flat
    assert 'scratch_bytes = 128 + slots * 256 + 2 * (slots + 1) * 8 + 8 * ceil(T / 2) + slots * 2 * 8 * max_landmarks * 8' in flat
    src = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'kb_control_plus_wide.hip')).read()
    for name, value in (('KB_CPW_SLOTS', 1024), ('KB_CPW_HEAD', 128), ('KB_CPW_REC', 256)):
        assert re.search(r'#define %s %d\b' % (name, value), src), name
    batch = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'kb_control_plus_batch.hip')).read()
    assert re.search(r'#define KB_CPB_W 8\b', batch)       # the arenas are always eight wide
    assert 'KB_CPW_HEAD + slots * KB_CPW_REC + 2 * (slots + 1) * 8 + 8 * ((T + 1) / 2)' in re.sub(r'\s+', ' ', src)
    assert 'slots * 2 * KB_CPB_W * (uint64_t)max_landmarks * sizeof(double)' in re.sub(r'\s+', ' ', src)
    api = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'rs_api.hip')).read()
    assert api.index('#include "kb_control_plus_batch.hip"') < api.index('#include "kb_control_plus_wide.hip"')


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
    assert [t.__name__ for t in L.kb_set_control_plus_wide.argtypes] == ['c_void_p', 'c_int', 'c_int', 'c_int']
    assert [t.__name__ for t in L.kb_get_control_plus_wide.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_int', 'LP_c_int', 'LP_c_ulong']
    assert [t.__name__ for t in L.kb_control_plus_wide_info.argtypes] == ['c_void_p', 'LP_c_ulong']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_control_plus_wide(None, 256, 2048, 32) == _lib.RS_EINVAL
    assert L.kb_get_control_plus_wide(None, None, None, None, None) == _lib.RS_EINVAL
    assert L.kb_control_plus_wide_info(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    sig = inspect.signature(VecKBRL.__init__).parameters
    assert sig['control_plus_wide'].default == 0 and sig['control_plus_wide_max'].default == 2048
    assert sig['control_plus_wide_rounds'].default == 32
    sig = inspect.signature(VecKBRL.set_control_plus_wide).parameters
    assert list(sig) == ['self', 'min_landmarks', 'max_landmarks', 'rounds']
    assert sig['min_landmarks'].default is inspect.Parameter.empty and sig['max_landmarks'].default == 2048 and sig['rounds'].default == 32
    assert isinstance(VecKBRL.control_plus_wide, property) and callable(VecKBRL.control_plus_wide_work)
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_control_plus_wide(object.__new__(SharedVecKBRL), 256)
    assert e.value.code == _lib.RS_ESTATE


def test_the_tools_take_the_switch():
    import experiments_kbrl
    import experiments_trained
    assert inspect.signature(experiments_kbrl.BatchedEvaluator.__init__).parameters['control_plus_wide'].default == 0
    assert inspect.signature(experiments_kbrl.evaluate_grid).parameters['control_plus_wide'].default == 0
    assert inspect.signature(experiments_trained.train_and_deploy).parameters['control_plus_wide'].default == 0
    assert inspect.signature(experiments_trained._evaluate_loaded).parameters['control_plus_wide'].default == 0
    with pytest.raises(ValueError):       # it needs a batch width
        experiments_kbrl.BatchedEvaluator(0, (0.99, 0.999), algorithm='projectron_plus', control_plus_wide=256)
    for path in (os.path.join(ROOT, 'network-slicing_amd', 'experiments_kbrl.py'), os.path.join(ROOT, 'network-slicing_amd', 'experiments_trained.py')):
        text = open(path).read()
        assert "'--control-plus-wide'" in text and '--control-plus-wide needs --control-plus-batch' in text, path
    assert "'--wide'" in open(os.path.join(ROOT, 'tools', 'control_plus_record.py')).read()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    # a dict of its own; the batch kernels' is what it was
    assert cr.CTL_BATCH == {'control_plus_batch_kernelILi2E': (209, 19968, 0), 'control_plus_batch_kernelILi4E': (249, 28240, 0),
                            'control_plus_batch_kernelILi8E': (256, 44784, 196)}
    assert all(k.startswith('cpw_') for k in cr.CTL_WIDE) and not set(cr.CTL_WIDE) & set(cr.CTL_BATCH)
    for k in ('cpw_rank1_kernel',) + tuple('cpw_pass_kernelILi%dE' % w for w in (2, 4, 8)):
        assert cr.CTL_WIDE[k] == 0, k                       # the two kernels that stream Kinv hold no scratch
    for w in (2, 4, 8):
        for stem in ('cpw_walk_kernel', 'cpw_finish_kernel', 'cpw_rows_kernel'):
            assert cr.CTL_WIDE['%sILi%dE' % (stem, w)] < cr.LIMIT, (stem, w)
    # no new name shadows an entry that is matched by substring
    older = list(cr.KB_SCRATCH) + list(cr.PRUNE) + list(cr.REF_SCRATCH) + list(cr.REBUILD_SCRATCH) + list(cr.FIT_SCRATCH)
    assert not [(o, n) for o in older for n in cr.CTL_WIDE if o in n]
