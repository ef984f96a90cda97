"""kb_set_fit_steps_batch / kb_get_fit_steps_batch / kb_fit_steps_batch_info at the C ABI and on the Python classes (no GPU needed):
declared, exported by both builds and bound; a NULL handle is an argument error; VecKBRL carries the defaults (width 0,
max_landmarks 1024) and SharedVecKBRL refuses; the example takes the width; the three instances of the kernel stand in
tools/check_resources.py beside the control loop's, whose entries are what they were."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_fit_steps_batch', 'kb_get_fit_steps_batch', 'kb_fit_steps_batch_info')


def test_declared_in_the_header():
    raw = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    text = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', raw, flags=re.S))
    assert 'int kb_set_fit_steps_batch(kb_handle* k, int32_t width, int32_t max_landmarks);' in text
    assert 'int kb_get_fit_steps_batch(kb_handle* k, int32_t* width, int32_t* max_landmarks, uint64_t* scratch_bytes);' in text
    assert 'int kb_fit_steps_batch_info(kb_handle* k, uint64_t work[8]);' in text
    assert text.index('int kb_control_plus_batch_info(') < text.index('int kb_set_fit_steps_batch(')
    # kb_fit_steps's own comment no longer promises one workgroup per learner whatever the settings
    flat = re.sub(r'\s+', ' ', raw.replace('\n *', ' '))
    assert 'one workgroup per learner always' not in flat
    assert flat.count('scratch_bytes = 128 + min(n_envs * n_slices, 1024) * 2 * width * max_landmarks * 8') == 2
    # the kernel file: after the control loop's in the one translation unit; the walk is called, not restated
    api = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'rs_api.hip')).read()
    assert api.index('#include "kb_control_plus_batch.hip"') < api.index('#include "kb_fit_steps_batch.hip"')
    src = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'kb_fit_steps_batch.hip')).read()
    code = re.sub(r'//[^\n]*', '', src)
    assert 'plus_group_walk<W>(' in code and '__launch_bounds__(256, 2)' in code
    assert 'hv_work' not in code and 'fver' not in code and 'finish_update' not in code and 'asm' not in code


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
    assert [t.__name__ for t in L.kb_set_fit_steps_batch.argtypes] == ['c_void_p', 'c_int', 'c_int']
    assert [t.__name__ for t in L.kb_get_fit_steps_batch.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_int', 'LP_c_ulong']
    assert [t.__name__ for t in L.kb_fit_steps_batch_info.argtypes] == ['c_void_p', 'LP_c_ulong']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int
    # no handle: an argument error, nothing is dereferenced
    assert L.kb_set_fit_steps_batch(None, 8, 1024) == _lib.RS_EINVAL
    assert L.kb_get_fit_steps_batch(None, None, None, None) == _lib.RS_EINVAL
    assert L.kb_fit_steps_batch_info(None, None) == _lib.RS_EINVAL


def test_python_surface():
    from ranslice import _lib
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    sig = inspect.signature(VecKBRL.__init__).parameters
    assert sig['fit_steps_batch'].default == 0 and sig['fit_steps_batch_max'].default == 1024
    assert sig['control_plus_batch'].default == 0 and sig['control_plus_batch_max'].default == 1024
    sig = inspect.signature(VecKBRL.set_fit_steps_batch).parameters
    assert list(sig) == ['self', 'width', 'max_landmarks'] and sig['max_landmarks'].default == 1024
    assert sig['width'].default is inspect.Parameter.empty
    assert isinstance(VecKBRL.fit_steps_batch, property) and callable(VecKBRL.fit_steps_batch_work)
    with pytest.raises(_lib.RanSliceError) as e:
        SharedVecKBRL.set_fit_steps_batch(object.__new__(SharedVecKBRL), 8)
    assert e.value.code == _lib.RS_ESTATE


def test_the_tools_take_the_width():
    assert "'--batch'" in open(os.path.join(ROOT, 'examples', 'teach_from_log.py')).read()
    assert 'fit_steps_batch_record.json' in open(os.path.join(ROOT, 'tools', 'fit_steps_record.py')).read()
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    assert sorted(cr.FIT_STEPS_BATCH) == ['fit_steps_batch_kernelILi%dE' % w for w in (2, 4, 8)]
    # widths 2 and 4 are held to no scratch at all, width 8 below the bound the project holds its spilling kernels to
    assert cr.FIT_STEPS_BATCH['fit_steps_batch_kernelILi2E'][2] == 0 and cr.FIT_STEPS_BATCH['fit_steps_batch_kernelILi4E'][2] == 0
    assert cr.FIT_STEPS_BATCH['fit_steps_batch_kernelILi8E'][2] <= cr.LIMIT
    # registers and LDS (Lds + pre + BatchLds<W>) are the control loop's instances': two workgroups per CU fit
    for w in (2, 4, 8):
        assert cr.FIT_STEPS_BATCH['fit_steps_batch_kernelILi%dE' % w][:2] == cr.CTL_BATCH['control_plus_batch_kernelILi%dE' % w][:2]
        assert 2 * cr.FIT_STEPS_BATCH['fit_steps_batch_kernelILi%dE' % w][1] <= 160 << 10
    # the control loop's entries are what they were
    assert cr.CTL_BATCH == {'control_plus_batch_kernelILi2E': (209, 19968, 0), 'control_plus_batch_kernelILi4E': (249, 28240, 0),
                            'control_plus_batch_kernelILi8E': (256, 44784, 196)}


def test_the_build_holds_the_instances_to_their_entries():
    """the resource log of the build that made the library (build() writes it): every instance is there, within its entry, and
    built for two waves per SIMD"""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    res = cr.parse()
    for key, (regs, lds, scratch) in cr.FIT_STEPS_BATCH.items():
        hit = [k for k in res if re.search(r'\d' + key, k)]
        assert len(hit) == 1, key
        r = res[hit[0]]
        print(key, r)
        assert r['VGPRs'] + r.get('AGPRs', 0) <= regs and r['LDS Size'] <= lds and r['ScratchSize'] <= scratch, (key, r)
        assert r['Occupancy'] >= 2, (key, r)
