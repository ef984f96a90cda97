"""The online budget of shared-dictionary handles (kb_set_shared_online_prune) at the C ABI, on SharedVecKBRL
and in the tools (no GPU needed): declared, exported, bound; every default is off; the per-replica keyword is still refused."""
import ctypes as C
import inspect
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_set_shared_online_prune', 'kb_get_shared_online_prune', 'kb_shared_online_prune_info', 'kb_shared_online_prune_stage')


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    assert re.search(r'int kb_set_shared_online_prune\(kb_handle\* k, int32_t target, int32_t rounds\);', text)
    assert re.search(r'int kb_get_shared_online_prune\(kb_handle\* k, int32_t\* target, int32_t\* rounds\);', text)
    assert re.search(r'int kb_shared_online_prune_info\(kb_handle\* k, uint64_t work\[8\]\);', text)
    assert re.search(r'int kb_shared_online_prune_stage\(kb_handle\* k\);', text)


def test_the_new_file_is_included_behind_the_two_it_builds_on():
    text = open(os.path.join(ROOT, 'network-slicing_amd', 'csrc', 'rs_api.hip')).read()
    at = [text.index('#include "%s"' % n) for n in ('kb_shared_prune.hip', 'kb_online_prune.hip', 'kb_shared_online_prune.hip')]
    assert at[2] > at[0] and at[2] > at[1]


def test_listed_among_the_exports():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS


def test_exported_and_bound():
    """the built library (build() of __graft_entry__.py makes it: a missing library is a failure, not a skip)"""
    from ranslice import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.kb_set_shared_online_prune.argtypes] == ['c_void_p', 'c_int', 'c_int']
    assert [t.__name__ for t in L.kb_get_shared_online_prune.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_int']
    assert [t.__name__ for t in L.kb_shared_online_prune_info.argtypes] == ['c_void_p', 'LP_c_ulong']
    assert [t.__name__ for t in L.kb_shared_online_prune_stage.argtypes] == ['c_void_p']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int


def test_python_surface_and_defaults():
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    for m in ('set_shared_online_prune', 'shared_online_prune_info'):
        assert callable(getattr(SharedVecKBRL, m)) and not hasattr(VecKBRL, m)
    assert isinstance(inspect.getattr_static(SharedVecKBRL, 'shared_online_prune'), property)
    p = inspect.signature(SharedVecKBRL.set_shared_online_prune).parameters
    assert list(p) == ['self', 'target', 'rounds'] and p['rounds'].default == 2
    p = inspect.signature(SharedVecKBRL.__init__).parameters
    assert p['shared_online_prune'].default is None and p['shared_online_prune_rounds'].default == 2
    # what was off by default still is
    assert p['shared_plus'].default is False and p['shared_plus_batch'].default is None and p['exchange'].default is None
    # the per-replica keyword is refused before the library is touched, as before; the message now names the shared switch too
    with pytest.raises(ValueError, match='online_prune') as ei:
        SharedVecKBRL(2, [10], 200, online_prune=64)
    assert 'shared_online_prune' in str(ei.value)


def test_the_new_kernel_is_in_the_resource_report():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import check_resources as cr
    assert list(cr.SHARED_ONLINE_PRUNE) == ['shared_budget_round_kernel']
    assert list(cr.ONLINE_PRUNE) == ['budget_list_kernel', 'budget_round_kernel']
    res = cr.parse()
    for key in cr.SHARED_ONLINE_PRUNE + cr.ONLINE_PRUNE:
        hit = [k for k in res if re.search(r'\d' + key, k)]
        assert len(hit) == 1, (key, hit)
        assert res[hit[0]].get('ScratchSize', 0) == 0, (key, res[hit[0]])


def test_the_record_tool_names_the_switch():
    """--online-prune / --online-prune-rounds in tools/shared_prune_record.py, and the mode excludes the periodic shrink"""
    text = open(os.path.join(ROOT, 'tools', 'shared_prune_record.py')).read()
    assert "'--online-prune'" in text and "'--online-prune-rounds'" in text
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import shared_prune_record as rec
    with pytest.raises(SystemExit, match='online-prune'):
        rec.main(['--child', 'shrink', '--online-prune', '768'])
