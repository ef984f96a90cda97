"""Deployment by reference (kb_deploy_ref) at the C ABI and on VecKBRL, without a GPU: the symbol is declared, exported and
bound; the argument checks that need no device answer RS_EINVAL; the pool of a by-reference handle is deploy_pool_bytes of the
distinct agents."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_in_the_header():
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'ranslice.h')).read(), flags=re.S)
    assert re.search(r'int kb_deploy_ref\(kb_handle\* src, const int32_t\* src_index, int32_t n, kb_handle\*\* out\);', text)


def test_exported_and_bound():
    from ranslice import _lib
    assert 'kb_deploy_ref' in _lib.EXPORTS
    for path in (_lib.LIB_PATH, _lib.DEV_LIB_PATH):
        assert os.path.exists(path), path + ': build first (python __graft_entry__.py build)'
        assert hasattr(C.CDLL(path), 'kb_deploy_ref'), path
    L = _lib.load()
    assert [t.__name__ for t in L.kb_deploy_ref.argtypes] == ['c_void_p', 'LP_c_int', 'c_int', 'LP_c_void_p']
    assert L.kb_deploy_ref.restype is C.c_int


def test_argument_checks_need_no_device():
    """NULL source, n <= 0 and out == NULL are answered before anything is looked at: the `handle` here is 4 KB of zeros"""
    from ranslice import _lib
    L = _lib.load()
    idx = np.zeros(4, dtype=np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
    out = C.c_void_p(0x5A5A)
    fake = C.create_string_buffer(4096)
    src = C.cast(fake, C.c_void_p)
    assert L.kb_deploy_ref(None, ip, 4, C.byref(out)) == _lib.RS_EINVAL
    assert L.kb_deploy_ref(src, None, 4, C.byref(out)) == _lib.RS_EINVAL
    assert L.kb_deploy_ref(src, ip, 0, C.byref(out)) == _lib.RS_EINVAL
    assert L.kb_deploy_ref(src, ip, -3, C.byref(out)) == _lib.RS_EINVAL
    assert L.kb_deploy_ref(src, ip, 4, None) == _lib.RS_EINVAL
    assert out.value == 0x5A5A and fake.raw == bytes(4096)


def test_vec_kbrl_surface():
    import inspect
    from ranslice.kbrl_dev import VecKBRL
    p = inspect.signature(VecKBRL.deploy).parameters
    assert list(p) == ['self', 'index', 'by_reference'] and p['by_reference'].default is False
    assert VecKBRL.by_reference is False and VecKBRL.frozen is False


def test_pool_of_the_distinct_agents():
    """512 + 15,360 x sum of ceil(m / 64) over the distinct (agent, slice) dictionaries: deploy_pool_bytes of the de-duplicated
    index, whatever the order and the number of the references"""
    from ranslice import kbrl_dev as kd
    sizes = np.array([[0, 1], [64, 65], [300, 2], [513, 128], [7, 7]], dtype=np.int32)   # shells: 1, 3, 6, 11, 2
    shells = [1, 3, 6, 11, 2]
    cases = [([0], [0]), ([3, 3, 3, 3], [3]), ([4, 1, 4, 1, 1, 4], [1, 4]), ([2, 0, 3, 1, 4, 0, 2], [0, 1, 2, 3, 4]),
             (list(np.random.default_rng(1).integers(1, 4, 1000)), [1, 2, 3])]
    for index, distinct in cases:
        want = 512 + 15360 * sum(shells[a] for a in distinct)
        assert kd.deploy_ref_pool_bytes(sizes, index) == want == kd.deploy_pool_bytes(sizes[distinct]), index
        assert kd.deploy_ref_pool_bytes(sizes, index) <= kd.deploy_pool_bytes(sizes[np.asarray(index)])
    # 30 agents on 65,536 replicas: the pool is the 30 agents', 2,184 times smaller than the copies' (less the preamble)
    big = np.full((30, 5), 500, dtype=np.int32)
    index = np.arange(65536) % 30
    assert kd.deploy_ref_pool_bytes(big, index) == 512 + 15360 * 30 * 5 * 8
    assert kd.deploy_pool_bytes(big[index]) == 512 + 15360 * 65536 * 5 * 8
