"""kb_fork_rebuild / kb_get_rebuild / kb_rebuild_time_ms at the C ABI and on VecKBRL (no GPU needed): the symbols are declared
with the signatures that are bound, exported by both builds of the library, and VecKBRL.load_agents refuses the one
combination of its arguments that names two different storages before it calls the library at all."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_fork_rebuild', 'kb_get_rebuild', 'kb_rebuild_time_ms')


def _header():
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_declared_in_the_header():
    text = _header()
    assert re.search(r'int kb_fork_rebuild\(kb_handle\* dst, kb_handle\* src, const int32_t\* src_index\);', text)
    assert re.search(r'int kb_get_rebuild\(kb_handle\* k, double\* min_delta\s*, uint64_t work\[4\]\);', text)
    assert re.search(r'int kb_rebuild_time_ms\(kb_handle\* k, double\* ms\);', text)


def test_exported_by_both_builds_and_bound():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS and n in _lib.KB_EXPORTS
    for path in (_lib.LIB_PATH, _lib.DEV_LIB_PATH):
        if not os.path.exists(path):
            pytest.skip('%s not built (python __graft_entry__.py build)' % os.path.basename(path))
        raw = C.CDLL(path)
        for n in NEW:
            assert hasattr(raw, n), (path, n)
    for L in (_lib.load(), _lib.load(dev=True)):
        assert [t.__name__ for t in L.kb_fork_rebuild.argtypes] == ['c_void_p', 'c_void_p', 'LP_c_int']
        assert [t.__name__ for t in L.kb_get_rebuild.argtypes] == ['c_void_p', 'LP_c_double', 'LP_c_ulong']
        assert [t.__name__ for t in L.kb_rebuild_time_ms.argtypes] == ['c_void_p', 'LP_c_double']
        for n in NEW:
            assert getattr(L, n).restype is C.c_int
    # the existing fork keeps its own entry point
    assert _lib.load().kb_fork is not _lib.load().kb_fork_rebuild


def test_vec_kbrl_surface():
    import inspect
    from ranslice.kbrl_dev import VecKBRL
    assert callable(VecKBRL.rebuild_stats)
    assert inspect.signature(VecKBRL.fork_from).parameters['rebuild'].default is False
    p = inspect.signature(VecKBRL.load_agents).parameters
    assert list(p) == ['blob', 'index', 'by_reference', 'device', 'learning', 'capacity', 'pool_bytes']
    assert p['learning'].default is False and p['capacity'].default is None and p['pool_bytes'].default is None


def test_learning_by_reference_is_refused_before_any_library_call(monkeypatch):
    from ranslice import _lib, kbrl_dev

    def no_library(*a, **k):
        raise AssertionError('the library was loaded')
    monkeypatch.setattr(_lib, 'load', no_library)
    with pytest.raises(ValueError, match='by_reference'):
        kbrl_dev.VecKBRL.load_agents(b'not even a file', learning=True, by_reference=True)


def test_with_capacity_rewrites_the_header_alone():
    """agent_file.with_capacity: the same agents under another limit -- what load_agents(learning=True, capacity=...) imports"""
    from ranslice import agent_file as af
    cfg = dict(n_prbs=20, capacity=64, dims=[3], alfa=0.05, accuracy_range=(0.99, 0.999), gamma=1.0, eta=0.1)
    rng = np.random.default_rng(1)
    ag = dict(landmarks=[rng.uniform(0, 1, (5, 4))], coeff=[rng.uniform(-1, 1, 5)], action=[3], security_factors=[2], margins=[1],
              adjusted=0, accuracies=rng.uniform(0, 1, (1, 20)))
    blob = af.pack(cfg, [ag])
    assert af.with_capacity(blob, 64) == blob
    big = af.with_capacity(blob, 1024)
    assert big == af.pack(dict(cfg, capacity=1024), [ag])
    u = af.unpack(big)      # (checks the hash)
    assert u['config']['capacity'] == 1024 and u['agents'][0]['landmarks'][0].tobytes() == ag['landmarks'][0].tobytes()
    with pytest.raises(ValueError):
        af.with_capacity(b'x' * 200, 128)
