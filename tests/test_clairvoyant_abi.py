"""The replica fork and the clairvoyant step at the C ABI and in the experiment script (no GPU needed): the symbols are
declared, exported and bound; the experiment seeds its runs as the KBRL evaluators do and records the reference's keys."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('rs_fork', 'rs_set_lookahead', 'rs_step_clairvoyant', 'rs_set_clairvoyant_fallback')


def _header():
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_declared_in_the_header():
    text = _header()
    assert re.search(r'int rs_fork\(rs_handle\* dst, rs_handle\* src, const int32_t\* src_index\);', text)
    assert re.search(r'int rs_set_lookahead\(rs_handle\* h, int max_branches\);', text)
    assert re.search(r'int rs_set_clairvoyant_fallback\(rs_handle\* h, int mode\);', text)
    assert re.search(r'int rs_step_clairvoyant\(rs_handle\* h, int32_t\* actions_out, float\* obs, double\* reward, '
                     r'int32_t\* labels,\s+int32_t\* violations\);', text)


def test_exported_and_bound():
    from ranslice import _lib
    for n in NEW:
        assert n in _lib.EXPORTS
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('libranslice.so not built (python __graft_entry__.py build)')
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert hasattr(raw, n), n
    L = _lib.load()
    assert [t.__name__ for t in L.rs_fork.argtypes] == ['c_void_p', 'c_void_p', 'LP_c_int']
    assert [t.__name__ for t in L.rs_set_lookahead.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.rs_set_clairvoyant_fallback.argtypes] == ['c_void_p', 'c_int']
    assert [t.__name__ for t in L.rs_step_clairvoyant.argtypes] == ['c_void_p', 'LP_c_int', 'LP_c_float', 'LP_c_double',
                                                                    'LP_c_int', 'LP_c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int


def test_vec_env_surface():
    from ranslice.vec_env import VecRanSlice
    for m in ('fork_from', 'set_lookahead', 'step_clairvoyant', 'set_clairvoyant_fallback'):
        assert callable(getattr(VecRanSlice, m))


def test_runs_are_seeded_as_the_kbrl_evaluators_seed_them():
    from numpy.random import default_rng
    import experiments_clairvoyant as ec
    seeds = ec.run_seeds(range(5))
    assert seeds.dtype == np.uint64
    for i in range(5):
        assert int(seeds[i]) == int(default_rng(seed=i).integers(0, 2 ** 63 - 1))


def test_step_record_has_the_reference_keys(tmp_path):
    import experiments_clairvoyant as ec
    rec = ec.StepRecord(2, 3)
    rec.add(0, np.array([[7, 3], [20, 1]]), np.array([[1, 1], [1, -1]]), np.array([[0, 0], [0, 2]]))
    rec.add(1, np.array([[0, 0], [70, 0]]), np.array([[-1, -1], [1, 1]]), np.array([[1, 1], [0, 0]]))
    path = str(tmp_path / 'results_1.npz')
    np.savez(path, **rec.results(1))
    z = np.load(path)
    assert sorted(z.files) == ['SLA', 'resources', 'violation']
    assert all(z[k].dtype == np.int64 and z[k].shape == (3,) for k in z.files)
    assert list(z['SLA']) == [0, 2, 0] and list(z['violation']) == [2, 0, 0] and list(z['resources']) == [21, 70, 0]
    assert ec.name == 'ORACLE'
