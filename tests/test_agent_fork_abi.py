"""The agent fork, the deployment and the learning switch at the C ABI, on VecKBRL and in the experiment script (no GPU
needed): the symbols are declared, exported and bound; the compact pool's size follows its stated rule; the experiment's
aggregation is the reference's mean_confidence_radius."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('kb_fork', 'kb_deploy', 'kb_set_learning')


def _header():
    text = open(os.path.join(ROOT, 'include', 'ranslice.h')).read()
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def test_declared_in_the_header():
    text = _header()
    assert re.search(r'int kb_fork\(kb_handle\* dst, kb_handle\* src, const int32_t\* src_index\);', text)
    assert re.search(r'int kb_deploy\(kb_handle\* src, const int32_t\* src_index, int32_t n, kb_handle\*\* out\);', text)
    assert re.search(r'int kb_set_learning\(kb_handle\* k, int on\);', text)


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
    assert [t.__name__ for t in L.kb_fork.argtypes] == ['c_void_p', 'c_void_p', 'LP_c_int']
    assert [t.__name__ for t in L.kb_deploy.argtypes] == ['c_void_p', 'LP_c_int', 'c_int', 'LP_c_void_p']
    assert [t.__name__ for t in L.kb_set_learning.argtypes] == ['c_void_p', 'c_int']
    for n in NEW:
        assert getattr(L, n).restype is C.c_int


def test_vec_kbrl_surface():
    from ranslice.kbrl_dev import VecKBRL
    for m in ('fork_from', 'deploy', 'set_learning'):
        assert callable(getattr(VecKBRL, m))
    assert VecKBRL.frozen is False


def test_deploy_pool_bytes_follows_its_rule():
    """fixed preamble + 15,360 bytes per started 64 landmarks.  The pool keeps offset 0 as "not allocated": its first 64
    doubles are never handed out, so the preamble is 512 bytes."""
    from ranslice import kbrl_dev
    sizes = [[0, 1, 64, 65, 300]]       # 0 + 1 + 1 + 2 + 5 = 9 shells
    preamble = kbrl_dev.deploy_pool_bytes(np.zeros((1, 5), dtype=np.int32))
    assert preamble == kbrl_dev.POOL_PREAMBLE_BYTES == 64 * 8
    assert kbrl_dev.deploy_pool_bytes(sizes) - preamble == 138240 == 9 * 15360
    assert kbrl_dev.VEC_PAGE_BYTES == 30 * 64 * 8 == 15360
    assert kbrl_dev.deploy_pool_bytes(np.array(sizes, dtype=np.int32)) == kbrl_dev.deploy_pool_bytes(sizes)
    assert kbrl_dev.deploy_pool_bytes([[64] * 5] * 3) - preamble == 15 * 15360


def test_aggregation_is_the_reference_interval():
    """window_statistics on a hand-made array: per-agent means over the window, then the mean and the 95 % t-interval over
    the agents, computed here with scipy.stats"""
    from scipy import stats
    import experiments_trained as et
    rng = np.random.default_rng(4)
    n_prbs = 200
    viol = rng.integers(0, 3, size=(6, 50)).astype(np.int16)
    res = rng.integers(60, 190, size=(6, 50)).astype(np.int16)

    def interval(per_agent):
        a = np.array(per_agent, dtype=np.float64)
        return a.mean(), stats.sem(a) * stats.t.ppf((1 + 0.95) / 2., len(a) - 1)
    got = et.window_statistics(viol, res, n_prbs, start=10, end=40)
    want_v = interval([viol[k, 10:40].mean() for k in range(6)])
    want_r = interval([res[k, 10:40].mean() / n_prbs for k in range(6)])
    assert got['violations'] == pytest.approx(want_v, rel=1e-12)
    assert got['occupation'] == pytest.approx(want_r, rel=1e-12)
    m, h = et.mean_confidence_radius([1.0, 2.0, 4.0, 7.0])
    assert (m, h) == pytest.approx(interval([1.0, 2.0, 4.0, 7.0]), rel=1e-12)
    # several replicas per agent: each agent's figure is the mean over its replicas and the window; the interval is over agents
    viol3 = rng.integers(0, 4, size=(5, 7, 20))
    res3 = rng.integers(50, 200, size=(5, 7, 20))
    got = et.window_statistics(viol3, res3, n_prbs)
    assert got['violations'] == pytest.approx(interval([viol3[k].mean() for k in range(5)]), rel=1e-12)
    assert got['occupation'] == pytest.approx(interval([res3[k].mean() / n_prbs for k in range(5)]), rel=1e-12)


def test_evaluation_seeds_are_apart_from_the_training_runs():
    import experiments_trained as et
    s = et.eval_seeds(4)
    assert s.dtype == np.uint64 and len(set(int(v) for v in s)) == 4
    train = {int(np.random.default_rng(seed=i).integers(0, 2 ** 63 - 1)) for i in range(64)}
    assert not train & set(int(v) for v in s)
