"""kb_fork_rebuild on the device: learning handles made from sources that hold no Kinv (kb_deploy, kb_import_agents), Kinv
rebuilt by replaying the insertions in slot order.

Where the slots are in insertion order (everything but the pruned and the reference-packed dictionaries) every comparison is
BYTES: against kb_fork's twin of the same agents, against the source's own Kinv, and of every later step of a continuation.
The pruned sources are held to the tolerance and the measure tests/test_gpu_prune.py applies to Kinv; the reference-trained
agent to the tolerances of the G17 case of tests/test_gpu_kbrl.py."""
import os

import numpy as np
import pytest

import prune_mirror as pm
from oracle import pyoracle as po
from ranslice import _lib, agent_file as af
from test_gpu_agent_fork import BIG, KEYS, N, Source, _index, _learners, _record, _same_control, _same_learner
from test_gpu_deploy_ref import GAMMA, _bits, grow, new_agent, rows
from test_gpu_prune import D_MARGIN, ETA, F_MARGIN, KINV_RTOL

pytestmark = pytest.mark.gpu

DIMS = [10, 3]
N_PRBS = 200
SMALL = 192     # KB_RB_SMALL: steps below it are replayed by one workgroup per dictionary, the rest in chip-wide rounds
# agent a: SIZES[a] landmarks of dims 10, SIZES[-1 - a] of dims 3 -- the seams: chunk and shell (64), the small / large
# threshold (192) and KB_BIG_M (320), each with its neighbours
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 319, 320, 321, 513]
G14_AGENT = len(SIZES)      # one more agent, fed the whole G14 stream into its dims-10 learner


def _g14(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g14_projectron_long.npz'))
    return g['x'], g['y'].astype(int)


def _g17(golden_dir):
    g = np.load(os.path.join(golden_dir, 'g17_projectron_3000.npz'))
    return np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1), g['y'].astype(int)


def _dev_agent(n, dims=DIMS, n_prbs=N_PRBS, capacity=1024, pool_bytes=0):
    """a learning handle of the test build, not reset (a destination)"""
    from ranslice.kbrl_dev import VecKBRL
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        return VecKBRL(n, dims, n_prbs, capacity=capacity, gamma=GAMMA, pool_bytes=pool_bytes)


def _dev_load(blob, **kw):
    from ranslice.kbrl_dev import VecKBRL
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        return VecKBRL.load_agents(blob, **kw)


def _kinv_dist(A, B):
    """the measure of tests/test_gpu_prune.py: the largest difference against the scale (the largest entry) of the second"""
    return float(np.abs(A - B).max() / np.abs(B).max())


# ------------------------------------------------------------------ 1. the twin of kb_fork
@pytest.fixture(scope='module', params=[0, 2])
def trained(request, golden_dir):
    """read-only: nothing in this module's tests that take it steps or updates it"""
    s = Source(golden_dir, request.param, tail=False)
    yield s
    s.close()


def test_twin_of_kb_fork(trained):
    """dep = deploy(index); dst.fork_from(dep, idx2, rebuild=True) against twin.fork_from(src, index[idx2]): landmarks,
    coefficients and Kinv of every (agent, slice) as bytes, control state, sizes and flags; the same from the learning handle
    itself; and again into the same handle"""
    src = trained
    rng = np.random.default_rng(5)
    index = _index(rng)
    S = len(src.dims)
    dep = src.agent.deploy(index)
    idx2 = np.concatenate([rng.permutation(len(index)), [7, 7, 6]]).astype(np.int32)
    both = index[idx2]
    twin = src.new_agent(len(idx2))
    twin.fork_from(src.agent, both)
    want = _learners(twin, range(len(idx2)), S)
    assert max(w['m'] for w in want.values()) >= 320
    dst = src.new_agent(len(idx2))
    for source, idx, what in ((dep, idx2, 'deployed'), (src.agent, both, 'learning handle'), (dep, idx2, 'again')):
        dst.fork_from(source, idx, rebuild=True)
        for key, w in want.items():
            assert _same_learner(dst.learner(*key, with_kinv=True), w), (what, key)
        assert _same_control(dst.control(), twin.control(), np.arange(len(idx2))), what
        assert (dst.dictionary_sizes() == twin.dictionary_sizes()).all(), what
        assert dst.flagged_replicas() == twin.flagged_replicas(), what
        assert dst.stats() == [0, 0, 0, 0], what
        st = dst.rebuild_stats()
        sizes = twin.dictionary_sizes()
        assert st['dictionaries'] == int((sizes > 0).sum()) and st['rounds'] == max(int(sizes.max()) - SMALL, 0), what
        assert (st['min_delta'] > 0).all() and (st['min_delta'][sizes < 2] == 1.0).all(), what
    # the cache of the last kb_predict restarted: kb_update wants a new kb_predict
    j = int(np.nonzero(both == BIG[0])[0][0])
    with pytest.raises(_lib.RanSliceError) as e:
        dst.update(j, BIG[1], np.zeros(src.dims[BIG[1]] + 1), 1)
    assert e.value.code == _lib.RS_ESTATE
    for h in (dst, twin, dep):
        h.close()


# ------------------------------------------------------------------ 2. the size ladder
class Ladder:
    def __init__(self, golden_dir):
        n = len(SIZES) + 1
        self.src = new_agent(n, DIMS, N_PRBS, capacity=1024)
        self.min_delta = np.ones((n, 2))
        for a in range(len(SIZES)):
            self._grow(a, 0, SIZES[a], 500 + 2 * a)
            self._grow(a, 1, SIZES[-1 - a], 501 + 2 * a)
        xs, ys = _g14(golden_dir)
        deltas = []
        for x, y in zip(xs, ys):
            self.src.predict(G14_AGENT, 0, x)
            br, dl = self.src.update(G14_AGENT, 0, x, int(y))
            if br == 2:
                deltas.append(dl)
        self.min_delta[G14_AGENT, 0] = min(deltas[1:])
        self.sizes = self.src.dictionary_sizes()
        assert self.sizes[:len(SIZES), 0].tolist() == SIZES and self.sizes[:len(SIZES), 1].tolist() == SIZES[::-1]
        assert self.sizes[G14_AGENT].tolist() == [790, 0]

    def _grow(self, e, s, m, seed):
        """test_gpu_deploy_ref.grow, keeping the delta of every insertion behind the first"""
        deltas, update = [], self.src.update

        def recording(e_, s_, x, y):
            br, dl = update(e_, s_, x, y)
            if br == 2:
                deltas.append(dl)
            return br, dl
        self.src.update = recording
        try:
            grow(self.src, e, s, m, seed)
        finally:
            del self.src.update
        assert len(deltas) == m
        if m >= 2:
            self.min_delta[e, s] = min(deltas[1:])

    def close(self):
        self.src.close()


@pytest.fixture(scope='module')
def ladder(golden_dir):
    ld = Ladder(golden_dir)
    yield ld
    ld.close()


def test_size_ladder(ladder):
    """dictionaries of 0 .. 513 landmarks of dims 10 and 3 and the G14 learner (790 landmarks, close neighbours, a float32
    first pair), deployed and rebuilt: Kinv equals the source's as bytes, min_delta is the smallest delta kb_update returned
    while the dictionary grew, and the work words follow the plan"""
    src = ladder.src
    n = src.n_envs
    dep = src.deploy(np.arange(n, dtype=np.int32))
    dst = _dev_agent(n)
    dst.fork_from(dep, np.arange(n, dtype=np.int32), rebuild=True)
    for e in range(n):
        for s in range(2):
            a, b = dst.learner(e, s, with_kinv=True), src.learner(e, s, with_kinv=True)
            assert _same_learner(a, b), (e, s, a['m'])
    g14 = src.learner(G14_AGENT, 0, with_kinv=True)['kinv']
    assert np.abs(g14 - np.eye(790)).max() > 1.0      # (entries well away from the identity)
    st = dst.rebuild_stats()
    assert _bits(st['min_delta']) == _bits(ladder.min_delta)
    assert ETA < st['min_delta'][G14_AGENT, 0] < 0.5
    tiles = units = 0
    for m in ladder.sizes.ravel():
        for j in range(1, int(m)):
            nb, nb1 = (j + 63) // 64, (j + 64) // 64
            tiles += nb * (nb + 1) // 2 if j >= 2 else 0
            units += nb1 * (nb1 + 1) // 2 * 4
    assert (st['matvec_tiles'], st['rank1_units'], st['rounds'], st['dictionaries']) == (tiles, units, 790 - SMALL, int((ladder.sizes > 0).sum()))
    assert st['replay_ms'] == 0.0
    dst.set_kernel_timing(True)
    dst.fork_from(dep, np.arange(n, dtype=np.int32), rebuild=True)
    st2 = dst.rebuild_stats()
    print('replay of the ladder: %.3f ms' % st2['replay_ms'])
    assert st2['replay_ms'] > 0.0 and _bits(st2['min_delta']) == _bits(st['min_delta'])
    assert _same_learner(dst.learner(G14_AGENT, 0, with_kinv=True), src.learner(G14_AGENT, 0, with_kinv=True))
    dst.close()
    dep.close()


# ------------------------------------------------------------------ 3. continuation through a file
@pytest.fixture(params=[0, 2])
def src(request, golden_dir):
    s = Source(golden_dir, request.param)
    yield s
    s.close()


def _load_learning(src, blob, index):
    from ranslice.kbrl_dev import VecKBRL
    return VecKBRL.load_agents(blob, index, learning=True, pool_bytes=512 << 20)


def test_continuation_through_a_file_teacher_forced(src):
    """export, load_agents(blob, index, learning=True): twenty teacher-forced steps as test_continuation_teacher_forced runs them
    -- equal hits, actions and adjusted at every step, equal dictionaries with Kinv at the end; the identity-index handle
    exports the file's bytes again"""
    index = _index(np.random.default_rng(6))
    S = len(src.dims)
    ident = np.arange(N, dtype=np.int32)
    blob = src.agent.export_agents(ident)
    seq = _record(src, 20)
    dst = _load_learning(src, blob, index)
    assert not dst.frozen and dst.capacity == src.agent.capacity
    for i, (state, act, lab, obs) in enumerate(seq):
        hs = src.agent.update_control(state, act, lab)
        hd = dst.update_control(state[index], act[index], lab[index])
        assert (hd == hs[index]).all(), i
        a_s, j_s = src.agent.select_action(obs)
        a_d, j_d = dst.select_action(obs[index])
        assert (a_d == a_s[index]).all() and (j_d == j_s[index]).all(), i
    want = _learners(src.agent, range(N), S)
    for j, r in enumerate(index):
        for s in range(S):
            assert _same_learner(dst.learner(j, s, with_kinv=True), want[(int(r), s)]), (j, s)
    assert _same_control(dst.control(), src.agent.control(), index)
    dst.close()
    whole = _load_learning(src, blob, None)
    assert whole.n_envs == N and whole.export_agents(ident) == blob
    whole.close()


@pytest.mark.parametrize('graph', [False, True])
def test_continuation_through_a_file_closed_loop(src, graph):
    """the agents through the file with their Kinv rebuilt, their environments through rs_fork: 24 run_resident steps record the
    source's histories, plain and as a hipGraph"""
    index = _index(np.random.default_rng(7))
    dst = _load_learning(src, src.agent.export_agents(np.arange(N, dtype=np.int32)), index)
    denv = src.new_env(len(index))
    denv.fork_from(src.env, index)
    steps = 24
    src.agent.history_begin(steps)
    dst.history_begin(steps)
    src.agent.run_resident(src.env, steps, graph=graph)
    dst.run_resident(denv, steps, graph=graph)
    hs, hd = src.agent.history_fetch(), dst.history_fetch()
    assert hs['recorded'] == hd['recorded'] == steps
    for key in KEYS:
        assert _bits(hd[key]) == _bits(hs[key][index]), key
    fs, fd = src.env.fetch(), denv.fetch()
    assert _bits(fd['obs']) == _bits(fs['obs'][index]) and _bits(fd['actions']) == _bits(fs['actions'][index])
    assert (dst.dictionary_sizes() == src.agent.dictionary_sizes()[index]).all()
    j = int(np.nonzero(index == BIG[0])[0][0])
    assert _same_learner(dst.learner(j, BIG[1], with_kinv=True), src.agent.learner(*BIG, with_kinv=True))
    dst.close()
    denv.close()


# ------------------------------------------------------------------ 4. a pruned source: not an insertion order
def test_pruned_source(golden_dir):
    """the G14 and the G17 learner pruned to 256, deployed and rebuilt: Kinv within KINV_RTOL of the pruned source's own (the
    downdated one) and of the mirror's bordering recursion over the same landmarks; then both handles continue on the rest of
    their streams with equal signs, branches and sizes wherever the margins of tests/test_gpu_prune.py hold"""
    from ranslice.kbrl_dev import VecKBRL
    streams = [(_g14(golden_dir), 4000, 500), (_g17(golden_dir), 1500, 300)]
    ag = VecKBRL(2, [10], 200, capacity=4096)
    ag.reset([[10]] * 2, [[3]] * 2)
    for e, ((xs, ys), n0, _) in enumerate(streams):
        for i in range(n0):
            ag.predict(e, 0, xs[i])
            ag.update(e, 0, xs[i], int(ys[i]))
    assert (ag.dictionary_sizes()[:, 0] > 256).all()
    ag.prune(256)
    dep = ag.deploy(np.arange(2, dtype=np.int32))
    dst = VecKBRL(2, [10], 200, capacity=4096, pool_bytes=256 << 20)
    dst.fork_from(dep, np.arange(2, dtype=np.int32), rebuild=True)
    st = dst.rebuild_stats()
    print('min_delta of the pruned slot orders: %s (eta %.1f)' % (st['min_delta'][:, 0], ETA))
    for e in range(2):
        a, b = dst.learner(e, 0, with_kinv=True), ag.learner(e, 0, with_kinv=True)
        assert a['m'] == b['m'] == 256 and _bits(a['landmarks']) == _bits(b['landmarks']) and _bits(a['coeff']) == _bits(b['coeff'])
        mr = pm.build_from_landmarks(b['landmarks'], b['coeff'], gamma=1.0)
        exact = np.asarray(pm.inv_longdouble(pm.gram_exact(b['landmarks'], 1.0)), dtype=np.float64)
        d_src, d_mir = _kinv_dist(a['kinv'], b['kinv']), _kinv_dist(a['kinv'], mr.P)
        print('dictionary %d: |rebuilt - downdated| / scale %.3e, |rebuilt - mirror| / scale %.3e; against the long double inverse of '
              'the exact Gram matrix: rebuilt %.3e, downdated %.3e' % (e, d_src, d_mir, _kinv_dist(a['kinv'], exact), _kinv_dist(b['kinv'], exact)))
        assert d_src <= KINV_RTOL and d_mir <= KINV_RTOL, (e, d_src, d_mir)
        assert np.array_equal(a['kinv'], a['kinv'].T)
    for e, ((xs, ys), n0, more) in enumerate(streams):
        compared = 0
        for i in range(n0, n0 + more):
            ya, fa = ag.predict(e, 0, xs[i])
            yd, fd = dst.predict(e, 0, xs[i])
            assert fd == pytest.approx(fa, rel=1e-8, abs=1e-9), (e, i)
            if abs(fa) > F_MARGIN:
                assert ya == yd, (e, i)
            bra, dla = ag.update(e, 0, xs[i], int(ys[i]))
            brd, dld = dst.update(e, 0, xs[i], int(ys[i]))
            if abs(fa) <= F_MARGIN or (bra and abs(dla - ETA) <= D_MARGIN):
                break       # (a decision on its threshold: the two may part here, and nothing behind it is comparable)
            assert bra == brd, (e, i, dla, dld)
            compared += 1
        print('dictionary %d: %d of %d samples compared' % (e, compared, more))
        assert compared >= more // 2, (e, compared)
        if compared == more:
            assert ag.dictionary_sizes()[e, 0] == dst.dictionary_sizes()[e, 0]
    for h in (dst, dep, ag):
        h.close()


# ------------------------------------------------------------------ 5. a reference-trained agent goes on learning
def test_reference_trained_agent_resumes(golden_dir):
    """OracleKBRL (the reference's KBRL_Control restated) consumes 1,500 samples of G17; its landmarks and coefficients are packed
    into an agent file, imported with learning=True, and device and oracle continue in lock-step for 300 samples under the
    tolerances of the G17 case of tests/test_gpu_kbrl.py: f 1e-8 relative, the sign wherever |f| > 1e-7, every branch and
    size, delta 1e-6"""
    from ranslice.kbrl_dev import VecKBRL
    xs, ys = _g17(golden_dir)
    oa = po.OracleKBRL([10], 200, [10], [3], capacity=4096)
    oa.set_seed(0)
    for i in range(1500):
        oa.predict(0, xs[i])
        oa.update(0, xs[i], int(ys[i]))
    m0 = oa.m(0)
    assert m0 >= 320
    cfg = dict(n_prbs=200, capacity=4096, dims=[10], alfa=0.05, accuracy_range=(0.99, 0.999), gamma=1.0, eta=0.1)
    blob = af.pack(cfg, [dict(landmarks=[oa.landmarks(0)], coeff=[oa.coeff(0)], action=[10], security_factors=oa.security_factors,
                              margins=oa.margins, adjusted=0, accuracies=oa.accuracies)])
    ag = VecKBRL.load_agents(blob, learning=True, pool_bytes=256 << 20)
    assert not ag.frozen and ag.dictionary_sizes()[0, 0] == m0
    ko = oa.kinv(0)
    assert _kinv_dist(ag.learner(0, 0, with_kinv=True)['kinv'], ko) <= 1e-6
    for i in range(1500, 1800):
        yp, f = ag.predict(0, 0, xs[i])
        oyp, of = oa.predict(0, xs[i])
        assert f == pytest.approx(of, rel=1e-8, abs=1e-9), i
        if abs(of) > 1e-7:
            assert yp == oyp, i
        br, dl = ag.update(0, 0, xs[i], int(ys[i]))
        obr, odl = oa.update(0, xs[i], int(ys[i]))
        assert br == obr, (i, br, obr, dl, odl)
        if br:
            assert dl == pytest.approx(odl, rel=1e-6, abs=1e-9), i
    assert ag.dictionary_sizes()[0, 0] == oa.m(0) > m0
    L = ag.learner(0, 0, with_kinv=True)
    np.testing.assert_array_equal(L['landmarks'], oa.landmarks(0))
    np.testing.assert_allclose(L['coeff'], oa.coeff(0), rtol=1e-6, atol=1e-8)
    ag.close()


# ------------------------------------------------------------------ 6. refusals and failure
def _stored(dep):
    """every stored row of an inference-only handle, through the probes of the test build"""
    out = []
    for e in range(dep.n_envs):
        for s in range(dep.S):
            r = rows(dep, e, s, 1024)
            L = dep.learner(e, s)
            out.append(b''.join(_bits(v) for v in (r['D0'], r['E'], r['idx'], r['coeff'], r['lam'], L['landmarks'], L['coeff'])))
    return out


def test_refusals_and_failure(ladder):
    from ranslice.kbrl_dev import fork_pool_bytes
    src = ladder.src
    n = src.n_envs
    ident = np.arange(n, dtype=np.int32)
    dep = src.deploy(ident)
    before = _stored(dep)
    ctl = dep.control()
    # a by-reference source, an inference-only destination
    ref = src.deploy(ident, by_reference=True)
    dst = _dev_agent(n)
    frozen = src.deploy(ident)
    for call in (lambda: dst.fork_from(ref, ident, rebuild=True), lambda: frozen.fork_from(dep, ident, rebuild=True)):
        with pytest.raises(_lib.RanSliceError) as e:
            call()
        assert e.value.code == _lib.RS_ESTATE
    with pytest.raises(_lib.RanSliceError) as e:
        dst.rebuild_stats()         # nothing replayed into it yet
    assert e.value.code == _lib.RS_ESTATE
    ref.close()
    frozen.close()
    dst.close()
    # the pool: exactly the full shells fit; one shell short does not, and leaves the destination reset and empty
    need = fork_pool_bytes(ladder.sizes)
    exact = _dev_agent(n, pool_bytes=need)
    exact.fork_from(dep, ident, rebuild=True)
    assert exact.pool()['used_bytes'] == exact.pool()['total_bytes'] == need
    assert _same_learner(exact.learner(G14_AGENT, 0, with_kinv=True), src.learner(G14_AGENT, 0, with_kinv=True))
    exact.close()
    short = _dev_agent(n, pool_bytes=need - (15360 + 32768 + 1024))
    with pytest.raises(_lib.RanSliceError) as e:
        short.fork_from(dep, ident, rebuild=True)
    assert e.value.code == _lib.RS_EOVERFLOW
    assert not short.dictionary_sizes().any() and _same_control(short.control(), ctl, ident)
    short.close()
    # a host-packed file whose dictionary repeats landmark 0 in slot 1: delta = 1 - 1 = 0 exactly, in the float32 path
    u = af.unpack(src.export_agents(ident))
    victim = (5, 0)
    assert u['m'][victim] == 65
    u['agents'][victim[0]]['landmarks'][victim[1]][1] = u['agents'][victim[0]]['landmarks'][victim[1]][0]
    bad = _dev_load(af.pack(u))
    dst = _dev_agent(n)
    with pytest.raises(_lib.RanSliceError) as e:
        dst.fork_from(bad, ident, rebuild=True)
    assert e.value.code == _lib.RS_ESTATE and '1 dictionaries' in str(e.value) and 'agent 5 slice 0' in str(e.value)
    st = dst.rebuild_stats()
    assert st['min_delta'][victim] == 0.0
    others = np.ones_like(st['min_delta'], dtype=bool)
    others[victim] = False
    assert (st['min_delta'][others] > 0).all() and _bits(st['min_delta'][others]) == _bits(ladder.min_delta[others])
    assert not dst.dictionary_sizes().any() and _same_control(dst.control(), ctl, ident)
    bad.close()
    # the same destination takes a good rebuild afterwards
    dst.fork_from(dep, ident, rebuild=True)
    for key in ((G14_AGENT, 0), (15, 0), (0, 1), victim):
        assert _same_learner(dst.learner(*key, with_kinv=True), src.learner(*key, with_kinv=True)), key
    dst.close()
    # the source was only read
    assert _stored(dep) == before
    dep.close()


# ------------------------------------------------------------------ 7. experiments_trained: the control leg from a file
def test_experiments_trained_learning_control_from_a_file(golden_dir, tmp_path):
    """2 agents trained 40 steps, 4 replicas each, 20 evaluation steps: the learning-control leg of the agents loaded from
    their file (Kinv rebuilt) gives the figures of the same-process one (full forks of the trained handle), number for number"""
    import experiments_trained as et
    import scenario_creator as sc
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    old = sc._FADING
    sc.set_fading([g['t0'], g['t1'], g['t2']])
    try:
        kw = dict(runs=range(2), train_steps=40, eval_replicas=4, eval_steps=20, capacity=256, pool_bytes=64 << 20, verbose=False,
                  learning_control=True)
        a_range = [0.99, 0.999]
        s1 = et.train_and_deploy(0, a_range, out_dir=str(tmp_path / 'same'), save_agents=str(tmp_path / 'agents'), **kw)
        s2 = et.train_and_deploy(0, a_range, out_dir=str(tmp_path / 'loaded'), load_agents=str(tmp_path / 'agents'), **kw)
        assert s2['loaded'] and s2['deployed'] == s1['deployed']
        for key in ('violations', 'occupation'):
            assert s2['learning_control'][key] == s1['learning_control'][key], key
        assert s2['learning_control']['pool']['used_bytes'] == s1['learning_control']['pool']['used_bytes']
        assert s2['learning_control']['rebuild_min_delta'] > 0
    finally:
        sc.set_fading(old)
