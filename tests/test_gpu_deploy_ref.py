"""kb_deploy_ref on the device: replicas that share their agent's read-only dictionaries against their COPY TWIN -- kb_deploy
with the same src_index, fed the same states, whose scores tests/test_gpu_scoring.py holds to tests/scoring_mirror.py bit
for bit.  Every comparison is bit for bit (a zero of either sign counts as zero): F[0 .. n_prbs], the direct-evaluation
flags and count, actions, adjusted, margins, security factors and the statistics totals.

Dictionaries are grown teacher-forced on the device through kb_predict / kb_update (scoring_mirror.random_samples / grow);
the test build is used wherever scores or rows are read (kb_dev_get_scores / kb_dev_get_rows, csrc/kb_probe.hip)."""
import ctypes as C

import numpy as np
import pytest

import scoring_mirror as sm
from ranslice import _lib
from test_gpu_scoring import _bind, _p, values_equal

pytestmark = pytest.mark.gpu

GAMMA = 1.0
DIMS = [10, 3]


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def new_agent(n_envs, dims, n_prbs, capacity, seed0=11, shared=False):
    """a reset learning handle of the test build"""
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        ag = (SharedVecKBRL if shared else VecKBRL)(n_envs, dims, n_prbs, capacity=capacity, gamma=GAMMA)
    _bind(ag.L)
    rng = np.random.default_rng(seed0)
    ag.reset(np.zeros((n_envs, len(dims)), dtype=np.int32), rng.integers(0, 4, (n_envs, len(dims))).astype(np.int32),
             seeds=np.arange(n_envs, dtype=np.uint64) + seed0)
    return ag


def grow(ag, e, s, m, seed, off_grid=(), f32=True):
    """learner (e, s) to exactly m landmarks, teacher-forced on the device"""
    rng = np.random.default_rng(seed)
    X = sm.random_samples(rng, 3 * m + 60, ag.dims[s], ag.n_prbs, f32=f32)
    size = [0]

    def update(x, y):
        br = ag.update(e, s, x, y)[0]
        size[0] += br == 2
        return br
    sm.grow(m, X, lambda x: ag.predict(e, s, x), update, lambda: size[0], set(off_grid), rng)
    assert ag.dictionary_sizes()[e, s] == m


def scores(ag):
    T = ag.n_envs * ag.S
    F, W, fd = np.zeros((T, 256)), np.zeros((T, 256)), np.zeros(T, dtype=np.int32)
    assert ag.L.kb_dev_get_scores(ag.h, _p(F, C.c_double), _p(W, C.c_double), _p(fd, C.c_int32)) == 0
    return F, fd


def rows(ag, e, s, cap):
    D0, E, co, lam, G = np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(256)
    idx = np.zeros(cap, dtype=np.int32)
    m = C.c_int32(-1)
    rc = ag.L.kb_dev_get_rows(ag.h, e, s, cap, C.byref(m), _p(D0, C.c_double), _p(E, C.c_double), _p(idx, C.c_int32),
                              _p(co, C.c_double), _p(lam, C.c_double), _p(G, C.c_double))
    assert rc == 0, rc
    m = m.value
    return dict(m=m, D0=D0[:m], E=E[:m], idx=idx[:m], coeff=co[:m], lam=lam[:m], G=G)


def random_states(n, rng, dims=DIMS):
    st = np.zeros((n, sum(dims)), dtype=np.float32)
    o = 0
    for dm in dims:
        st[:, o:o + dm] = rng.uniform(0.0, sm.SPREAD[dm], (n, dm))
        o += dm
    return st


def select_both(R, Cp, states, what=''):
    """one selection on the by-reference handle and on its copy twin: everything the contract names must be equal"""
    n = R.n_prbs
    aR, jR = R.select_action(states)
    aC, jC = Cp.select_action(states)
    FR, fdR = scores(R)
    FC, fdC = scores(Cp)
    ok = values_equal(FR[:, :n + 1], FC[:, :n + 1])
    bad = np.nonzero(~ok.all(axis=1))[0]
    assert ok.all(), (what, 'F differs for tasks', bad[:8], 'candidates', np.nonzero(~ok[bad[0]])[0][:8])
    assert (fdR == fdC).all(), (what, 'fdirect', np.nonzero(fdR != fdC)[0][:8])
    assert _bits(aR) == _bits(aC) and _bits(jR) == _bits(jC), (what, 'actions', np.nonzero((aR != aC).any(axis=1))[0][:8])
    cR, cC = R.control(), Cp.control()
    for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
        assert _bits(cR[key]) == _bits(cC[key]), (what, key)
    assert R.stats() == Cp.stats(), (what, R.stats(), Cp.stats())
    return aR, FR, fdR


# ------------------------------------------------------------------ the ladder source, shared by the cases that only read it
LADDER = [(513, 65), (321, 0), (257, 1), (256, 2), (64, 257), (65, 64)]   # (dims 10, dims 3) landmarks of agents 0 .. 5
REFS = [33, 17, 16, 15, 1, 0]                                            # replicas per agent: agent 5 is referenced by nobody
F32BAD = 1                                                               # the agent whose dims-10 dictionary holds non-float32 values
N_LADDER = 70


class Ladder:
    def __init__(self):
        self.src = new_agent(len(LADDER), DIMS, N_LADDER, capacity=640)
        for a, sizes in enumerate(LADDER):
            for s, m in enumerate(sizes):
                grow(self.src, a, s, m, 100 + 2 * a + s, f32=not (a == F32BAD and s == 0))
        self.sizes = self.src.dictionary_sizes()
        assert self.sizes.tolist() == [list(x) for x in LADDER]
        rng = np.random.default_rng(2)
        self.index = rng.permutation(np.repeat(np.arange(len(LADDER)), REFS)).astype(np.int32)   # interleaved, not sorted
        self.n = len(self.index)
        self.lm_single = self.src.learner(2, 1)['landmarks'][0, :3]

    def states(self, seed):
        """a different random state per replica; two replicas of agent 0 share one; the replicas of the single-landmark
        dictionary stand near it (it is scored in float32: further away k is below the float32 range)"""
        rng = np.random.default_rng(seed)
        st = random_states(self.n, rng)
        for j in np.nonzero(self.index == 2)[0]:
            st[j, 10:13] = (self.lm_single + rng.uniform(0.1, 0.4, 3)).astype(np.float32)
        twins = np.nonzero(self.index == 0)[0]
        st[twins[5]] = st[twins[1]]
        return st

    def deploy_pair(self, index=None):
        index = self.index if index is None else index
        return self.src.deploy(index, by_reference=True), self.src.deploy(index)

    def close(self):
        self.src.close()


@pytest.fixture(scope='module')
def ladder():
    ld = Ladder()
    yield ld
    ld.close()


def test_ladder_and_group_shapes(ladder):
    """dictionaries of 0 .. 513 landmarks (one, two and three segments; float32 rows and the f64 fall-back; dims 10 and 3)
    referenced 1, 15, 16, 17 and 33 times, interleaved: full, ragged and single-replica groups, several groups on one
    dictionary at once.  Two selections on different states, everything equal to the copy twin's; the pool is the distinct
    agents'"""
    from ranslice.kbrl_dev import deploy_pool_bytes, deploy_ref_pool_bytes
    R, Cp = ladder.deploy_pair()
    try:
        assert R.frozen and R.by_reference and Cp.frozen and not Cp.by_reference and R.n_envs == ladder.n
        want = 512 + 15360 * int(((ladder.sizes[:5].astype(np.int64) + 63) // 64).sum())
        p = R.pool()
        assert p['used_bytes'] == p['total_bytes'] == want == deploy_ref_pool_bytes(ladder.sizes, ladder.index)
        assert Cp.pool()['used_bytes'] == deploy_pool_bytes(ladder.sizes[ladder.index]) > want
        assert (R.dictionary_sizes() == ladder.sizes[ladder.index]).all()
        for j in (0, 1, ladder.n - 1, int(np.nonzero(ladder.index == 4)[0][0])):
            for s in range(2):
                a, b = R.learner(j, s), ladder.src.learner(int(ladder.index[j]), s)
                assert a['m'] == b['m'] and _bits(a['landmarks']) == _bits(b['landmarks']) and _bits(a['coeff']) == _bits(b['coeff'])
        for k, seed in enumerate((3, 4)):
            st = ladder.states(seed)
            _, F, fd = select_both(R, Cp, st, 'selection %d' % k)
            empty = np.nonzero(ladder.index == 1)[0] * 2 + 1
            assert not F[empty, :N_LADDER + 1].any(), 'an empty dictionary scores zero everywhere'
            twins = np.nonzero(ladder.index == 0)[0]
            assert _bits(F[2 * twins[5]:2 * twins[5] + 2, :N_LADDER + 1]) == _bits(F[2 * twins[1]:2 * twins[1] + 2, :N_LADDER + 1])
            assert F[:, :N_LADDER + 1].any(axis=1).sum() > ladder.n
    finally:
        R.close()
        Cp.close()


@pytest.mark.parametrize('n_prbs', [1, 17, 64, 200, 255])
def test_candidate_grid_edges(n_prbs):
    """tile (n / 16 + 1), group (64 g <= n) and KA edges of the product, dictionaries of 2, 65 and 300 landmarks, 17 replicas per
    agent (a full group and a single-replica one per dictionary)"""
    src = new_agent(3, DIMS, n_prbs, capacity=320)
    try:
        for a, sizes in enumerate([(2, 65), (65, 300), (300, 2)]):
            for s, m in enumerate(sizes):
                grow(src, a, s, m, 600 + 7 * n_prbs + 2 * a + s)
        index = np.random.default_rng(n_prbs).permutation(np.repeat(np.arange(3), 17)).astype(np.int32)
        R, Cp = src.deploy(index, by_reference=True), src.deploy(index)
        rng = np.random.default_rng(n_prbs + 1)
        for k in range(2):
            _, F, _ = select_both(R, Cp, random_states(len(index), rng), 'n_prbs %d, selection %d' % (n_prbs, k))
        assert F[:, :n_prbs + 1].any()
        R.close()
        Cp.close()
    finally:
        src.close()


def test_direct_evaluation_off_the_grid_and_the_mirror():
    """0, 48, 49 and 130 landmarks off the candidate grid: the list holds 48, so the last two take the recompute path -- D0 / E
    formed again from the coordinates, where the copy reads its stored rows.  Then the learning source itself selects on the
    states of one replica per agent, and the mirror fed with ITS rows gives the by-reference handle's F"""
    n, m, counts = 50, 150, [0, 48, 49, 130]
    src = new_agent(len(counts), [10], n, capacity=192)
    try:
        for a, k in enumerate(counts):
            grow(src, a, 0, m, 2000 + k, off_grid=range(3, 3 + k))
        index = np.random.default_rng(5).permutation(np.repeat(np.arange(4), 6)).astype(np.int32)
        R, Cp = src.deploy(index, by_reference=True), src.deploy(index)
        rng = np.random.default_rng(6)
        for k in range(2):
            st = random_states(len(index), rng, [10])
            _, F, fd = select_both(R, Cp, st, 'selection %d' % k)
            for j, a in enumerate(index):
                assert fd[j] == ((3 | (counts[a] << 8)) if counts[a] else 0), (j, a, hex(fd[j]))
        first = [int(np.nonzero(index == a)[0][0]) for a in range(4)]
        src.select_action(st[first])
        for a, j in enumerate(first):
            r = rows(src, a, 0, 192)
            out = sm.ordered_scores(r['E'], r['idx'], r['coeff'], r['lam'], r['D0'], r['G'], n, GAMMA)
            assert fd[j] == out['fdirect']
            ok = values_equal(F[j, :n + 1], out['F'])
            assert ok.all(), ('the mirror', a, np.nonzero(~ok)[0][:8])
        R.close()
        Cp.close()
    finally:
        src.close()


def test_band_settled_rule_and_all_underflow_ties():
    """replicas in a band state (every E_j in (5e-324, 1e-300) or zero) beside replicas in random states, in the same groups; a
    dictionary whose binned sum crosses 1e-240 along the candidates; then the state where everything underflows and every
    candidate is an exact tie decided by the replica's own Philox stream -- action, draws consumed (the statistics) and a
    FOLLOWING selection equal the copy twin's"""
    n = 255
    src = new_agent(2, DIMS, n, capacity=320)
    try:
        grow(src, 0, 0, 257, 3010)
        grow(src, 0, 1, 257, 3003)
        grow(src, 1, 0, 40, 3011)
        for x in [np.array([0.5 + 23.493, 0.5, 0.5, 0.0]), np.array([26.8, 0.5, 0.5, 1.0]), np.array([0.5, 26.9, 0.5, 100.0 / 255.0])]:
            y, _ = src.predict(1, 1, x)
            assert src.update(1, 1, x, -y if y else 1)[0] == 2
        index = np.array([0, 1, 0, 0, 1, 0, 1, 0, 0, 1, 1, 0], dtype=np.int32)
        R, Cp = src.deploy(index, by_reference=True), src.deploy(index)
        rng = np.random.default_rng(8)
        st = random_states(len(index), rng)
        L0, L1 = src.learner(0, 0)['landmarks'], src.learner(0, 1)['landmarks']
        for j in np.nonzero(index == 0)[0][::2]:      # every other replica of agent 0: the band
            st[j, :10] = sm.band_coordinate(L0[:, :10])
            st[j, 10:] = sm.band_coordinate(L1[:, :3])
        for j in np.nonzero(index == 1)[0][:3]:       # three replicas of agent 1: the crafted crossing
            st[j, :10] = 1.0
            st[j, 10:] = 0.5
        _, F, fd = select_both(R, Cp, st, 'band and settled')
        j0, j1 = int(np.nonzero(index == 0)[0][0]), int(np.nonzero(index == 1)[0][0])
        for s in (0, 1):
            t = 2 * j0 + s
            assert fd[t] & 1 and (fd[t] >> 8) >= 1 and F[t, :n + 1].any(), 'the band terms are not zero'
        t = 2 * j1 + 1
        settled = np.abs(F[t, :n + 1]) >= sm.KB_F_SETTLED
        assert fd[t] == (1 | (2 << 8)) and settled.any() and (~settled).any()
        stats0 = R.stats()
        far = np.full((len(index), 13), 60.0, dtype=np.float32)
        for k in range(2):
            act, F, fd = select_both(R, Cp, far, 'all underflow %d' % k)
            assert not F[:, :n + 1].any() and not fd.any()
        assert R.stats()[0] > stats0[0]
        select_both(R, Cp, random_states(len(index), rng), 'the selection that follows')
        R.close()
        Cp.close()
    finally:
        src.close()


def test_independence_of_grouping(ladder):
    """the same (agent, state) pairs under a permuted src_index, the states permuted alike: other groups, other columns of the
    product, other neighbours -- every replica's F and action follow it bit for bit"""
    R1 = ladder.src.deploy(ladder.index, by_reference=True)
    perm = np.random.default_rng(12).permutation(ladder.n)
    R2 = ladder.src.deploy(ladder.index[perm], by_reference=True)
    try:
        st = ladder.states(13)
        a1, j1 = R1.select_action(st)
        a2, j2 = R2.select_action(st[perm])
        F1, fd1 = scores(R1)
        F2, fd2 = scores(R2)
        n = N_LADDER
        t = (2 * perm[:, None] + np.arange(2)[None, :]).reshape(-1)
        assert _bits(F2[:, :n + 1]) == _bits(F1[t, :n + 1]) and _bits(fd2) == _bits(fd1[t])
        assert _bits(a2) == _bits(a1[perm]) and _bits(j2) == _bits(j1[perm])
        assert _bits(R2.control()['margins']) == _bits(R1.control()['margins'][perm])
    finally:
        R1.close()
        R2.close()


def test_dictionaries_are_read_only(ladder):
    """the rows of every stored dictionary -- D0, E, grid indices, coefficients, last coordinates -- are bitwise the same
    before the first and after the third selection: the kernel writes nothing into a page"""
    R = ladder.src.deploy(ladder.index, by_reference=True)
    try:
        first = [int(np.nonzero(ladder.index == a)[0][0]) for a in range(5)]
        keys = ('D0', 'E', 'idx', 'coeff', 'lam')

        def snapshot():
            return {(a, s): rows(R, j, s, 640) for a, j in enumerate(first) for s in range(2)}
        before = snapshot()
        for (a, s), r in before.items():
            assert r['m'] == LADDER[a][s]
        for seed in (20, 21, 22):
            R.select_action(ladder.states(seed))
        after = snapshot()
        for key, r in before.items():
            for k in keys:
                assert _bits(r[k]) == _bits(after[key][k]), (key, k)
        last = ladder.index.tolist().index(0, first[0] + 1)     # another replica of agent 0 reads the same stored rows
        assert all(_bits(rows(R, last, 0, 640)[k]) == _bits(after[(0, 0)][k]) for k in keys)
    finally:
        R.close()


def test_source_continues_untouched():
    """a source that goes on learning after kb_deploy_ref equals a twin of itself that was never deployed from: landmarks,
    coefficients, Kinv; and the deployment keeps the dictionaries of the moment it was made"""
    n = 50
    A, B = (new_agent(2, DIMS, n, capacity=256) for _ in range(2))
    try:
        for ag in (A, B):
            grow(ag, 0, 0, 130, 7000)
            grow(ag, 0, 1, 70, 7001)
            grow(ag, 1, 0, 20, 7002)
        index = np.array([1, 0, 0, 1, 0], dtype=np.int32)
        R = A.deploy(index, by_reference=True)
        kept = R.learner(1, 0)
        rng = np.random.default_rng(30)
        R.select_action(random_states(5, rng))
        X = sm.random_samples(np.random.default_rng(31), 60, 10, n)
        for ag in (A, B):
            for i, x in enumerate(X):
                ag.predict(0, 0, x)
                ag.update(0, 0, x, 1 if i % 3 else -1)
        R.select_action(random_states(5, rng))
        assert A.dictionary_sizes()[0, 0] > 130
        for e in range(2):
            for s in range(2):
                a, b = A.learner(e, s, with_kinv=True), B.learner(e, s, with_kinv=True)
                assert a['m'] == b['m'] and all(_bits(a[k]) == _bits(b[k]) for k in ('landmarks', 'coeff', 'kinv')), (e, s)
        now = R.learner(1, 0)
        assert now['m'] == kept['m'] == 130 and _bits(now['landmarks']) == _bits(kept['landmarks']) and _bits(now['coeff']) == _bits(kept['coeff'])
        R.close()
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ closed loop
@pytest.fixture(scope='module', params=[0, 2])
def trained(request, golden_dir):
    from test_gpu_agent_fork import Source
    s = Source(golden_dir, request.param, grow=1500, tail=False)
    yield s
    s.close()


@pytest.mark.parametrize('graph', [False, True])
def test_closed_loop(trained, graph):
    """40 replicas of 3 trained agents (one of them past 320 landmarks, off-grid and non-float32 landmarks in scenario 2) on a
    fresh environment, the same seeds on both sides: 60 steps of run_resident, plain and as a replayed hipGraph"""
    from test_gpu_agent_fork import BIG, KEYS
    src = trained
    rng = np.random.default_rng(40)
    index = rng.permutation(np.concatenate([[BIG[0], 5, 20], rng.choice([BIG[0], 5, 20], 37)])).astype(np.int32)
    steps = 60
    got = []
    for by_ref in (True, False):
        ag = src.agent.deploy(index, by_reference=by_ref)
        env = src.new_env(len(index), seed=91)
        env.reset()
        env.step(ag.control()['action'])
        ag.history_begin(steps)
        ag.run_resident(env, steps, graph=graph)
        got.append((ag.history_fetch(), env.fetch(), ag.control(), ag.stats()))
        ag.close()
        env.close()
    (hr, fr, cr, sr), (hc, fc, cc, sc) = got
    assert hr['recorded'] == hc['recorded'] == steps
    for key in KEYS:
        assert _bits(hr[key]) == _bits(hc[key]), key
    for key in ('reward', 'obs', 'labels', 'violations', 'actions'):
        assert _bits(fr[key]) == _bits(fc[key]), key
    for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
        assert _bits(cr[key]) == _bits(cc[key]), key
    assert sr == sc and sr[0] > 0
    assert hr['resources'].any()


# ------------------------------------------------------------------ refusals
def test_refusals(ladder):
    """what a by-reference handle refuses, by code and with a message that names the call; a copy-deployed handle as the source
    is fine; and after all the refusals the handle still selects as its copy twin does"""
    R, Cp = ladder.deploy_pair()
    n = ladder.n
    idx = np.arange(4, dtype=np.int32)
    x = np.zeros(11)
    st = ladder.states(50)
    zero = np.zeros((n, 2), dtype=np.int32)
    full = new_agent(4, DIMS, N_LADDER, capacity=640)
    shared = new_agent(4, DIMS, N_LADDER, capacity=640, shared=True)
    try:
        estate = dict(
            update_control=lambda: R.update_control(st, zero, zero + 1), kb_update=lambda: R.update(0, 0, x, 1),
            set_learning=lambda: R.set_learning(True), get_learner=lambda: R.learner(0, 0, with_kinv=True),
            save_state=lambda: R.save_state(), load_state=lambda: R.load_state(np.zeros(256, dtype=np.uint8)),
            kb_reset=lambda: R.reset(zero, zero), kb_predict=lambda: R.predict(0, 0, x), kernel_row=lambda: R.kernel_row(0, 0),
            kb_prune=lambda: R.prune(64), kb_deploy=lambda: R.deploy(idx), kb_deploy_ref=lambda: R.deploy(idx, by_reference=True),
            kb_fork=lambda: full.fork_from(R, idx))
        for name, call in estate.items():
            with pytest.raises(_lib.RanSliceError) as e:
                call()
            assert e.value.code == _lib.RS_ESTATE, name
            assert name in str(e.value), (name, str(e.value))
        bad = ladder.index.copy()
        bad[7] = len(LADDER)
        for call in (lambda: ladder.src.deploy(bad, by_reference=True), lambda: shared.deploy(idx, by_reference=True)):
            with pytest.raises(_lib.RanSliceError) as e:
                call()
            assert e.value.code == _lib.RS_EINVAL
        select_both(R, Cp, st, 'after the refusals')
        # a copy-deployed handle fans out by reference too: replica j of R2 is agent index[sub[j]] of the source
        sub = np.random.default_rng(51).integers(0, n, 40).astype(np.int32)
        R2, C2 = Cp.deploy(sub, by_reference=True), Cp.deploy(sub)
        select_both(R2, C2, st[sub], 'deployed from a copy-deployed handle')
        R2.close()
        C2.close()
    finally:
        for h in (R, Cp, full, shared):
            h.close()
