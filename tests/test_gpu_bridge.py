"""kb_unshare / kb_share on the device: dictionaries cross between a shared-dictionary handle and a per-replica one bit for
bit, in both directions, and whoever receives them goes on as the project's own references say.

Dictionaries are grown teacher-forced through kb_predict / kb_update (scoring_mirror.random_samples / grow); the test build is
used wherever scores are read (kb_dev_get_scores, csrc/kb_probe.hip).  The shape of every ladder case: n_prbs 24, gamma 1.0,
capacity 640, dims [10, 10, 10, 3, 3, 10, 3]; the sizes {0, 1, 2, 63, 64, 65, 129, 193, 257} are spread over the seven slices of
two shared handles -- 129 and 193 reach the upper-tile index b + 1 + bi with bi > 0, 257 crosses KB_GEMM_M; one dictionary
carries three off-grid landmarks and one dims-10 dictionary is grown from values that are no float32 numbers.

Not covered here: the refusal of handles on different devices (one GPU), and ranks (no second GPU either)."""
import ctypes as C
import os

import numpy as np
import pytest

import scoring_mirror as sm
from ranslice import _lib, agent_file as af
from test_gpu_deploy_ref import _bits, new_agent, random_states, scores
from test_gpu_scoring import values_equal

pytestmark = pytest.mark.gpu

N_PRBS, CAP = 24, 640
DIMS = [10, 10, 10, 3, 3, 10, 3]
#           slice:  0    1    2   3    4   5   6
LADDER_X = [257, 129, 64, 193, 1, 65, 0]
LADDER_Y = [2, 63, 0, 65, 129, 193, 257]
OFFGRID = {'X': (3, (5, 70, 130)), 'Y': (4, (1, 64, 100))}   # ladder -> (slice, the landmarks that get an off-grid last coordinate)
F32BAD = {'X': 1, 'Y': 5}                                     # ladder -> the dims-10 slice grown from non-float32 values
INDEX_X = [2, 0, 2, 3, 1]
INDEX_Y = [1, 0, 1]
RS_EINVAL, RS_EOVERFLOW, RS_ESTATE = -1, -2, -4


def in_dev(fn, *a, **k):
    """fn(...) with the handles it creates coming from the test build"""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        return fn(*a, **k)


def grow_dict(ag, e, s, m, seed, off_grid=(), f32=True):
    """dictionary s of `ag` (through replica / agent e) to exactly m landmarks, teacher-forced on the device"""
    rng = np.random.default_rng(seed)
    X = sm.random_samples(rng, 3 * m + 60, ag.dims[s], ag.n_prbs, f32=f32)
    size = [0]

    def update(x, y):
        br = ag.update(e, s, x, y)[0]
        size[0] += br == 2
        return br
    sm.grow(m, X, lambda x: ag.predict(e, s, x), update, lambda: size[0], set(off_grid), rng)
    assert ag.learner(e, s)['m'] == m


def grow_ladder(ag, e, name, seed):
    ladder = LADDER_X if name == 'X' else LADDER_Y
    for s, m in enumerate(ladder):
        grow_dict(ag, e, s, m, seed + s, off_grid=OFFGRID[name][1] if s == OFFGRID[name][0] else (), f32=s != F32BAD[name])


def flags(ag):
    e = np.zeros(ag.n_envs, dtype=np.int32)
    assert ag.L.kb_get_flags(ag.h, e.ctypes.data_as(C.POINTER(C.c_int32))) == 0
    return e


def learners(ag, e=0, kinv=True):
    return [ag.learner(e, s, with_kinv=kinv) for s in range(ag.S)]


def same_learner(a, b, kinv=True):
    return (a['m'] == b['m'] and _bits(a['landmarks']) == _bits(b['landmarks']) and _bits(a['coeff']) == _bits(b['coeff'])
            and (not kinv or a['m'] == 0 or _bits(a['kinv']) == _bits(b['kinv'])))


CTL_KEYS = ('action', 'adjusted', 'margins', 'security_factors', 'accuracies')


def same_control(cA, cX, index=None, what=''):
    for key in CTL_KEYS:
        want = cX[key] if index is None else cX[key][np.asarray(index)]
        assert _bits(cA[key]) == _bits(want), (what, key)


def call(L, fn, dst, src, *args):
    """a bridge entry point at the C ABI -> (code, message)"""
    rc = getattr(L, fn)(dst.h, src.h, *args)
    return rc, L.kb_last_error(dst.h).decode()


def idx(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(C.POINTER(C.c_int32))


def tie_counters(h):
    """the tie-break counters [n_envs, S] of a learning handle, read out of its checkpoint (kb_save_state: a 72-byte header, then
    every device array in the order kb_create allocates them; the pool's part is as long as the header's fourth word says).
    The seeds follow the counters: they are known, and finding them there is the check that the offset is right."""
    blob = h.save_state()
    used = int(np.frombuffer(blob[24:32].tobytes(), dtype=np.uint64)[0])
    shared = bool(h.cfg.shared_dictionary)
    T, N = h.n_envs * h.S, h.n_envs
    ND = h.S if shared else T
    shells = (h.capacity + 63) // 64
    before = [4 * ND, 8 * ND * shells, 4 * ND * 256, 8, 8 * 264, 4 * ND, 4 * (T + 4)] + [4 * T] * 5 + \
             [8 * T, 8 * T, 8 * 256 * T, 8 * (T + 1), 8 * (T + 1), 64, 4 * 2 * 4097, 4 * 2 * T, 8 * used, 8 * T, 4 * T]
    at = 72 + sum(before)
    ctr = np.frombuffer(blob[at:at + 4 * T].tobytes(), dtype=np.uint32).reshape(N, h.S)
    seeds = np.frombuffer(blob[at + 4 * T:at + 4 * T + 8 * N].tobytes(), dtype=np.uint64)
    return ctr, seeds


def clone_shared(X):
    """a second shared handle in X's state (checkpoint and restore): what the cases that go on learning consume instead of X"""
    Xc = new_agent(X.n_envs, X.dims, X.n_prbs, X.capacity, shared=True)
    Xc.load_state(X.save_state())
    return Xc


def select_same(P, Q, states, what=''):
    aP, jP = P.select_action(states)
    aQ, jQ = Q.select_action(states)
    assert _bits(aP) == _bits(aQ) and _bits(jP) == _bits(jQ), (what, 'actions')
    cP, cQ = P.control(), Q.control()
    for key in ('action', 'adjusted', 'margins'):
        assert _bits(cP[key]) == _bits(cQ[key]), (what, key)


def control_batch(n, rng, dims=DIMS, n_prbs=N_PRBS):
    """states, actions and labels of one update_control call"""
    return (random_states(n, rng, dims), rng.integers(0, n_prbs + 1, (n, len(dims))).astype(np.int32),
            rng.choice(np.array([-1, 1], dtype=np.int32), (n, len(dims))))


class World:
    """the two shared ladders, built once and only read by the cases"""

    def __init__(self):
        self.X = new_agent(4, DIMS, N_PRBS, CAP, seed0=21, shared=True)
        self.Y = new_agent(2, DIMS, N_PRBS, CAP, seed0=31, shared=True)
        grow_ladder(self.X, 1, 'X', 500)    # (through replica 1: the dictionaries are everybody's)
        grow_ladder(self.Y, 0, 'Y', 600)
        assert self.X.dictionary_sizes().tolist() == LADDER_X and self.Y.dictionary_sizes().tolist() == LADDER_Y
        rng = np.random.default_rng(7)
        for h in (self.X, self.Y):          # actions, margins, adjusted and tie counters away from their reset values, per replica
            h.select_action(random_states(h.n_envs, rng, DIMS))
            h.select_action(random_states(h.n_envs, rng, DIMS))
        assert len({_bits(self.X.control()['action'][r]) for r in range(4)}) > 1

    def get(self, name):
        return (self.X, INDEX_X) if name == 'X' else (self.Y, INDEX_Y)

    def close(self):
        self.X.close()
        self.Y.close()


@pytest.fixture(scope='module')
def world():
    w = World()
    yield w
    w.close()


# ------------------------------------------------------------------ 1. unshare, data
@pytest.mark.parametrize('name', ['X', 'Y'])
def test_unshare_data(world, name):
    """every agent holds the shared dictionaries as bytes (landmarks, coefficients, Kinv), the control state of its replica,
    its flags; statistics restart; the same call into a fresh handle gives the same checkpoint bytes"""
    X, index = world.get(name)
    want = learners(X)
    for s, w in enumerate(want):      # precondition on the shared mode itself: Kinv is symmetric bit for bit
        assert w['m'] == 0 or _bits(w['kinv']) == _bits(np.ascontiguousarray(w['kinv'].T)), s
    cX, fX = X.control(), flags(X)
    A = in_dev(X.to_agents, index)
    B = in_dev(X.to_agents, index)
    try:
        assert not A.frozen and A.n_envs == len(index) and A.dims == DIMS
        for j in range(len(index)):
            for s in range(len(DIMS)):
                assert same_learner(A.learner(j, s, with_kinv=True), want[s]), (j, s)
        same_control(A.control(), cX, index)
        assert _bits(flags(A)) == _bits(fX[np.asarray(index)])
        assert (A.dictionary_sizes() == np.tile(X.dictionary_sizes(), (len(index), 1))).all()
        assert A.stats() == [0, 0, 0, 0]
        assert _bits(A.save_state()) == _bits(B.save_state())
        # the source is as it was
        assert all(same_learner(a, b) for a, b in zip(learners(X), want))
        same_control(X.control(), cX)
    finally:
        A.close()
        B.close()


def test_unshare_after_learning_steps():
    """a small fleet that has LEARNED together (three shared steps: accuracies, security factors and hits differ per replica)"""
    dims = [3, 10]
    Z = new_agent(4, dims, N_PRBS, 128, seed0=41, shared=True)
    A = None
    try:
        rng = np.random.default_rng(8)
        for _ in range(3):
            Z.update_control(*control_batch(4, rng, dims))
        Z.select_action(random_states(4, rng, dims))
        cZ = Z.control()
        assert len({_bits(cZ['accuracies'][r]) for r in range(4)}) > 1 and Z.dictionary_sizes().min() > 0
        A = in_dev(Z.to_agents, INDEX_X)
        same_control(A.control(), cZ, INDEX_X)
        want = learners(Z)
        for j in range(5):
            for s in range(2):
                assert same_learner(A.learner(j, s, with_kinv=True), want[s]), (j, s)
    finally:
        Z.close()
        if A is not None:
            A.close()


def test_bridge_time_reports_the_plan(world):
    """kb_bridge_time_ms: with kernel timing on in the destination the gather's device time is positive, and the bytes are the
    plan's -- written: everything the destination's pool holds above its 512-byte preamble; read (kb_unshare): that less the
    partial-sum areas, 1 KB per stored tile of every agent's copy; read (kb_share): as much as written, every off-diagonal
    lower tile once per orientation.  Without timing the time is 0 and the bytes are still reported."""
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL, fork_pool_bytes, shared_pool_bytes
    X, index = world.get('X')
    shells = (np.asarray(LADDER_X) + 63) // 64
    tiles = int((shells * (shells + 1) // 2).sum())
    pool = fork_pool_bytes(np.tile(LADDER_X, (len(index), 1)))
    made = []
    try:
        for timing in (True, False):
            A = in_dev(VecKBRL, len(index), DIMS, N_PRBS, capacity=CAP, gamma=1.0, pool_bytes=pool)
            made.append(A)
            assert A.bridge_time_ms() == dict(ms=0.0, read_bytes=0, written_bytes=0), 'before any call'
            A.set_kernel_timing(timing)
            A.unshare_from(X, index)
            bt = A.bridge_time_ms()
            assert bt['written_bytes'] == A.pool()['used_bytes'] - 512 == pool - 512
            assert bt['read_bytes'] == bt['written_bytes'] - len(index) * tiles * 1024
            assert (bt['ms'] > 0.0) == timing, bt
            Sh = in_dev(SharedVecKBRL, 3, DIMS, N_PRBS, capacity=CAP, gamma=1.0)
            made.append(Sh)
            Sh.set_kernel_timing(timing)
            Sh.share_from(A, 1)
            bt = Sh.bridge_time_ms()
            assert bt['written_bytes'] == bt['read_bytes'] == Sh.pool()['used_bytes'] - 512 == shared_pool_bytes(LADDER_X) - 512
            assert (bt['ms'] > 0.0) == timing, bt
        # an overflow gathers no shell: nothing is counted
        tight = in_dev(VecKBRL, 2, DIMS, N_PRBS, capacity=CAP, gamma=1.0, pool_bytes=64 * 8 + 14 * (30 * 64 + 4096 + 128) * 8)
        made.append(tight)
        rc, _ = call(X.L, 'kb_unshare', tight, X, idx([0, 1])[1])
        assert rc == RS_EOVERFLOW and tight.bridge_time_ms()['written_bytes'] == 0
    finally:
        for h in made:
            h.close()


# ------------------------------------------------------------------ 2. unshare, pages
def test_unshare_pages_against_the_import_twin(world):
    """The twin: X's landmarks and coefficients, pulled through kb_get_learner, packed on the host with X's control state for the
    same src_index and imported (kb_import_agents writes its pages from the values alone) -- a handle whose scores the suite
    already holds to the mirror.  Scores F[0 .. n_prbs], the direct-evaluation flags, actions, adjusted and margins of the
    unshared handle equal the twin's bit for bit on random states and where everything underflows: the grid-index rows, chain
    links, heads, off-grid counts and float32 rows crossed intact.  The twin's seeds and tie-break counters are X's own, read
    out of X's checkpoint (tie_counters): nothing in the twin comes from the handle under test."""
    from ranslice.kbrl_dev import VecKBRL
    X, index = world.get('X')
    A = in_dev(X.to_agents, index)
    T = None
    try:
        cX = X.control()
        ctr, seeds = tie_counters(X)
        assert seeds.tolist() == [21, 22, 23, 24] and ctr.any(), 'the selections of the fixture drew ties (the empty dictionary)'
        mine = af.unpack(A.export_agents(np.arange(len(index))))['agents']
        assert all(mine[j]['tie_ctr'].tolist() == ctr[r].tolist() and mine[j]['seed'] == seeds[r] for j, r in enumerate(index))
        L = learners(X, kinv=False)
        cfg = dict(n_prbs=N_PRBS, capacity=CAP, dims=DIMS, alfa=X.cfg.alfa, accuracy_range=(X.cfg.acc_lo, X.cfg.acc_hi), gamma=X.cfg.gamma,
                   eta=X.cfg.eta)
        agents = [dict(landmarks=[l['landmarks'] for l in L], coeff=[l['coeff'] for l in L], action=cX['action'][r],
                       security_factors=cX['security_factors'][r], margins=cX['margins'][r], adjusted=cX['adjusted'][r],
                       accuracies=cX['accuracies'][r], seed=int(seeds[r]), tie_ctr=ctr[r], flags=int(flags(X)[r]))
                  for j, r in enumerate(index)]
        T = in_dev(VecKBRL.load_agents, af.pack(cfg, agents))
        rng = np.random.default_rng(9)
        states = [random_states(len(index), rng, DIMS) for _ in range(2)] + [np.full((len(index), sum(DIMS)), 60.0, dtype=np.float32)] + \
                 [random_states(len(index), rng, DIMS)]
        for k, st in enumerate(states):
            aA, jA = A.select_action(st)
            aT, jT = T.select_action(st)
            FA, fdA = scores(A)
            FT, fdT = scores(T)
            ok = values_equal(FA[:, :N_PRBS + 1], FT[:, :N_PRBS + 1])
            assert ok.all(), (k, 'F differs for tasks', np.nonzero(~ok.all(axis=1))[0][:8])
            assert (fdA == fdT).all(), (k, 'fdirect', np.nonzero(fdA != fdT)[0][:8])
            assert _bits(aA) == _bits(aT) and _bits(jA) == _bits(jT), (k, 'actions')
            cA, cT = A.control(), T.control()
            for key in ('action', 'adjusted', 'margins'):
                assert _bits(cA[key]) == _bits(cT[key]), (k, key)
            if k == 0:
                assert FA[:, :N_PRBS + 1].any(axis=1).sum() >= 4 * len(index)
                off = fdA.reshape(len(index), len(DIMS))[:, OFFGRID['X'][0]]
                assert (off == (3 | (3 << 8))).all(), 'the three off-grid landmarks take the direct evaluation'
            if k == 2:
                assert not FA[:, :N_PRBS + 1].any()
    finally:
        A.close()
        if T is not None:
            T.close()


# ------------------------------------------------------------------ 3. round trips
def test_round_trip_shared_agents_shared(world):
    """X -> A -> kb_share(dict_agent = 1) -> X': the dictionaries as bytes, the same selections (ties included: the size-0 and
    all-underflow cases draw), and after three identical learning steps on both still the same bytes"""
    X0, index = world.get('X')
    X = clone_shared(X0)
    A = in_dev(X.to_agents, index)
    X2 = None
    try:
        # replica r of X' takes the control state of an agent that holds replica r's: index = [2, 0, 2, 3, 1]
        X2 = in_dev(A.to_shared, 1, 4, ctl_index=[1, 4, 0, 3])
        assert X2.dictionary_sizes().tolist() == LADDER_X
        assert all(same_learner(a, b) for a, b in zip(learners(X2), learners(X)))
        same_control(X2.control(), X.control())
        assert _bits(flags(X2)) == _bits(flags(X))
        rng = np.random.default_rng(10)
        select_same(X, X2, random_states(4, rng, DIMS), 'first selection')
        select_same(X, X2, np.full((4, sum(DIMS)), 60.0, dtype=np.float32), 'all underflow')
        for k in range(3):
            st, ac, lb = control_batch(4, rng)
            hX, h2 = X.update_control(st, ac, lb), X2.update_control(st, ac, lb)
            assert _bits(hX) == _bits(h2) and X.rounds_last == X2.rounds_last, k
        assert X.dictionary_sizes().sum() > sum(LADDER_X), 'the steps learned something'
        assert all(same_learner(a, b) for a, b in zip(learners(X2), learners(X)))
        same_control(X2.control(), X.control())
        select_same(X, X2, random_states(4, rng, DIMS), 'after learning')
    finally:
        for h in (X, A, X2):
            if h is not None:
                h.close()


def test_share_into_a_used_handle_continues_as_a_fresh_one(world):
    """kb_share into a destination that has LEARNED -- it holds a dictionary beyond KB_GEMM_M scored on the matrix cores (Q, F
    and E laid out for its own landmarks), proposal cursors of its last rounds, work areas of its last apply, and larger
    dictionaries than the ones it receives in some slices -- against the same call into a handle that was never used: equal
    bytes at once, the same selections, and the same bytes after three identical learning steps.  Everything the shared mode
    derives from a dictionary is rebuilt from the new ones."""
    X, _ = world.get('X')
    Y, _ = world.get('Y')
    used = clone_shared(Y)              # its slice 6 holds 257 landmarks where the source has none, its slice 0 two where it has 257
    A = in_dev(X.to_agents, [3, 1, 0])
    fresh = None
    try:
        rng = np.random.default_rng(18)
        for k in range(3):
            used.update_control(*control_batch(2, rng))
            used.select_action(random_states(2, rng, DIMS))
        assert used.dictionary_sizes().sum() > sum(LADDER_Y)
        fresh = in_dev(A.to_shared, 2, 2, ctl_index=[1, 0])
        used.share_from(A, 2, [1, 0])
        assert used.dictionary_sizes().tolist() == fresh.dictionary_sizes().tolist() == LADDER_X
        assert all(same_learner(a, b) for a, b in zip(learners(used), learners(fresh)))
        same_control(used.control(), fresh.control())
        assert used.stats() == fresh.stats() == [0, 0, 0, 0]
        select_same(used, fresh, random_states(2, rng, DIMS), 'first selection')
        for k in range(3):
            st, ac, lb = control_batch(2, rng)
            assert _bits(used.update_control(st, ac, lb)) == _bits(fresh.update_control(st, ac, lb)), k
            assert used.rounds_last == fresh.rounds_last, k
            select_same(used, fresh, random_states(2, rng, DIMS), 'selection %d' % k)
        assert used.dictionary_sizes().sum() > sum(LADDER_X), 'the steps learned something'
        assert all(same_learner(a, b) for a, b in zip(learners(used), learners(fresh)))
        same_control(used.control(), fresh.control())
        assert used.stats() == fresh.stats()
    finally:
        for h in (used, A, fresh):
            if h is not None:
                h.close()


def test_share_into_a_handle_inside_a_resident_loop(world):
    """The destination steps a simulator in the device-resident loop, with a dictionary beyond KB_GEMM_M: after every step its
    scoring products (workF / workE) describe the observation it keeps as d_prev_state against ITS dictionaries, and the next
    step's first scan would reuse them (gemm_fresh).  kb_share in that state, then three closed-loop steps, against a
    never-used handle that received the same call and steps a fork of the simulator: the same dictionaries, bytes and all, the
    same control state and the same actions in the simulators' buffers -- the stale products are not reused."""
    from ranslice.config import make_config, EMBB_A, MMTC_A
    from ranslice.fading import synth_fading
    from ranslice.vec_env import VecRanSlice
    n = 8
    cfg = make_config(2, n_envs=n)
    dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
    fading = [synth_fading(k, 512) for k in range(3)]
    rng = np.random.default_rng(19)
    ia = np.concatenate([rng.integers(EMBB_A[0], EMBB_A[1], size=(n, cfg.n_embb)), rng.integers(MMTC_A[0], MMTC_A[1], size=(n, cfg.n_mmtc))],
                        axis=1).astype(np.int32)
    made = []

    def mk(h):
        made.append(h)
        return h
    try:
        U = mk(new_agent(n, dims, cfg.n_prbs, CAP, seed0=81, shared=True))
        P = mk(new_agent(1, dims, cfg.n_prbs, CAP, seed0=91))
        grow_dict(U, 0, 0, 257, 1000)
        grow_dict(P, 0, 0, 257, 1001)
        grow_dict(P, 0, 1, 5, 1002)
        env_u = mk(in_dev(VecRanSlice, n_envs=n, cfg=cfg, fading=fading, seed=5))
        env_u.reset()
        env_u.enqueue_step(ia)
        for _ in range(3):
            U.step_resident(env_u)
            env_u.step_resident()
        assert U.dictionary_sizes()[0] >= 257
        env_f = mk(in_dev(VecRanSlice, n_envs=n, cfg=cfg, fading=fading, seed=5))
        env_f.reset()
        env_f.fork_from(env_u, np.arange(n, dtype=np.int32))
        U.share_from(P, 0)
        F = mk(in_dev(P.to_shared, 0, n))
        assert all(same_learner(a, b) for a, b in zip(learners(U), learners(F)))
        for k in range(3):
            U.step_resident(env_u, count_rounds=True)
            F.step_resident(env_f, count_rounds=True)
            assert U.rounds_last == F.rounds_last, k
            env_u.step_resident()
            env_f.step_resident()
            ou, of = env_u.fetch(), env_f.fetch()
            assert all(_bits(ou[key]) == _bits(of[key]) for key in ('actions', 'obs', 'labels', 'violations')), k
            assert all(same_learner(a, b) for a, b in zip(learners(U), learners(F))), k
            same_control(U.control(), F.control(), what='step %d' % k)
        assert U.dictionary_sizes().tolist() == F.dictionary_sizes().tolist() and U.dictionary_sizes().sum() > 257 + 5
    finally:
        for h in made:
            h.close()


def test_round_trip_agents_shared_agents():
    """per-replica P -> kb_share -> kb_unshare -> P', against kb_fork(P) with the same indices: equal bytes, equal after three
    identical update_control calls, equal selections"""
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    P = new_agent(2, DIMS, N_PRBS, CAP, seed0=51)
    hs = [P]
    try:
        grow_ladder(P, 1, 'Y', 700)
        for s, m in enumerate([3, 0, 1, 2, 0, 0, 5]):
            grow_dict(P, 0, s, m, 800 + s)
        rng = np.random.default_rng(11)
        P.select_action(random_states(2, rng, DIMS))
        before, cP = [learners(P, e) for e in range(2)], P.control()
        S = in_dev(P.to_shared, 1, 3)            # ctl_index NULL: agent 1's control state for every replica
        hs.append(S)
        P2 = in_dev(S.to_agents, [0, 2, 1])
        hs.append(P2)
        sizes = np.tile(P.dictionary_sizes()[1], (3, 1))
        Tw = in_dev(VecKBRL, 3, DIMS, N_PRBS, capacity=CAP, gamma=1.0, pool_bytes=fork_pool_bytes(np.minimum(sizes + 128, CAP)))
        hs.append(Tw)
        Tw.fork_from(P, [1, 1, 1])
        assert (P2.dictionary_sizes() == sizes).all()
        for j in range(3):
            for s in range(len(DIMS)):
                assert same_learner(P2.learner(j, s, with_kinv=True), Tw.learner(j, s, with_kinv=True)), (j, s)
        same_control(P2.control(), Tw.control())
        same_control(P2.control(), cP, [1, 1, 1])
        # the source is as it was
        assert all(same_learner(a, b) for e in range(2) for a, b in zip(learners(P, e), before[e]))
        for k in range(3):
            st, ac, lb = control_batch(3, rng)
            assert _bits(P2.update_control(st, ac, lb)) == _bits(Tw.update_control(st, ac, lb)), k
        assert P2.dictionary_sizes().sum() > sizes.sum(), 'the steps learned something'
        assert (P2.dictionary_sizes() == Tw.dictionary_sizes()).all()
        for j in range(3):
            for s in range(len(DIMS)):
                assert same_learner(P2.learner(j, s, with_kinv=True), Tw.learner(j, s, with_kinv=True)), (j, s)
        select_same(P2, Tw, random_states(3, rng, DIMS), 'after learning')
        select_same(P2, Tw, np.full((3, sum(DIMS)), 60.0, dtype=np.float32), 'all underflow')
    finally:
        for h in hs:
            h.close()


# ------------------------------------------------------------------ 4. continuation against the oracle
TOL = 1e-9
N_BEFORE, N_AFTER = 600, 200


def lock_step(ag, orc, xs, ys, lo, hi, sizes, exempt):
    """samples lo .. hi - 1 through predict / update on the device handle and on the oracle, held to the tolerances of the G17
    case of tests/test_gpu_kbrl.py: f 1e-8 relative (1e-9 absolute), the predicted sign wherever |f| > 1e-7, every branch and
    every size, delta 1e-6"""
    for i in range(lo, hi):
        yp, f = ag.predict(0, 0, xs[i])
        yo, fo = orc.predict(0, xs[i])
        assert f == pytest.approx(fo, rel=1e-8, abs=TOL), i
        if abs(fo) > 1e-7:
            assert yp == yo, i
        else:
            exempt.append(i)
        br, dl = ag.update(0, 0, xs[i], int(ys[i]))
        bo, do = orc.update(0, xs[i], int(ys[i]))
        assert br == bo, (i, dl, do)
        if br:
            assert dl == pytest.approx(do, rel=1e-6, abs=1e-9), i
        assert sizes() == orc.m(0), i


def end_state(ag, orc):
    L = ag.learner(0, 0)
    assert L['m'] == orc.m(0)
    np.testing.assert_array_equal(L['landmarks'], orc.landmarks(0))
    np.testing.assert_allclose(L['coeff'], orc.coeff(0), rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('direction', ['unshare', 'share'])
def test_continuation_against_the_oracle(golden_dir, direction):
    """The first 600 samples of the G14 sequence go through one kind of handle in lock-step with the oracle, the dictionary
    crosses the bridge, and the other kind goes on with the oracle for 200 more -- no bit-for-bit claim across the storages (the
    triangle forms d* in another summation order), the project's own tolerances against the oracle instead.  Window: samples
    600 .. 799 (97 landmarks at the crossing, 127 at the end; 6 projections and 30 insertions in the window).  The oracle
    alone over that window on the CPU: 0 of the 200 samples have |f| <= 1e-7 (0 %), inside the cap of 1 % that may fall under
    the sign exemption -- asserted below as well."""
    from oracle import pyoracle as po
    from ranslice.kbrl_dev import SharedVecKBRL, VecKBRL
    g = np.load(os.path.join(golden_dir, 'g14_projectron_long.npz'))
    xs, ys = g['x'], g['y']
    orc = po.OracleKBRL([10], 200, [10], [3], capacity=1024)
    first = SharedVecKBRL(1, [10], 200, capacity=1024) if direction == 'unshare' else VecKBRL(1, [10], 200, capacity=1024)
    second = None
    try:
        first.reset([[10]], [[3]])
        exempt = []
        lock_step(first, orc, xs, ys, 0, N_BEFORE, lambda: int(first.dictionary_sizes().ravel()[0]), exempt)
        second = first.to_agents([0]) if direction == 'unshare' else first.to_shared(0, 1)
        assert bool(second.cfg.shared_dictionary) == (direction == 'share')
        end_state(second, orc)
        exempt = []
        lock_step(second, orc, xs, ys, N_BEFORE, N_BEFORE + N_AFTER, lambda: int(second.dictionary_sizes().ravel()[0]), exempt)
        assert len(exempt) <= N_AFTER // 100, exempt
        end_state(second, orc)
        assert orc.m(0) == 127
    finally:
        first.close()
        if second is not None:
            second.close()


# ------------------------------------------------------------------ 5. refusals and overflow
SMALL_DIMS = [3, 3]
SHELL0_TRI = (30 * 64 + 4096 + 128) * 8     # bytes of shell 0 of a per-replica dictionary
SHELL0_FULL = (30 * 64 + 4096) * 8          # ... of a shared one


class Small:
    """a shared handle (3 replicas) and a per-replica one (2 agents) with a dictionary beyond one shell each"""

    def __init__(self):
        self.X = new_agent(3, SMALL_DIMS, N_PRBS, 128, seed0=61, shared=True)
        self.P = new_agent(2, SMALL_DIMS, N_PRBS, 128, seed0=71)
        grow_dict(self.X, 0, 0, 70, 900)
        grow_dict(self.X, 0, 1, 5, 901)
        grow_dict(self.P, 1, 0, 66, 902)
        grow_dict(self.P, 1, 1, 4, 903)
        rng = np.random.default_rng(12)
        self.X.select_action(random_states(3, rng, SMALL_DIMS))
        self.P.select_action(random_states(2, rng, SMALL_DIMS))

    def agents(self, n, capacity=128, pool_bytes=0, n_prbs=N_PRBS, reset=False):
        from ranslice.kbrl_dev import VecKBRL
        ag = in_dev(VecKBRL, n, SMALL_DIMS, n_prbs, capacity=capacity, gamma=1.0, pool_bytes=pool_bytes)
        if reset:
            ag.reset(np.zeros((n, 2), dtype=np.int32), np.ones((n, 2), dtype=np.int32))
        return ag

    def shared(self, n, capacity=128, pool_bytes=0, reset=False):
        from ranslice.kbrl_dev import SharedVecKBRL
        sh = in_dev(SharedVecKBRL, n, SMALL_DIMS, N_PRBS, capacity=capacity, gamma=1.0, pool_bytes=pool_bytes)
        if reset:
            sh.reset(np.zeros((n, 2), dtype=np.int32), np.ones((n, 2), dtype=np.int32))
        return sh

    def close(self):
        self.X.close()
        self.P.close()


@pytest.fixture(scope='module')
def small():
    w = Small()
    yield w
    w.close()


def snapshot(h):
    n = 1 if h.cfg.shared_dictionary else h.n_envs
    return [learners(h, e) for e in range(n)], h.control(), flags(h)


def unchanged(h, snap):
    ls, c, f = snapshot(h)
    assert all(same_learner(a, b) for la, lb in zip(ls, snap[0]) for a, b in zip(la, lb))
    same_control(c, snap[1])
    assert _bits(f) == _bits(snap[2])


def test_unshare_refusals(small):
    X, P, L = small.X, small.P, small.X.L
    snapX, snapP = snapshot(X), snapshot(P)
    _, i2 = idx([0, 2])
    made = []

    def mk(h):
        made.append(h)
        return h
    try:
        dst = mk(small.agents(2))
        rc, msg = call(L, 'kb_unshare', dst, P, i2)
        assert rc == RS_EINVAL and 'source is not a shared-dictionary handle' in msg
        rc, msg = call(L, 'kb_unshare', mk(small.shared(2)), X, i2)
        assert rc == RS_EINVAL and 'destination is a shared-dictionary handle' in msg
        rc, msg = call(L, 'kb_unshare', mk(small.agents(2, n_prbs=N_PRBS + 1)), X, i2)
        assert rc == RS_EINVAL and 'configurations differ' in msg
        for bad in ([0, 3], [-1, 0]):
            rc, msg = call(L, 'kb_unshare', dst, X, idx(bad)[1])
            assert rc == RS_EINVAL and 'out of range' in msg and str(bad[0] if bad[0] < 0 else bad[1]) in msg
        rc, msg = call(L, 'kb_unshare', dst, mk(small.shared(3)), i2)
        assert rc == RS_ESTATE and 'never reset' in msg
        frozen = mk(P.deploy([0, 1]))
        rc, msg = call(L, 'kb_unshare', frozen, X, i2)
        assert rc == RS_ESTATE and 'inference-only' in msg
        byref = mk(P.deploy([0, 1], by_reference=True))
        rc, msg = call(L, 'kb_unshare', byref, X, i2)
        assert rc == RS_ESTATE and 'by-reference' in msg
        assert dst.L.kb_unshare(dst.h, dst.h, i2) == RS_EINVAL
        # nothing above touched the destination: it was never reset, and still is not
        st = np.zeros((2, 6), dtype=np.float32)
        with pytest.raises(_lib.RanSliceError, match='kb_reset'):
            dst.select_action(st)
        unchanged(X, snapX)
        unchanged(P, snapP)
    finally:
        for h in made:
            h.close()


def test_unshare_refuses_inside_a_round_and_works_after_the_commit(small):
    """between kb_shared_scan and kb_shared_commit of a round the dictionaries are between two states of a step"""
    X = clone_shared(small.X)
    dst = small.agents(2)
    try:
        L = X.L
        rng = np.random.default_rng(13)
        st, ac, lb = control_batch(3, rng, SMALL_DIMS)
        hits, counts, props = np.zeros((3, 2), dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros((2, X.budget, 18))
        fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
        assert L.kb_shared_scan(X.h, st.ctypes.data_as(fp), ac.ctypes.data_as(ip), lb.ctypes.data_as(ip), 0, X.budget, hits.ctypes.data_as(ip),
                                counts.ctypes.data_as(ip), props.ctypes.data_as(dp)) == 0
        assert counts.sum() > 0, 'the scan found no mistake: choose another seed'
        rc, msg = call(L, 'kb_unshare', dst, X, idx([0, 2])[1])
        assert rc == RS_ESTATE and 'kb_shared_scan' in msg and 'kb_shared_commit' in msg
        taken = np.minimum(counts, X.budget).astype(np.int32)
        assert L.kb_shared_apply(X.h, taken.ctypes.data_as(ip), props.ctypes.data_as(dp), X.budget) == 0
        rc, msg = call(L, 'kb_unshare', dst, X, idx([0, 2])[1])
        assert rc == RS_ESTATE
        assert L.kb_shared_commit(X.h, taken.ctypes.data_as(ip)) == 0
        rc, msg = call(L, 'kb_unshare', dst, X, idx([0, 2])[1])
        assert rc == 0, msg
        want = learners(X)
        assert all(same_learner(dst.learner(j, s, with_kinv=True), want[s]) for j in range(2) for s in range(2))
        # and the same guard on a shared DESTINATION
        rng = np.random.default_rng(14)
        st, ac, lb = control_batch(3, rng, SMALL_DIMS)
        assert L.kb_shared_scan(X.h, st.ctypes.data_as(fp), ac.ctypes.data_as(ip), lb.ctypes.data_as(ip), 0, X.budget, hits.ctypes.data_as(ip),
                                counts.ctypes.data_as(ip), props.ctypes.data_as(dp)) == 0
        assert counts.sum() > 0
        rc, msg = call(L, 'kb_share', X, small.P, 1, None)
        assert rc == RS_ESTATE and 'kb_shared_commit' in msg
    finally:
        X.close()
        dst.close()


def test_unshare_overflow_leaves_the_destination_reset_and_empty(small):
    X = small.X
    snapX = snapshot(X)
    cX = X.control()
    index = [2, 0]
    for what, kw, word in (('pool', dict(pool_bytes=64 * 8 + 4 * SHELL0_TRI), 'bytes of pool'), ('capacity', dict(capacity=64), 'capacity')):
        dst = small.agents(2, **kw)
        try:
            rc, msg = call(X.L, 'kb_unshare', dst, X, idx(index)[1])
            assert rc == RS_EOVERFLOW and word in msg and 'empty dictionaries' in msg, (what, rc, msg)
            assert (dst.dictionary_sizes() == 0).all() and dst.pool()['used_bytes'] == 64 * 8, what
            same_control(dst.control(), cX, index, what)
            dst.select_action(np.zeros((2, 6), dtype=np.float32))      # reset: it selects (and would learn from scratch)
            dst.update_control(*control_batch(2, np.random.default_rng(15), SMALL_DIMS))
        finally:
            dst.close()
    unchanged(X, snapX)


def test_share_refusals_and_overflow(small):
    X, P, L = small.X, small.P, small.X.L
    snapX, snapP = snapshot(X), snapshot(P)
    made = []

    def mk(h):
        made.append(h)
        return h
    try:
        dst = mk(small.shared(3, reset=True))
        blob = _bits(dst.save_state())
        rc, msg = call(L, 'kb_share', dst, X, 0, None)
        assert rc == RS_EINVAL and 'source is a shared-dictionary handle' in msg
        rc, msg = call(L, 'kb_share', mk(small.agents(3)), P, 0, None)
        assert rc == RS_EINVAL and 'destination is not a shared-dictionary handle' in msg
        for agent in (-1, 2):
            rc, msg = call(L, 'kb_share', dst, P, agent, None)
            assert rc == RS_EINVAL and 'dict_agent' in msg
        rc, msg = call(L, 'kb_share', dst, P, 1, idx([0, 1, 2])[1])
        assert rc == RS_EINVAL and 'out of range' in msg
        rc, msg = call(L, 'kb_share', dst, mk(small.agents(2)), 1, None)
        assert rc == RS_ESTATE and 'never reset' in msg
        rc, msg = call(L, 'kb_share', dst, mk(P.deploy([0, 1])), 1, None)
        assert rc == RS_ESTATE and 'inference-only' in msg and 'kb_fork_rebuild' in msg
        rc, msg = call(L, 'kb_share', dst, mk(P.deploy([0, 1], by_reference=True)), 1, None)
        assert rc == RS_ESTATE and 'by-reference' in msg
        assert _bits(dst.save_state()) == blob, 'a refusal touched the destination'
        # a handle of smaller capacity: refused without touching it
        low = mk(small.shared(3, capacity=64, reset=True))
        blob = _bits(low.save_state())
        rc, msg = call(L, 'kb_share', low, P, 1, None)
        assert rc == RS_EINVAL and 'configurations differ' in msg and _bits(low.save_state()) == blob
        # a pool that holds shell 0 of both dictionaries and nothing more: agent 1's 66 landmarks do not fit
        tight = mk(small.shared(3, pool_bytes=64 * 8 + 2 * SHELL0_FULL))
        rc, msg = call(L, 'kb_share', tight, P, 1, idx([1, 0, 1])[1])
        assert rc == RS_EOVERFLOW and 'bytes of pool' in msg and 'empty dictionaries' in msg
        assert (tight.dictionary_sizes() == 0).all() and tight.pool()['used_bytes'] == 64 * 8
        same_control(tight.control(), snapP[1], [1, 0, 1])
        tight.select_action(np.zeros((3, 6), dtype=np.float32))
        tight.update_control(*control_batch(3, np.random.default_rng(16), SMALL_DIMS))
        # ... and agent 0's (empty) dictionaries do
        rc, msg = call(L, 'kb_share', tight, P, 0, None)
        assert rc == 0, msg
        assert (tight.dictionary_sizes() == 0).all()
        unchanged(X, snapX)
        unchanged(P, snapP)
    finally:
        for h in made:
            h.close()


# ------------------------------------------------------------------ 6. downstream
def test_per_replica_tools_work_behind_the_bridge(world):
    """what the bridge exists for: to_agents(...) first, then deployment (by reference = the copy), export / import, pruning"""
    from ranslice.kbrl_dev import VecKBRL
    X, _ = world.get('X')
    for name in ('deploy', 'export_agents', 'prune', 'set_learning'):      # the refusals on the shared handle itself stay
        with pytest.raises(_lib.RanSliceError):
            getattr(X, name)(*{'deploy': ([0],), 'export_agents': ([0],), 'prune': (64,), 'set_learning': (False,)}[name])
    A = in_dev(X.to_agents, [0])
    made = [A]
    try:
        R, Cp = A.deploy([0] * 33, by_reference=True), A.deploy([0] * 33)
        made += [R, Cp]
        rng = np.random.default_rng(17)
        for k in range(2):
            st = random_states(33, rng, DIMS)
            aR, jR = R.select_action(st)
            aC, jC = Cp.select_action(st)
            assert _bits(aR) == _bits(aC) and _bits(jR) == _bits(jC), k
        blob = A.export_agents([0])
        B = in_dev(VecKBRL.load_agents, blob)
        made.append(B)
        assert B.export_agents([0]) == blob
        want = learners(X, kinv=False)
        assert all(same_learner(B.learner(0, s), want[s], kinv=False) for s in range(len(DIMS)))
        removed = A.prune(64)
        assert removed == sum(max(m - 64, 0) for m in LADDER_X)
        assert A.dictionary_sizes()[0].tolist() == [min(m, 64) for m in LADDER_X]
        A.select_action(random_states(1, rng, DIMS))
    finally:
        for h in made:
            h.close()
