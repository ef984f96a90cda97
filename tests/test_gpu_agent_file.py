"""Agent files on the device: kb_export_agents / kb_import_agents against the TWIN -- kb_deploy with the same src_index, whose
scores tests/test_gpu_scoring.py holds to tests/scoring_mirror.py bit for bit -- and reference-trained agents packed on the
host (ranslice.agent_file) against tests/agent_restatement.py, which tests/test_agent_file.py holds to what the reference
recorded.  Comparisons with the twin are bit for bit (a zero of either sign counts as zero).

Dictionaries are grown teacher-forced on the device through kb_predict / kb_update; the test build is used wherever scores,
rows or chains are read (kb_dev_get_scores / kb_dev_get_rows / kb_dev_get_chains, csrc/kb_probe.hip)."""
import ctypes as C
import os

import numpy as np
import pytest

import agent_restatement as ar
from ranslice import _lib, agent_file as af
from test_gpu_deploy_ref import _bits, grow, new_agent, random_states, rows, scores
from test_gpu_scoring import _p, values_equal

pytestmark = pytest.mark.gpu

DIMS = [10, 3]
SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 319, 320, 321, 513]   # agent a: SIZES[a] landmarks of dims 10, SIZES[11 - a] of dims 3
OFFGRID, F32BAD = 6, 7            # the agents whose dims-10 dictionary holds 49 off-grid landmarks / a non-float32 coordinate
N_PRBS = 200


def load(blob, index=None, by_reference=False):
    """VecKBRL.load_agents on the test build (the handles that meet in one comparison come from the same library)"""
    from ranslice.kbrl_dev import VecKBRL
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv('RANSLICE_DEV_BUILD', '1')
        ag = VecKBRL.load_agents(blob, index, by_reference=by_reference)
    return ag


def chains(ag, e, s, cap):
    ag.L.kb_dev_get_chains.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32] + [C.POINTER(C.c_int32)] * 4
    ag.L.kb_dev_get_chains.restype = C.c_int
    head, link, off, m = np.zeros(256, dtype=np.int32), np.zeros(cap, dtype=np.int32), C.c_int32(-1), C.c_int32(-1)
    rc = ag.L.kb_dev_get_chains(ag.h, e, s, cap, C.byref(m), _p(head, C.c_int32), _p(link, C.c_int32), C.byref(off))
    assert rc == 0, rc
    return dict(m=m.value, head=head, link=link[:m.value], offgrid=off.value)


def same_selection(X, Y, states, what=''):
    """one selection on both handles: everything the contract names is equal"""
    n = X.n_prbs
    aX, jX = X.select_action(states)
    aY, jY = Y.select_action(states)
    FX, fdX = scores(X)
    FY, fdY = scores(Y)
    ok = values_equal(FX[:, :n + 1], FY[:, :n + 1])
    assert ok.all(), (what, 'F differs for tasks', np.nonzero(~ok.all(axis=1))[0][:8])
    assert (fdX == fdY).all(), (what, 'fdirect', np.nonzero(fdX != fdY)[0][:8])
    assert _bits(aX) == _bits(aY) and _bits(jX) == _bits(jY), (what, 'actions', np.nonzero((aX != aY).any(axis=1))[0][:8])
    cX, cY = X.control(), Y.control()
    for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
        assert _bits(cX[key]) == _bits(cY[key]), (what, key)
    assert X.stats() == Y.stats(), (what, X.stats(), Y.stats())
    return aX, FX, fdX


def same_agents(X, Y, what=''):
    """dictionaries, control state, flags and pool through the public getters"""
    assert (X.dictionary_sizes() == Y.dictionary_sizes()).all(), what
    for j in range(X.n_envs):
        for s in range(X.S):
            a, b = X.learner(j, s), Y.learner(j, s)
            assert a['m'] == b['m'] and _bits(a['landmarks']) == _bits(b['landmarks']) and _bits(a['coeff']) == _bits(b['coeff']), (what, j, s)
    cX, cY = X.control(), Y.control()
    for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
        assert _bits(cX[key]) == _bits(cY[key]), (what, key)
    assert X.flagged_replicas() == Y.flagged_replicas() and X.pool() == Y.pool(), what


class Ladder:
    def __init__(self):
        n = len(SIZES)
        self.src = new_agent(n, DIMS, N_PRBS, capacity=640)
        for a in range(n):
            grow(self.src, a, 0, SIZES[a], 300 + 2 * a, off_grid=range(3, 52) if a == OFFGRID else (), f32=a != F32BAD)
            grow(self.src, a, 1, SIZES[n - 1 - a], 301 + 2 * a)
        self.sizes = self.src.dictionary_sizes()
        assert self.sizes[:, 0].tolist() == SIZES and self.sizes[:, 1].tolist() == SIZES[::-1]
        rng = np.random.default_rng(3)
        self.src.select_action(random_states(n, rng))      # (margins, actions, tie counters and statistics away from their reset values)
        self.index = np.concatenate([rng.permutation(n), [3, 3, 11]]).astype(np.int32)   # a permutation and repeats
        self.blob = self.src.export_agents(self.index)
        self.lm_single = self.src.learner(1, 0)['landmarks'][0, :10], self.src.learner(n - 2, 1)['landmarks'][0, :3]

    def states(self, seed, index=None):
        """a random state per agent; the agents of the single-landmark dictionaries stand near their landmark (one landmark is
        scored in float32: further away its kernel value is below the float32 range)"""
        index = self.index if index is None else index
        rng = np.random.default_rng(seed)
        st = random_states(len(index), rng)
        for j, a in enumerate(index):
            if a == 1:
                st[j, :10] = (self.lm_single[0] + rng.uniform(0.05, 0.2, 10)).astype(np.float32)
            if a == len(SIZES) - 2:
                st[j, 10:] = (self.lm_single[1] + rng.uniform(0.1, 0.4, 3)).astype(np.float32)
        return st

    def close(self):
        self.src.close()


@pytest.fixture(scope='module')
def ladder():
    ld = Ladder()
    yield ld
    ld.close()


# ------------------------------------------------------------------ 1. the twin
def test_import_is_the_deploy_twin(ladder):
    """A = kb_deploy(src, idx), B = kb_import_agents(kb_export_agents(src, idx)): dictionaries of 0 .. 513 landmarks, dims 10 and
    3, 49 landmarks off the grid, a non-float32 coordinate, n_prbs 200.  Getters, three selections (the third in the state
    where everything underflows and every candidate is a tie to be drawn), grid-index rows, links, heads, off-grid counts"""
    from ranslice.kbrl_dev import deploy_pool_bytes
    A, B = ladder.src.deploy(ladder.index), load(ladder.blob)
    try:
        assert B.frozen and not B.by_reference and B.n_envs == len(ladder.index) and B.dims == DIMS and B.n_prbs == N_PRBS
        same_agents(A, B, 'after the import')
        assert B.pool()['used_bytes'] == B.pool()['total_bytes'] == deploy_pool_bytes(ladder.sizes[ladder.index]) == af.info(ladder.blob)['pool_bytes']
        assert B.stats() == [0, 0, 0, 0]
        for k, seed in enumerate((4, 5)):
            _, F, fd = same_selection(A, B, ladder.states(seed), 'selection %d' % k)
            assert F[:, :N_PRBS + 1].any(axis=1).sum() > len(ladder.index)
        off = [j for j, a in enumerate(ladder.index) if a == OFFGRID]
        assert all(fd[2 * j] == (3 | (49 << 8)) for j in off), 'the off-grid landmarks take the direct evaluation'
        far = np.full((len(ladder.index), 13), 60.0, dtype=np.float32)
        stats0 = B.stats()
        _, F, fd = same_selection(A, B, far, 'all underflow')
        assert not F[:, :N_PRBS + 1].any() and B.stats()[0] > stats0[0]
        same_selection(A, B, ladder.states(6), 'the selection that follows the draws')
        same_agents(A, B, 'after the selections')
        for j, a in enumerate(ladder.index):
            for s in range(2):
                ra, rb = rows(A, j, s, 640), rows(B, j, s, 640)
                assert ra['m'] == rb['m'] and _bits(ra['idx']) == _bits(rb['idx']) and _bits(ra['lam']) == _bits(rb['lam']), (j, s)
                ca, cb = chains(A, j, s, 640), chains(B, j, s, 640)
                assert ca['m'] == cb['m'] and ca['offgrid'] == cb['offgrid'] == (49 if (a == OFFGRID and s == 0) else 0), (j, s)
                assert _bits(ca['head']) == _bits(cb['head']) and _bits(ca['link']) == _bits(cb['link']), (j, s)
    finally:
        A.close()
        B.close()


def test_twin_at_17_prbs():
    """the candidate grid of 17 PRBs (one tile and a bit, one group), dictionaries of 2, 65 and 130 landmarks"""
    src = new_agent(2, DIMS, 17, capacity=192)
    try:
        for t, m in enumerate([2, 65, 130, 65]):
            grow(src, t // 2, t % 2, m, 900 + t)
        index = np.array([1, 0, 1], dtype=np.int32)
        A, B = src.deploy(index), load(src.export_agents(index))
        same_agents(A, B)
        rng = np.random.default_rng(17)
        for k in range(2):
            _, F, _ = same_selection(A, B, random_states(3, rng), 'selection %d' % k)
        assert F[:, :18].any()
        A.close()
        B.close()
    finally:
        src.close()


# ------------------------------------------------------------------ 2. closed loop
@pytest.fixture(scope='module')
def trained(golden_dir):
    from test_gpu_agent_fork import Source
    s = Source(golden_dir, 2, grow=1500, tail=False)
    yield s
    s.close()


@pytest.mark.parametrize('graph', [False, True])
def test_closed_loop(trained, graph):
    """trained agents (one past 320 landmarks, with off-grid and non-float32 landmarks) deployed and imported, on fresh
    environments with the same seeds: 60 steps of run_resident, plain and as a replayed hipGraph -- identical histories"""
    from ranslice.kbrl_dev import VecKBRL
    from test_gpu_agent_fork import BIG, KEYS
    src = trained
    rng = np.random.default_rng(41)
    index = rng.permutation(np.concatenate([[BIG[0], 5, 20], rng.choice([BIG[0], 5, 20, 33], 21)])).astype(np.int32)
    steps = 60
    got = []
    for imported in (True, False):
        ag = VecKBRL.load_agents(src.agent.export_agents(index)) if imported else src.agent.deploy(index)
        env = src.new_env(len(index), seed=92)
        env.reset()
        env.step(ag.control()['action'])
        ag.history_begin(steps)
        ag.run_resident(env, steps, graph=graph)
        got.append((ag.history_fetch(), env.fetch(), ag.control(), ag.stats()))
        ag.close()
        env.close()
    (hb, fb, cb, sb), (ha, fa, ca, sa) = got
    assert hb['recorded'] == ha['recorded'] == steps
    for key in KEYS:
        assert _bits(hb[key]) == _bits(ha[key]), key
    for key in ('reward', 'obs', 'labels', 'violations', 'actions'):
        assert _bits(fb[key]) == _bits(fa[key]), key
    for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
        assert _bits(cb[key]) == _bits(ca[key]), key
    assert sb == sa and sb[0] > 0 and hb['resources'].any()


# ------------------------------------------------------------------ 3. fan-out from a file
def test_fan_out_from_a_file(ladder):
    """agents of the file named 1, 16 and 17 times: by reference from the import, by reference and by copy from the deploy
    twin, and VecKBRL.load_agents(blob, index, by_reference=True) -- the same on the same states; the store holds the three
    distinct agents once"""
    from ranslice.kbrl_dev import deploy_ref_pool_bytes
    A, B = ladder.src.deploy(ladder.index), load(ladder.blob)
    names = [int(np.nonzero(ladder.index == a)[0][0]) for a in (5, 9, 11)]     # agents of the file: 65 / 2, 320 / 2, 513 / 0 landmarks
    idx2 = np.random.default_rng(8).permutation(np.repeat(names, [1, 16, 17])).astype(np.int32)
    hs = [A, B]
    try:
        RB, RA, CA = B.deploy(idx2, by_reference=True), A.deploy(idx2, by_reference=True), A.deploy(idx2)
        RL = load(ladder.blob, idx2, by_reference=True)
        hs += [RB, RA, CA, RL]
        want = deploy_ref_pool_bytes(ladder.sizes[ladder.index], idx2)
        for R in (RB, RA, RL):
            assert R.frozen and R.by_reference and R.pool()['used_bytes'] == R.pool()['total_bytes'] == want
        for seed in (9, 10):
            st = ladder.states(seed, ladder.index[idx2])
            same_selection(RB, CA, st, 'by reference from the import')
            aC = CA.control()
            FC, fdC = scores(CA)
            for X, what in ((RA, 'by reference from the deploy twin'), (RL, 'load_agents')):
                X.select_action(st)
                FX, fdX = scores(X)
                assert values_equal(FX[:, :N_PRBS + 1], FC[:, :N_PRBS + 1]).all() and (fdX == fdC).all(), what
                cX = X.control()
                for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
                    assert _bits(cX[key]) == _bits(aC[key]), (what, key)
                assert X.stats() == CA.stats(), what
    finally:
        for h in hs:
            h.close()


# ------------------------------------------------------------------ 4. determinism and idempotence
def test_exports_are_deterministic_and_idempotent(ladder):
    """two exports are byte-identical; the export from the copy-deployed twin, and from the imported handle, is the blob; the
    host packer writes the device's bytes"""
    A, B = ladder.src.deploy(ladder.index), load(ladder.blob)
    try:
        ident = np.arange(len(ladder.index), dtype=np.int32)
        assert ladder.src.export_agents(ladder.index) == ladder.blob
        assert A.export_agents(ident) == ladder.blob, 'from the copy-deployed handle'
        assert B.export_agents(ident) == ladder.blob, 'from the handle the blob built'
        u = af.unpack(ladder.blob)
        assert af.pack(u) == ladder.blob
        assert (u['m'] == ladder.sizes[ladder.index]).all() and af.info(ladder.blob)['n_agents'] == len(ladder.index)
        j = int(np.nonzero(ladder.index == F32BAD)[0][0])
        assert u['agents'][j]['f32bad'].tolist() == [1, 0] and sum(int(a['f32bad'].sum()) for a in u['agents']) == 1
        sub = np.array([2, 0, 2], dtype=np.int32)
        assert af.pack(u['config'], [u['agents'][k] for k in sub]) == B.export_agents(sub)
    finally:
        A.close()
        B.close()


# ------------------------------------------------------------------ 5. reference-trained agents
@pytest.mark.parametrize('name', ar.FIXTURES)
def test_reference_trained_agents_select_as_the_reference(golden_dir, name):
    """the reference's final dictionaries and last control state, packed on the host and imported: select_action(final_state)
    gives the recorded last action, adjusted flag and margins exactly; on the last 64 recorded states every (state, slice)
    decision equals the restatement's wherever its smallest scanned |f| is at least 10 tolerances (at most 1 % of the pairs
    may be left out: measured 1 of 320 for g10_kbrl_s0, none for the others), and F is within 1e-9 (1 + sum |k c|) of it"""
    fx = ar.Fixture(golden_dir, name)
    blob = af.pack(fx.config(), [fx.agent()])
    one = load(blob)
    many = load(blob, np.zeros(64, dtype=np.int32))
    try:
        act, adj = one.select_action(fx.final_state[None, :])
        c = one.control()
        assert (act[0] == fx.action).all() and int(adj[0]) == fx.adjusted and (c['margins'][0] == fx.margins).all()
        st = fx.state[-64:]
        many.select_action(st)
        c = many.control()
        found = c['action'] - c['margins']          # the candidate each learner stopped at: invariant under the adjustment
        F, _ = scores(many)
        F = F.reshape(64, fx.S, 256)
        out = 0
        for i in range(64):
            r = ar.select_action(fx, st[i])
            err = np.abs(F[i, :, :fx.n_prbs + 1].astype(np.longdouble) - r['f'])
            assert (err <= r['tol']).all(), (i, float((err / r['tol']).max()))
            sure = r['ratio'] >= 10.0
            out += int((~sure).sum())
            assert (found[i][sure] == r['found'][sure]).all(), (i, found[i], r['found'])
        print('%s: %d of %d (state, slice) pairs left out' % (name, out, 64 * fx.S))
        assert out <= 0.01 * 64 * fx.S
    finally:
        one.close()
        many.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals(ladder):
    from ranslice.kbrl_dev import VecKBRL
    src, n = ladder.src, len(SIZES)
    R = src.deploy(np.array([0, 1], dtype=np.int32), by_reference=True)
    shared = new_agent(2, DIMS, N_PRBS, capacity=640, shared=True)
    full = new_agent(2, DIMS, N_PRBS, capacity=640)
    B = load(ladder.blob)
    try:
        with pytest.raises(_lib.RanSliceError) as e:
            R.export_agents([0])
        assert e.value.code == _lib.RS_ESTATE and 'kb_export' in str(e.value)
        for call in (lambda: shared.export_agents([0]), lambda: src.export_agents([0, n]), lambda: src.export_agents([-1])):
            with pytest.raises(_lib.RanSliceError) as e:
                call()
            assert e.value.code == _lib.RS_EINVAL
        # a blob of another size than kb_export_bytes': refused, untouched
        idx = np.array([5, 2], dtype=np.int32)
        ip = idx.ctypes.data_as(C.POINTER(C.c_int32))
        nb = C.c_uint64()
        assert src.L.kb_export_bytes(src.h, ip, 2, C.byref(nb)) == 0
        for size in (nb.value - 8, nb.value + 8):
            buf = np.full(nb.value + 8, 0xA5, dtype=np.uint8)
            assert src.L.kb_export_agents(src.h, ip, 2, buf.ctypes.data_as(C.c_void_p), size) == _lib.RS_EINVAL
            assert (buf == 0xA5).all()
        # a coefficient that is not a number, with a hash that is right: refused by the device's check, *out stays NULL
        u = af.unpack(ladder.blob)
        j = int(np.nonzero(ladder.index == 9)[0][0])
        u['agents'][j]['coeff'][0][300] = np.nan
        bad = np.frombuffer(af.pack(u), dtype=np.uint8)
        assert af.info(bad.tobytes())['n_agents'] == len(ladder.index)
        h = C.c_void_p(12345)
        assert B.L.kb_import_agents(bad.ctypes.data_as(C.c_void_p), bad.size, 0, C.byref(h)) == _lib.RS_EINVAL
        assert h.value is None and b'finite' in B.L.kb_last_error(None)
        with pytest.raises(_lib.RanSliceError) as e:
            VecKBRL.load_agents(ladder.blob[:-8])
        assert e.value.code == _lib.RS_EINVAL
        # the imported handle refuses what a kb_deploy handle refuses
        st = ladder.states(50)
        zero = np.zeros((B.n_envs, 2), dtype=np.int32)
        estate = dict(update_control=lambda: B.update_control(st, zero, zero + 1), set_learning=lambda: B.set_learning(True),
                      save_state=lambda: B.save_state(), kb_reset=lambda: B.reset(zero, zero),
                      kb_fork=lambda: full.fork_from(B, np.array([0, 1], dtype=np.int32)), kb_update=lambda: B.update(0, 0, np.zeros(11), 1),
                      get_learner=lambda: B.learner(int(np.nonzero(ladder.index == n - 1)[0][0]), 0, with_kinv=True))
        for name, call in estate.items():
            with pytest.raises(_lib.RanSliceError) as e:
                call()
            assert e.value.code == _lib.RS_ESTATE, name
    finally:
        for h in (R, shared, full, B):
            h.close()


def test_source_continues_untouched(trained):
    """a source exported from goes on exactly as a twin of itself that was not: ten closed-loop steps of learning, then states,
    control state and dictionaries are equal"""
    from test_gpu_agent_fork import N
    src = trained
    index = np.arange(N, dtype=np.int32)
    pairs = [src.fork_pair(index) for _ in range(2)]
    try:
        blob = pairs[0][0].export_agents(np.array([3, 3, 40, 7], dtype=np.int32))
        assert af.info(blob)['n_agents'] == 4
        for ag, env in pairs:
            ag.run_resident(env, 10, graph=False)
        (a0, e0), (a1, e1) = pairs
        f0, f1 = e0.fetch(), e1.fetch()
        for key in ('reward', 'obs', 'labels', 'violations', 'actions'):
            assert _bits(f0[key]) == _bits(f1[key]), key
        c0, c1 = a0.control(), a1.control()
        for key in ('action', 'adjusted', 'margins', 'security_factors', 'accuracies'):
            assert _bits(c0[key]) == _bits(c1[key]), key
        assert (a0.dictionary_sizes() == a1.dictionary_sizes()).all() and a0.stats() == a1.stats()
        # (not the save_state blobs: where a dictionary's new shells lie in the pool is the allocator's order, not a result)
        for e in (3, 7, 40, 0, N - 1):
            for s in range(a0.S):
                x, y = a0.learner(e, s, with_kinv=True), a1.learner(e, s, with_kinv=True)
                assert x['m'] == y['m'] and all(_bits(x[k]) == _bits(y[k]) for k in ('landmarks', 'coeff', 'kinv')), (e, s)
        assert a0.stats()[1] > 0, 'the ten steps learned'
    finally:
        for ag, env in pairs:
            ag.close()
            env.close()


# ------------------------------------------------------------------ 7. experiments_trained at toy size
def test_experiments_trained_saves_and_loads_its_agents(golden_dir, tmp_path):
    """2 agents trained 40 steps, 4 replicas each, 20 evaluation steps: the evaluation of the agents loaded from their file
    equals the same-process one number for number"""
    import experiments_trained as et
    import scenario_creator as sc
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    old = sc._FADING
    sc.set_fading([g['t0'], g['t1'], g['t2']])
    try:
        kw = dict(runs=range(2), train_steps=40, eval_replicas=4, eval_steps=20, capacity=256, pool_bytes=64 << 20, verbose=False)
        a_range = [0.99, 0.999]
        s1 = et.train_and_deploy(0, a_range, out_dir=str(tmp_path / 'same'), save_agents=str(tmp_path / 'agents'), **kw)
        assert os.path.getsize(et.agents_path(str(tmp_path / 'agents'), 0, a_range)) > af.HEADER_BYTES
        s2 = et.train_and_deploy(0, a_range, out_dir=str(tmp_path / 'loaded'), load_agents=str(tmp_path / 'agents'), **kw)
        s3 = et.train_and_deploy(0, a_range, out_dir=str(tmp_path / 'by_ref'), load_agents=str(tmp_path / 'agents'), by_reference=True, **kw)
        assert s2['loaded'] and s2['deployed'] == s1['deployed'] == s3['deployed'] and s2['max_dictionary'] == s1['max_dictionary']
        assert s2['deployed_pool_bytes'] == s1['deployed_pool_bytes'] > s3['deployed_pool_bytes']
        for i in range(2):
            za, zb, zc = (np.load(os.path.join(s['path'], 'evaluation_%d.npz' % i)) for s in (s1, s2, s3))
            for key in ('violation', 'resources', 'reward'):
                assert za[key].shape == (4, 20) and _bits(za[key]) == _bits(zb[key]) == _bits(zc[key]), (i, key)
            assert za['resources'].any()
    finally:
        sc.set_fading(old)
