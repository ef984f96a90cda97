"""kb_fork / kb_deploy / kb_set_learning: trained KBRL agents gathered into other handles on the device, deployed without
Kinv, and the resident loop with learning switched off.  Every comparison is bit for bit: an agent's results do not depend on
its neighbours in the batch (tests/test_gpu_kbrl.py pins that), so a forked agent must continue exactly as its source does
whatever index array built the fork (repeats, a reversed range, a permutation).

Source: 64 agents trained closed-loop for 150 steps (scenario 0, and scenario 2 with its mMTC learners), one learner of which
is then grown past KB_BIG_M (320 landmarks) by the committed teacher-forced fixture g17_projectron_3000 through kb_predict /
kb_update -- a multi-shell dictionary; in scenario 2 (100 PRBs) half of the fixture's allocations are off the candidate grid,
and a few samples are nudged off the float32 lattice, so the offgrid / f32bad marks are set too."""
import os

import numpy as np
import pytest

from ranslice import _lib
from ranslice.config import make_config

pytestmark = pytest.mark.gpu

N = 64
BIG = (3, 0)     # the learner grown past KB_BIG_M
KEYS = ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation')


def _fading(golden_dir):
    g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
    return [g['t0'], g['t1'], g['t2']]


def _dims(scenario):
    cfg = make_config(scenario)
    return [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _index(rng):
    return np.concatenate([[5, 5, 5, 0, 63, 63, BIG[0], BIG[0]], np.arange(N - 1, -1, -1), rng.permutation(N)]).astype(np.int32)


class Source:
    """the trained pair, and what a host-driven continuation needs: the observation the pending action was chosen in (prev),
    that action, the labels of its step and the observation it led to"""

    def __init__(self, golden_dir, scenario, grow=1500, graph=False, tail=True):
        from ranslice.kbrl_dev import VecKBRL
        from ranslice.vec_env import VecRanSlice
        self.scenario, self.fading = scenario, _fading(golden_dir)
        self.dims, self.n_prbs = _dims(scenario)
        rng = np.random.default_rng(17 + scenario)
        ia = np.stack([[rng.integers(4, 20) if d == 10 else rng.integers(2, 10) for d in self.dims] for _ in range(N)]).astype(np.int32)
        sf = np.stack([[rng.integers(2, 8) if d == 10 else rng.integers(1, 4) for d in self.dims] for _ in range(N)]).astype(np.int32)
        self.env = VecRanSlice(n_envs=N, cfg=make_config(scenario, n_envs=N), fading=self.fading, seed=31)
        self.agent = VecKBRL(N, self.dims, self.n_prbs, capacity=1024, pool_bytes=256 << 20)
        self.env.reset()
        self.agent.reset(ia, sf, seeds=np.arange(N, dtype=np.uint64) + 2)
        self.env.step(ia)
        self.agent.run_resident(self.env, 149, graph=graph)
        if grow:
            g = np.load(os.path.join(golden_dir, 'g17_projectron_3000.npz'))
            xs = np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1)[:grow].copy()
            xs[::50, 0] += 1e-9     # not float32 values: the dictionary must fall back to its f64 coordinate rows (f32bad)
            for x, y in zip(xs, g['y'][:grow]):
                self.agent.predict(BIG[0], BIG[1], x)
                self.agent.update(BIG[0], BIG[1], x, int(y))
            assert self.agent.dictionary_sizes()[BIG] >= 320
        if not tail:
            return
        self.agent.step_resident(self.env)
        self.prev = self.env.fetch()['obs']
        self.env.step_resident()
        f = self.env.fetch()
        self.action, self.labels, self.obs = f['actions'], f['labels'], f['obs']

    def new_agent(self, n, pool_bytes=512 << 20, **kw):
        from ranslice.kbrl_dev import VecKBRL
        kw.setdefault('capacity', 1024)
        return VecKBRL(n, kw.pop('dims', self.dims), kw.pop('n_prbs', self.n_prbs), pool_bytes=pool_bytes, **kw)

    def new_env(self, n, seed=77):
        from ranslice.vec_env import VecRanSlice
        return VecRanSlice(n_envs=n, cfg=make_config(self.scenario, n_envs=n), fading=self.fading, seed=seed)

    def fork_pair(self, index):
        ag, env = self.new_agent(len(index)), self.new_env(len(index))
        ag.fork_from(self.agent, index)
        env.fork_from(self.env, index)
        return ag, env

    def close(self):
        self.env.close()
        self.agent.close()


@pytest.fixture(params=[0, 2])
def src(request, golden_dir):
    s = Source(golden_dir, request.param)
    yield s
    s.close()


def _learners(ag, agents, S, with_kinv=True):
    return {(e, s): ag.learner(e, s, with_kinv=with_kinv) for e in agents for s in range(S)}


def _same_learner(a, b, with_kinv=True):
    keys = ('landmarks', 'coeff') + (('kinv',) if with_kinv else ())
    return a['m'] == b['m'] and all(_bits(a[k]) == _bits(b[k]) for k in keys)


def _same_control(cd, cs, index):
    return all(_bits(cd[k]) == _bits(cs[k][index]) for k in ('margins', 'security_factors', 'action', 'adjusted', 'accuracies'))


def test_identity_and_determinism(src):
    """after fork_from every agent holds its source's dictionaries (landmarks, coefficients, Kinv: bytes), control state,
    sizes and flags; two forks with the same arguments give equal save_state blobs"""
    index = _index(np.random.default_rng(5))
    S = len(src.dims)
    sizes = src.agent.dictionary_sizes()
    assert sizes[BIG] >= 320 and (sizes > 64).sum() >= 1
    dst = src.new_agent(len(index))
    dst.fork_from(src.agent, index)
    want = _learners(src.agent, range(N), S)
    for j, r in enumerate(index):
        for s in range(S):
            assert _same_learner(dst.learner(j, s, with_kinv=True), want[(int(r), s)]), (j, s)
    assert _same_control(dst.control(), src.agent.control(), index)
    assert (dst.dictionary_sizes() == sizes[index]).all()
    fs, fd = src.agent.flagged_replicas(), dst.flagged_replicas()
    for key in ('saturated', 'pool_full'):
        assert fd[key] == [j for j, r in enumerate(index) if int(r) in fs[key]]
    assert dst.stats() == [0, 0, 0, 0]
    # the K_f row of the source's last predict travels with its guards: kb_update without a new kb_predict is refused or
    # accepted alike, and the kernel row is the same
    j = int(np.nonzero(index == BIG[0])[0][0])
    assert _bits(dst.kernel_row(j, BIG[1])) == _bits(src.agent.kernel_row(*BIG))
    twin = src.new_agent(len(index))
    twin.fork_from(src.agent, index)
    assert _bits(dst.save_state()) == _bits(twin.save_state())
    dst.fork_from(src.agent, index)       # and again into the same handle
    assert _bits(dst.save_state()) == _bits(twin.save_state())
    dst.close()
    twin.close()


def _record(src, steps):
    """a closed-loop run of identity forks, host-driven: [(state, action, labels, next obs)] per step"""
    ident = np.arange(N, dtype=np.int32)
    rec, renv = src.fork_pair(ident)
    prev, act, lab, obs = src.prev, src.action, src.labels, src.obs
    seq = []
    for _ in range(steps):
        seq.append((prev, act, lab, obs))
        rec.update_control(prev, act, lab)
        nact, _ = rec.select_action(obs)
        o2, _, _, info = renv.step(nact)
        prev, act, lab, obs = obs, nact, info['SLA_labels'], o2
    rec.close()
    renv.close()
    return seq


def test_continuation_teacher_forced(src):
    """src and dst driven by the same recorded (state, action, labels) sequence, indexed by the fork's index for dst: equal
    update_control hits and select_action outputs at every step, equal dictionaries at the end -- against a source whose
    select-score cache is warm while the fork's restarted"""
    index = _index(np.random.default_rng(6))
    S = len(src.dims)
    seq = _record(src, 20)
    dst = src.new_agent(len(index))
    dst.fork_from(src.agent, index)
    for i, (state, act, lab, obs) in enumerate(seq):
        hs = src.agent.update_control(state, act, lab)
        hd = dst.update_control(state[index], act[index], lab[index])
        assert (hd == hs[index]).all(), i
        a_s, j_s = src.agent.select_action(obs)
        a_d, j_d = dst.select_action(obs[index])
        assert (a_d == a_s[index]).all() and (j_d == j_s[index]).all(), i
        assert (a_s == seq[i + 1][1]).all() if i + 1 < len(seq) else True     # (and the recording was the same run)
    want = _learners(src.agent, range(N), S)
    for j, r in enumerate(index):
        for s in range(S):
            assert _same_learner(dst.learner(j, s, with_kinv=True), want[(int(r), s)]), (j, s)
    assert _same_control(dst.control(), src.agent.control(), index)
    dst.close()


@pytest.mark.parametrize('graph', [False, True])
def test_continuation_closed_loop(src, graph):
    """the agents forked with kb_fork and their environments with rs_fork, same index: run_resident on both pairs records
    equal histories"""
    index = _index(np.random.default_rng(7))
    dst, denv = src.fork_pair(index)
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
    dst.close()
    denv.close()


def _host_learning_step(ag, env, prev, act, lab, obs):
    hits = ag.update_control(prev, act, lab)
    nact, _ = ag.select_action(obs)
    o2, _, _, info = env.step(nact)
    return hits, (obs, nact, info['SLA_labels'], o2)


def test_inference_mode(src):
    """set_learning(False): the resident loop selects only.  F (resident) against a twin G of the same fork driven from the
    host through the oracle-pinned entry points on a second forked environment."""
    index = _index(np.random.default_rng(8))
    n, S = len(index), len(src.dims)
    F, FE = src.fork_pair(index)
    G, GE = src.fork_pair(index)
    F.history_begin(41)
    # one learning step first, so that there are hits to retain
    F.step_resident(FE)
    FE.step_resident()
    hits0, st = _host_learning_step(G, GE, src.prev[index], src.action[index], src.labels[index], src.obs[index])
    assert _bits(FE.fetch()['actions']) == _bits(st[1])
    F.set_learning(False)
    sample = sorted({0, 1, 6, 7, n - 1, int(np.nonzero(index == BIG[0])[0][0])})
    before, ctl0, stats0 = _learners(F, sample, S), F.control(), F.stats()
    obs = st[3]
    for i in range(30):
        F.step_resident(FE)
        a_f = FE.fetch()['actions']
        FE.step_resident()
        a_g, adj_g = G.select_action(obs)
        assert _bits(a_f) == _bits(a_g), i
        prev_obs = obs
        obs, _, _, info = GE.step(a_g)
        last = (prev_obs, a_g, info['SLA_labels'], obs)
    stats1 = F.stats()
    assert stats1[1] == stats0[1] and stats1[2] == stats0[2] and stats1[0] > stats0[0]
    after, ctl1 = _learners(F, sample, S), F.control()
    for key in before:
        assert _same_learner(before[key], after[key]), key
    assert _bits(ctl0['accuracies']) == _bits(ctl1['accuracies']) and _bits(ctl0['security_factors']) == _bits(ctl1['security_factors'])
    assert (F.dictionary_sizes() == G.dictionary_sizes()).all()
    # learning resumes: ten more resident steps equal the twin's, which was never frozen but fed the same select-only steps
    F.set_learning(True)
    st = last
    hits_g = []
    for i in range(10):
        F.step_resident(FE)
        a_f = FE.fetch()['actions']
        FE.step_resident()
        h, st = _host_learning_step(G, GE, *st)
        hits_g.append(h)
        assert _bits(a_f) == _bits(st[1]), i
    hist = F.history_fetch()
    assert hist['recorded'] == 41
    assert (hist['hits'][:, :, 0] == hits0).all()
    for i in range(1, 31):     # the inference columns repeat the retained hits
        assert (hist['hits'][:, :, i] == hits0).all(), i
    for i in range(10):
        assert (hist['hits'][:, :, 31 + i] == hits_g[i]).all(), i
    got, want = _learners(F, sample, S), _learners(G, sample, S)
    for key in got:
        assert _same_learner(got[key], want[key]), key
    assert _same_control(F.control(), G.control(), np.arange(n))
    for h in (F, FE, G, GE):
        h.close()
    # a fresh fork put in inference mode at once has no hits to repeat: zeros
    Z, ZE = src.fork_pair(index[:8])
    Z.set_learning(False)
    Z.history_begin(3)
    Z.run_resident(ZE, 3, graph=False)
    hz = Z.history_fetch()
    assert hz['recorded'] == 3 and not hz['hits'].any() and Z.stats()[1] == 0 and Z.stats()[2] == 0
    Z.close()
    ZE.close()


def test_deploy(src):
    """deploy(index): vector pages only, in a pool of exactly deploy_pool_bytes; it selects as a full fork in inference mode
    does, refuses everything that would need Kinv, and can be deployed again"""
    from ranslice.kbrl_dev import deploy_pool_bytes
    index = _index(np.random.default_rng(9))
    n, S = len(index), len(src.dims)
    sizes = src.agent.dictionary_sizes()
    D = src.agent.deploy(index)
    assert D.frozen and D.n_envs == n
    p = D.pool()
    assert p['used_bytes'] == p['total_bytes'] == deploy_pool_bytes(sizes[index])
    assert p['used_bytes'] < src.agent.pool()['used_bytes']          # 136 agents without Kinv in less than 64 with
    assert (D.dictionary_sizes() == sizes[index]).all()
    want = _learners(src.agent, sorted(set(int(r) for r in index[:12])), S, with_kinv=False)
    for j in range(12):
        for s in range(S):
            assert _same_learner(D.learner(j, s), want[(int(index[j]), s)], with_kinv=False), (j, s)
    assert _same_control(D.control(), src.agent.control(), index)
    x = np.zeros(src.dims[0] + 1)
    refused = [lambda: D.update_control(src.prev[index], src.action[index], src.labels[index]), lambda: D.update(0, 0, x, 1),
               lambda: D.set_learning(True), lambda: D.learner(0, 0, with_kinv=True), lambda: D.save_state(),
               lambda: D.load_state(np.zeros(256, dtype=np.uint8)),
               lambda: D.reset(src.action[index], src.action[index] * 0 + 2)]
    full = src.new_agent(n)
    refused += [lambda: full.fork_from(D, np.arange(n, dtype=np.int32))]
    for k, call in enumerate(refused):
        with pytest.raises(_lib.RanSliceError) as e:
            call()
        assert e.value.code == _lib.RS_ESTATE, k
    D.set_learning(False)     # (already so)
    D2 = D.deploy(np.arange(n, dtype=np.int32))
    assert D2.frozen and D2.pool()['used_bytes'] == p['used_bytes']
    full.fork_from(src.agent, index)
    full.set_learning(False)
    envs = [src.new_env(n, seed=80 + k) for k in range(3)]
    for e in envs:
        e.fork_from(src.env, index)
    agents = [full, D, D2]
    for i in range(30):
        acts = []
        for ag, e in zip(agents, envs):
            ag.step_resident(e)
            acts.append(e.fetch()['actions'])
            e.step_resident()
        assert _bits(acts[1]) == _bits(acts[0]) and _bits(acts[2]) == _bits(acts[0]), i
    assert D.stats()[1] == 0 and D.stats()[2] == 0
    assert D.pool()['used_bytes'] == p['used_bytes']
    for h in agents + envs:
        h.close()


def test_refusals(golden_dir):
    from ranslice.kbrl_dev import SharedVecKBRL
    src = Source(golden_dir, 0)
    idx = np.arange(8, dtype=np.int32)
    for kw in (dict(capacity=512), dict(dims=[10, 10, 10, 10, 3])):
        other = src.new_agent(8, **kw)
        with pytest.raises(_lib.RanSliceError) as e:
            other.fork_from(src.agent, idx)
        assert e.value.code == _lib.RS_EINVAL, kw
        other.close()
    dst = src.new_agent(8)
    for bad in (N, -1):
        j = idx.copy()
        j[3] = bad
        with pytest.raises(_lib.RanSliceError) as e:
            dst.fork_from(src.agent, j)
        assert e.value.code == _lib.RS_EINVAL
        with pytest.raises(_lib.RanSliceError) as e:
            src.agent.deploy(j)
        assert e.value.code == _lib.RS_EINVAL
    never = src.new_agent(8)
    with pytest.raises(_lib.RanSliceError) as e:
        dst.fork_from(never, idx)      # a source that was never reset
    assert e.value.code == _lib.RS_ESTATE
    never.close()
    # a destination pool too small: 8 x 5 first shells fit (kb_create asks for that much), the grown learner's six do not
    small = src.new_agent(8, pool_bytes=2 << 20)
    with pytest.raises(_lib.RanSliceError) as e:
        small.fork_from(src.agent, idx)
    assert e.value.code == _lib.RS_EOVERFLOW
    assert not small.dictionary_sizes().any() and small.pool()['used_bytes'] == 512
    ia = np.full((8, 5), 10, np.int32)
    small.reset(ia, ia * 0 + 2)
    act, _ = small.select_action(src.obs[:8])
    small.update_control(src.obs[:8], act, src.labels[:8])
    assert small.dictionary_sizes().any()
    small.close()
    shared = SharedVecKBRL(8, src.dims, src.n_prbs, capacity=1024)
    shared.reset(ia, ia * 0 + 2)
    for call in (lambda: shared.fork_from(src.agent, idx), lambda: dst.fork_from(shared, idx), lambda: shared.deploy(idx),
                 lambda: shared.set_learning(False)):
        with pytest.raises(_lib.RanSliceError) as e:
            call()
        assert e.value.code == _lib.RS_EINVAL
    shared.close()
    dst.fork_from(src.agent, idx[::-1].copy())      # and the good fork still works after the refusals
    assert (dst.dictionary_sizes() == src.agent.dictionary_sizes()[idx[::-1]]).all()
    dst.close()
    src.close()


def test_graph_replay_in_inference_mode(src):
    """run_resident(graph=True) in inference mode == graph=False == step by step; then learning is switched back on: a loop
    captured in one mode must not be replayed in the other"""
    index = _index(np.random.default_rng(10))
    frozen_steps, learn_steps = 13, 8
    hists, finals = [], []
    for mode in ('graph', 'plain', 'stepwise'):
        ag, env = src.fork_pair(index)
        ag.history_begin(frozen_steps + learn_steps)
        for on, steps in ((False, frozen_steps), (True, learn_steps)):
            ag.set_learning(on)
            if mode == 'stepwise':
                for _ in range(steps):
                    ag.step_resident(env)
                    env.step_resident()
            else:
                ag.run_resident(env, steps, graph=mode == 'graph')
            if not on:
                assert ag.stats()[1] == 0 and ag.stats()[2] == 0
        hists.append(ag.history_fetch())
        finals.append(env.fetch())
        ag.close()
        env.close()
    assert hists[0]['hits'][:, :, frozen_steps:].any()        # learning did resume
    assert not hists[0]['hits'][:, :, :frozen_steps].any()    # and a fresh fork had no hits to repeat
    for h, f in zip(hists[1:], finals[1:]):
        assert h['recorded'] == hists[0]['recorded'] == frozen_steps + learn_steps
        for key in KEYS:
            assert _bits(h[key]) == _bits(hists[0][key]), key
        assert _bits(f['obs']) == _bits(finals[0]['obs']) and _bits(f['actions']) == _bits(finals[0]['actions'])


def test_source_replaying_a_captured_loop_waits_for_the_gather(golden_dir):
    """The source was advanced with run_resident(graph=True) and goes on with graph=True right after the fork: the replayed
    loop runs on the simulator's stream, and must still start behind the gather that is reading the source's dictionaries.
    A fork taken at rest (synchronised before and after) is the reference: equal save_state blobs, byte for byte.  The fork is
    wide (every agent sixteen times) so that the gather takes as long as many steps of the source."""
    src = Source(golden_dir, 0, graph=True, tail=False)      # 1 plain step + 74 captured pairs: the next run replays at once
    index = np.tile(_index(np.random.default_rng(12)), 16).astype(np.int32)
    src.agent.synchronize()
    src.env.synchronize()
    rest = src.new_agent(len(index), pool_bytes=3 << 30)
    rest.fork_from(src.agent, index)
    rest.synchronize()
    want = rest.save_state()
    rest.close()
    for attempt in range(3):
        dst = src.new_agent(len(index), pool_bytes=3 << 30)
        src.agent.synchronize()
        src.env.synchronize()
        dst.fork_from(src.agent, index)
        src.agent.run_resident(src.env, 24, graph=True)      # the cached loop, parities aligned: no plain step first
        got = dst.save_state()
        dst.close()
        # (the source has moved on: the reference for the next attempt is a fork at rest of the source as it now is)
        assert _bits(got) == _bits(want), attempt
        src.agent.synchronize()
        src.env.synchronize()
        rest = src.new_agent(len(index), pool_bytes=3 << 30)
        rest.fork_from(src.agent, index)
        rest.synchronize()
        want = rest.save_state()
        rest.close()
    src.close()


def test_load_state_keeps_pool_full_in_a_pool_of_the_same_size(golden_dir):
    """a handle whose pool was exhausted, saved and loaded into a pool of the same size still reports pool_full (the flag
    travels with the agent, as through kb_fork); a strictly larger pool drops it; the previous blob format is refused by name"""
    from ranslice.kbrl_dev import VecKBRL
    g = np.load(os.path.join(golden_dir, 'g17_projectron_3000.npz'))
    xs = np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1)
    make = lambda pool: VecKBRL(1, [10], 200, capacity=4096, pool_bytes=pool)   # noqa: E731
    ag = make(300 << 10)      # shells 0, 1, 2 (48 + 81 + 114 KB) fit, shell 3 does not
    ag.reset([[10]], [[3]])
    for x, y in zip(xs[:1500], g['y'][:1500]):
        ag.predict(0, 0, x)
        ag.update(0, 0, x, int(y))
    assert ag.dictionary_sizes()[0, 0] == 192 and ag.pool()['pool_full'] == 1
    blob = ag.save_state()
    same = make(300 << 10)
    same.reset([[1]], [[1]])
    same.load_state(blob)
    assert same.pool()['pool_full'] == 1 and same.flagged_replicas()['pool_full'] == [0]
    twin = make(300 << 10)
    twin.fork_from(ag, np.zeros(1, dtype=np.int32))
    assert twin.pool()['pool_full'] == 1
    bigger = make(4 << 20)
    bigger.reset([[1]], [[1]])
    bigger.load_state(blob)
    assert bigger.pool()['pool_full'] == 0 and bigger.dictionary_sizes()[0, 0] == 192
    old = blob.copy()
    old[:8] = np.frombuffer((0x4b42534c49434535).to_bytes(8, 'little'), dtype=np.uint8)
    with pytest.raises(_lib.RanSliceError) as e:
        same.load_state(old)
    assert 'older checkpoint format' in str(e.value)
    for h in (ag, same, twin, bigger):
        h.close()
