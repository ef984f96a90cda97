"""The online budget on the device (kb_set_online_prune, csrc/kb_online_prune.hip), AS BITS.

The budget stage is kb_prune's removal behind every update phase, planned on the device.  The rule forms no sum, so nothing
here carries a tolerance: the stage is held to the host-driven kb_prune at the same points of the same loop (four ways), to
tests/prune_mirror.py loaded with a twin's state removal by removal (carry), and to a handle that never had the switch.

Dictionaries are grown by VecKBRL.fit on prefixes of one seeded random stream per kind of learner, to sizes that straddle the
target and the 64-row seams of Kinv's block storage: 60, 63, 64, 65, 66, 127, 128, 129, 130, 191 and what the carry cases need.
Two fleets at capacity 256 on tests/golden/fading_small.npz: 16 replicas of scenario 0 (five learners of ten state variables,
200 PRBs) and 16 of scenario index 2 (one of ten, four of three, 100 PRBs)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_prune_chain as tpc   # noqa: E402  (_Dev, _load, _hold: a handle's checkpoint as a window on its device state)
from ranslice import _lib   # noqa: E402
from ranslice.config import make_config   # noqa: E402

pytestmark = pytest.mark.gpu

CAP, POOL = 256, 256 << 20
SIZES = (60, 63, 64, 65, 66, 127, 128, 129, 130, 191)
FLAG_UNPRUNED = 32


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _random_stream(rng, d, n, n_prbs, offgrid_every=0, spread=1.0):
    """n samples of d coordinates that are float32 values, the last one an allocation k / n_prbs (every offgrid_every-th off that
    grid), and random labels"""
    xs = (rng.random((n, d)) * spread).astype(np.float32).astype(np.float64)
    xs[:, d - 1] = rng.integers(0, n_prbs + 1, size=n) / float(n_prbs)
    if offgrid_every:
        xs[::offgrid_every, d - 1] += 0.0012345
    return xs, rng.choice([-1, 1], size=n)


class _Fleet:
    """a scenario's shapes, its streams, and the dictionary size after every sample of each kind's stream"""

    def __init__(self, scenario, golden_dir):
        from ranslice.kbrl_dev import VecKBRL
        cfg = make_config(scenario)
        self.scenario, self.n_prbs = scenario, cfg.n_prbs
        self.dims = [10] * cfg.n_embb + [3] * cfg.n_mmtc
        self.S = len(self.dims)
        g = np.load(os.path.join(golden_dir, 'fading_small.npz'))
        self.fading = [g['t0'], g['t1'], g['t2']]
        rng = np.random.default_rng(770 + scenario)
        self.stream = {10: _random_stream(rng, 11, 1500, self.n_prbs, offgrid_every=17),
                       3: _random_stream(rng, 4, 1600, self.n_prbs, offgrid_every=13, spread=4.0)}   # (three variables: spread out)
        kinds = sorted(set(self.dims), reverse=True)
        ag = VecKBRL(1, kinds, self.n_prbs, capacity=CAP, pool_bytes=64 << 20)
        ag.reset([[10] * len(kinds)], [[3] * len(kinds)])
        r = ag.fit([(0, i) for i in range(len(kinds))], [self.stream[k][0] for k in kinds], [self.stream[k][1] for k in kinds])
        self.curve = {k: np.asarray(r['m'][i]).copy() for i, k in enumerate(kinds)}
        ag.close()
        self._blobs = {}

    def ia(self, n):
        return np.tile(np.array([10 if d == 10 else 5 for d in self.dims], dtype=np.int32), (n, 1))

    def sf(self, n):
        return np.tile(np.array([3 if d == 10 else 2 for d in self.dims], dtype=np.int32), (n, 1))

    def agent(self, n, **kw):
        """a reset handle of n replicas (empty dictionaries)"""
        from ranslice.kbrl_dev import VecKBRL
        ag = VecKBRL(n, self.dims, self.n_prbs, capacity=CAP, pool_bytes=POOL, **kw)
        ag.reset(self.ia(n), self.sf(n), seeds=np.arange(n, dtype=np.uint64) + 5)
        return ag

    def env(self, n):
        from ranslice.vec_env import VecRanSlice
        return VecRanSlice(n_envs=n, cfg=make_config(self.scenario, n_envs=n), fading=self.fading, seed=41)

    def grown(self, n, sizes):
        """-> (checkpoint of n replicas whose learner (e, s) holds sizes[(e * S + s) % len(sizes)] landmarks, those sizes [n, S]):
        grown once per (n, sizes) by kb_fit on the shortest prefix of the kind's stream that reaches the size; the blob is never
        edited in place"""
        key = (n, tuple(sizes))
        if key not in self._blobs:
            ag = self.agent(n)
            want = np.array([sizes[t % len(sizes)] for t in range(n * self.S)]).reshape(n, self.S)
            learners, X, Y = [], [], []
            for e in range(n):
                for s, d in enumerate(self.dims):
                    curve = self.curve[d]
                    assert curve.max() >= want[e, s], (d, want[e, s], curve.max())
                    cut = int(np.argmax(curve >= want[e, s])) + 1
                    learners.append((e, s))
                    X.append(self.stream[d][0][:cut])
                    Y.append(self.stream[d][1][:cut])
            ag.fit(learners, X, Y)
            assert (ag.dictionary_sizes() == want).all()
            self._blobs[key] = (ag.save_state(), want)
            ag.close()
        blob, want = self._blobs[key]
        return blob.copy(), want.copy()


_fleets = {}


@pytest.fixture(scope='module')
def fleet(golden_dir):
    def get(scenario):
        if scenario not in _fleets:
            _fleets[scenario] = _Fleet(scenario, golden_dir)
        return _fleets[scenario]
    yield get
    _fleets.clear()


def _snapshot(ag):
    """everything the ways must agree on, as bytes by name"""
    out = {'sizes': _bits(ag.dictionary_sizes()), 'pruned': _bits(ag.pruned()), 'flags': _bits(ag.flags())}
    for k, v in ag.control().items():
        out['control.' + k] = _bits(v)
    for e in range(ag.n_envs):
        for s in range(ag.S):
            L = ag.learner(e, s, with_kinv=True)
            for q in ('landmarks', 'coeff', 'kinv'):
                out['learner(%d, %d).%s' % (e, s, q)] = (L['m'], _bits(L[q]))
    return out


def _agree(a, b, what):
    assert a.keys() == b.keys()
    diff = [k for k in a if a[k] != b[k]]
    assert not diff, '%s: %d items differ, the first: %s' % (what, len(diff), diff[:4])


HIST = ('reward', 'resources', 'hits', 'adjusted', 'SLA', 'violation')


def _host_loop(fl, ag, n, steps, prune_to=None):
    """env.step; update_control; [prune(prune_to)]; select_action -- -> per step (sizes after the update phase and what may follow
    it inside update_control, landmarks the prune call removed)"""
    env = fl.env(n)
    state, action = env.reset(), fl.ia(n)
    log = []
    for _ in range(steps):
        obs, _, _, info = env.step(action)
        ag.update_control(state, action, info['SLA_labels'])
        sizes = ag.dictionary_sizes().copy()
        removed = ag.prune(prune_to) if prune_to else 0
        action, _ = ag.select_action(obs)
        state = obs
        log.append((sizes, removed))
    env.close()
    return log


def _resident_loop(fl, ag, n, steps, graph, env=None):
    """the same loop on the device (kb_run_resident), its histories recorded -> the six history columns"""
    own = env is None
    if own:
        env = fl.env(n)
        env.reset()
        env.enqueue_step(fl.ia(n))
    ag.history_begin(steps)
    ag.run_resident(env, steps, graph=graph)
    ag.synchronize()
    h = ag.history_fetch()
    assert h['recorded'] == steps
    if own:
        env.close()
    return {k: _bits(h[k]) for k in HIST}


def _loaded(fl, n, blob, **kw):
    ag = fl.agent(n, **kw)
    ag.load_state(blob)
    return ag


@pytest.mark.parametrize('scenario,target', [(0, 64), (0, 128), (2, 64), (2, 128)])
def test_the_four_ways_agree(fleet, scenario, target):
    """(a) the host loop with kb_prune(target) between update_control and select_action, switch off; (b) the same host loop with
    the switch on and no prune call; (c) run_resident plain and (d) captured, switch on: the same bytes everywhere.  The sizes
    straddle the target within `rounds`, so (a)'s prune to the target and the stage's min(excess, rounds) are one definition --
    which the carry counter of (b) confirms."""
    fl = fleet(scenario)
    n, steps, rounds = 16, 24, 8
    sizes = [z for z in SIZES if z <= target + 2]
    blob, start = fl.grown(n, sizes)
    assert (start > target).any() and (start <= target).any() and (start - target).max() <= rounds
    a = _loaded(fl, n, blob)
    log = _host_loop(fl, a, n, steps, prune_to=target)
    assert a.online_prune is None and a.online_prune_info()['stages'] == 0
    # the case is not vacuous: removals in at least three steps; a dictionary that started at or below the target inserted in
    # the loop and was pruned there
    removing = [i for i, (_, removed) in enumerate(log) if removed]
    print('scenario %d target %d: removals in steps %s, %d in all; largest size behind an update phase %d'
          % (scenario, target, removing, a.pruned().sum(), max(int(z.max()) for z, _ in log)))
    assert len(removing) >= 3
    assert (a.pruned()[start <= target] > 0).any()
    assert a.dictionary_sizes().max() <= target
    want = _snapshot(a)
    a.close()
    hists = {}
    for way in 'bcd':
        ag = _loaded(fl, n, blob)
        ag.set_online_prune(target, rounds)
        assert ag.online_prune == (target, rounds)
        if way == 'b':
            _host_loop(fl, ag, n, steps)
        else:
            hists[way] = _resident_loop(fl, ag, n, steps, graph=way == 'd')
        info = ag.online_prune_info()
        print('way (%s): %s' % (way, info))
        assert info['stages'] == steps and info['carry'] == 0 and info['flagged'] == 0
        assert info['removed'] == ag.pruned().sum() > 0 and 0 < info['max_excess'] <= rounds
        _agree(want, _snapshot(ag), 'way (%s) against (a)' % way)
        ag.close()
    assert hists['c'] == hists['d']


@pytest.mark.parametrize('rounds', [1, 2])
@pytest.mark.parametrize('scenario,target', [(0, 64), (2, 186)])
def test_carry_against_the_mirror(fleet, scenario, target, rounds):
    """Dictionaries 0, 1, 2 and 5 above the target, at most `rounds` removals per stage.  Before every update_control a twin with
    the switch off is forked from the budgeted handle and given the same rows; a mirror loaded with the TWIN's dictionary and
    advanced by min(excess, rounds) removals must then be the budgeted dictionary: size, victims (the landmark rows by slot),
    coefficients, every stored entry of Kinv, chains and zeros in what was vacated.  The counters are the closed forms."""
    fl = fleet(scenario)
    n, steps = 4, 6
    blob, start = fl.grown(n, [target, target + 1, target + 2, target + 5])
    ag = _loaded(fl, n, blob)
    ag.set_online_prune(target, rounds)
    twin = fl.agent(n)
    dev, tdev = tpc._Dev(ag), tpc._Dev(twin)
    env = fl.env(n)
    state, action = env.reset(), fl.ia(n)
    nd = n * fl.S
    carry = removed = units = 0
    grown_by = np.zeros(nd, dtype=np.int64)
    start, most = start.reshape(-1), 0
    for t in range(steps):
        twin.fork_from(ag, np.arange(n))
        assert twin.online_prune is None
        before = ag.dictionary_sizes().reshape(-1).copy()
        obs, _, _, info = env.step(action)
        h1 = ag.update_control(state, action, info['SLA_labels'])
        h2 = twin.update_control(state, action, info['SLA_labels'])
        assert (h1 == h2).all()
        v, tv = dev.views(), tdev.views()
        for d in range(nd):
            m0 = int(tv['m'][d])
            grown_by[d] += m0 - before[d]
            k = min(max(m0 - target, 0), rounds)
            most = max(most, m0 - target)
            mr = tpc._load(tdev, tv, d)
            for i in range(k):
                assert mr.remove_one()['diag_ok']
                units += dev.units(m0 - i)
            removed += k
            carry += m0 - k > target
            what = 'step %d, dictionary %d (%d landmarks behind the update phase, %d removals)' % (t, d, m0, k)
            tpc._hold(dev, v, d, mr, m0, what)
            assert int(v['m'][d]) == m0 - k, what
            # a dictionary that inserted nothing is at the target after ceil(excess / rounds) stages, and stays there
            if not grown_by[d] and t + 1 >= math.ceil((start[d] - target) / rounds):
                assert int(v['m'][d]) == target, what
        got = ag.online_prune_info()
        assert (got['stages'], got['removed'], got['carry'], got['max_excess'], got['flagged']) == (t + 1, removed, carry, most, 0), (t, got)
        assert got['downdate_bytes'] == units * 16384
        assert ag.pruned().sum() == removed and not twin.pruned().any()
        action, _ = ag.select_action(obs)
        state = obs
    print('scenario %d target %d rounds %d: %d removals, carry %d, insertions per dictionary %s' % (scenario, target, rounds, removed, carry,
                                                                                                  grown_by.tolist()))
    # (an insertion puts a dictionary one landmark further from the target: every one of them is there once ceil(5 / rounds)
    # stages and a stage per insertion have passed, which the sizes above imply; here the run is long enough for the still ones)
    assert carry > 0 and removed >= (start - target).sum() and math.ceil(5 / rounds) <= steps
    quiet = grown_by == 0
    assert (ag.dictionary_sizes().reshape(-1)[quiet] == target).all()
    env.close()
    twin.close()
    ag.close()


def test_projectron_plus_ways_agree(fleet):
    """the fleet of scenario index 2 under Projectron++ (control_plus, eight candidates per pass over Kinv): the stage sits behind
    that update phase as well -- host loop, plain and captured resident loop leave the same bytes, with removals"""
    fl = fleet(2)
    n, steps, target, rounds = 16, 24, 128, 8
    blob, start = fl.grown(n, [z for z in SIZES if z <= target + 2])
    kw = dict(algorithm='projectron_plus', control_plus=True, control_plus_batch=8, control_plus_batch_max=CAP)
    snaps, hists = {}, {}
    for way in 'bcd':
        ag = _loaded(fl, n, blob, **kw)
        assert ag.algorithm == 'projectron_plus' and ag.control_plus_batch[0] == 8
        ag.set_online_prune(target, rounds)
        if way == 'b':
            _host_loop(fl, ag, n, steps)
        else:
            hists[way] = _resident_loop(fl, ag, n, steps, graph=way == 'd')
        info = ag.online_prune_info()
        print('Projectron++, way (%s): %s' % (way, info))
        assert info['stages'] == steps and info['removed'] == ag.pruned().sum() > 0 and info['flagged'] == 0
        snaps[way] = _snapshot(ag)
        ag.close()
    _agree(snaps['b'], snaps['c'], 'Projectron++: (c) against (b)')
    _agree(snaps['b'], snaps['d'], 'Projectron++: (d) against (b)')
    assert hists['c'] == hists['d']


def test_switch(fleet):
    """Switched on and off again before the loop: the bytes of a handle that never had the switch, and no stage counted.  Toggled
    between two captured run_resident calls: the second call runs the stage (the graph of the first is not replayed), and no
    dictionary ends above the target plus what that call inserted (kb_get_stats, [2]); toggled off, the third runs none."""
    fl = fleet(0)
    n, target = 16, 64
    blob, start = fl.grown(n, [z for z in SIZES if z <= 130])
    never, toggled = _loaded(fl, n, blob), _loaded(fl, n, blob)
    toggled.set_online_prune(target, 8)
    toggled.set_online_prune(None)
    assert toggled.online_prune is None and never.online_prune is None
    h1 = _resident_loop(fl, never, n, 8, graph=True)
    h2 = _resident_loop(fl, toggled, n, 8, graph=True)
    assert h1 == h2
    _agree(_snapshot(never), _snapshot(toggled), 'on and off again against never on')
    assert toggled.online_prune_info()['stages'] == 0 and not toggled.pruned().any()
    never.close()
    toggled.close()
    # one handle, one environment, three captured calls
    ag = _loaded(fl, n, blob)
    env = fl.env(n)
    env.reset()
    env.enqueue_step(fl.ia(n))
    _resident_loop(fl, ag, n, 8, graph=True, env=env)
    grown0 = ag.dictionary_sizes()
    assert (grown0 >= start).all() and grown0.max() > 128 and ag.online_prune_info()['stages'] == 0
    ag.set_online_prune(target, 64)
    ins0 = ag.stats()[2]
    _resident_loop(fl, ag, n, 8, graph=True, env=env)
    ins = ag.stats()[2] - ins0
    sizes, info = ag.dictionary_sizes(), ag.online_prune_info()
    print('second call: %d insertions, largest dictionary %d, %s' % (ins, sizes.max(), info))
    assert info['stages'] == 8 and info['removed'] == ag.pruned().sum() >= (grown0 - target).clip(0).sum()
    assert sizes.max() <= target + ins and sizes.max() <= target    # (the stage is the last to touch a dictionary in a step)
    assert info['max_excess'] >= (grown0 - target).max()      # (the first stage met them, and what its step added)
    ag.set_online_prune(0)
    _resident_loop(fl, ag, n, 4, graph=True, env=env)
    after = ag.online_prune_info()
    assert after['stages'] == 8 and after['removed'] == info['removed'] and (ag.dictionary_sizes() >= sizes).all()
    assert not (ag.flags() & FLAG_UNPRUNED).any()
    env.close()
    ag.close()


def test_refusals(fleet):
    """every RS_EINVAL / RS_ESTATE of kb_set_online_prune, its message naming the remedy; the handle stays as it was"""
    from ranslice.kbrl_dev import VecKBRL, SharedVecKBRL
    fl = fleet(0)
    blob, _ = fl.grown(4, [66, 65])
    ag = _loaded(fl, 4, blob)

    def refused(obj, args, code, *words):
        with pytest.raises(_lib.RanSliceError) as ei:
            obj.set_online_prune(*args)
        assert ei.value.code == code and 'kb_set_online_prune' in str(ei.value), str(ei.value)
        for w in words:
            assert w in str(ei.value), (w, str(ei.value))

    for t in (63, 1, -1, CAP - 63, CAP):
        refused(ag, (t, 2), _lib.RS_EINVAL, 'target', 'capacity - 64')
    for r in (0, -1, 65):
        refused(ag, (64, r), _lib.RS_EINVAL, 'rounds', '1 .. 64')
    assert ag.online_prune is None
    for t, r in ((64, 1), (CAP - 64, 64), (0, 2)):
        ag.set_online_prune(t, r)
        assert ag.online_prune == ((t, r) if t else None)
    ag.set_online_prune(70, 3)
    refused(ag, (63, 2), _lib.RS_EINVAL)
    assert ag.online_prune == (70, 3)              # a refusal leaves the setting
    for by_reference in (False, True):
        dep = ag.deploy([0, 1], by_reference=by_reference)
        refused(dep, (64, 2), _lib.RS_ESTATE, 'learning handle', 'deploy again')
        assert dep.select_action(np.zeros((2, 50), dtype=np.float32))[0].shape == (2, 5)
        dep.close()
    sh = SharedVecKBRL(2, [10], 200, capacity=CAP)
    sh.reset([[10]] * 2, [[3]] * 2)
    refused(sh, (64, 2), _lib.RS_ESTATE, 'kb_shared_prune')
    sh.close()
    fresh = VecKBRL(2, [10], 200, capacity=CAP, pool_bytes=64 << 20)
    refused(fresh, (64, 2), _lib.RS_ESTATE, 'kb_reset')
    fresh.close()
    # the constructor's keyword waits for the first reset
    kw = VecKBRL(2, [10], 200, capacity=CAP, pool_bytes=64 << 20, online_prune=64, online_prune_rounds=5)
    assert kw.online_prune == (64, 5)
    kw.reset([[10]] * 2, [[3]] * 2)
    assert kw.online_prune == (64, 5) and kw._online_prune_pending is None
    kw.reset([[10]] * 2, [[3]] * 2)
    assert kw.online_prune == (64, 5)              # kb_reset leaves the switch
    kw.close()
    # the setting is the handle's: a checkpoint does not bring one, a fork does not take it along
    other = fl.agent(4)
    other.load_state(ag.save_state())
    assert other.online_prune is None and ag.online_prune == (70, 3)
    other.set_online_prune(64, 2)
    other.fork_from(ag, np.arange(4))
    assert other.online_prune == (64, 2)
    other.close()
    ag.close()


def test_poisoned_dictionary(fleet):
    """Kinv[5][5] of dictionary 0 is -1 (edited into a checkpoint).  Step by step against a twin forked before the update phase
    and a clean handle given the same rows: the poisoned dictionary keeps the bytes the update phase alone leaves it, its
    replica carries bit 32 and nothing else changes in the flag words, the dictionaries of the other replicas are pruned as in
    the clean run, one dictionary is counted as flagged however many stages meet it; kb_synchronize reports no error and the
    captured loop runs on."""
    fl = fleet(0)
    n, steps, target, rounds = 4, 4, 64, 8
    blob, start = fl.grown(n, [66, 65, 64, 63, 60])
    clean = _loaded(fl, n, blob)
    bad_blob = blob.copy()
    dev0 = tpc._Dev(clean)
    tpc._set_diag(dev0, dev0.views(bad_blob), 0, 5, -1.0)
    bad = _loaded(fl, n, bad_blob)
    twin = fl.agent(n)
    for h in (clean, bad):
        h.set_online_prune(target, rounds)
    assert not bad.flags().any()
    diag = []
    env = fl.env(n)
    state, action = env.reset(), fl.ia(n)
    for t in range(steps):
        twin.fork_from(bad, np.arange(n))
        obs, _, _, info = env.step(action)
        for h in (bad, twin, clean):
            h.update_control(state, action, info['SLA_labels'])
        a, b = bad.learner(0, 0, with_kinv=True), twin.learner(0, 0, with_kinv=True)
        assert a['m'] == b['m'] > target, (t, a['m'], b['m'])
        for q in ('landmarks', 'coeff', 'kinv'):
            assert _bits(a[q]) == _bits(b[q]), (t, q)
        diag.append(float(a['kinv'][5, 5]))
        assert diag[-1] < 0.0, diag          # (the insertions' rank-1 updates move it, by d[5]^2 / delta each; it stays what the stage refuses)
        f = bad.flags()
        assert (f & FLAG_UNPRUNED).tolist() == [FLAG_UNPRUNED, 0, 0, 0] and (f[1:] == clean.flags()[1:]).all(), f
        assert f[0] & ~FLAG_UNPRUNED == twin.flags()[0] & ~FLAG_UNPRUNED
        for e in range(1, n):
            for s in range(fl.S):
                a, b = bad.learner(e, s, with_kinv=True), clean.learner(e, s, with_kinv=True)
                assert a['m'] == b['m'] <= target, (t, e, s)
                for q in ('landmarks', 'coeff', 'kinv'):
                    assert _bits(a[q]) == _bits(b[q]), (t, e, s, q)
        assert (bad.pruned()[1:] == clean.pruned()[1:]).all() and bad.pruned()[0, 0] == 0
        i = bad.online_prune_info()
        assert i['stages'] == t + 1 and i['flagged'] == 1 and clean.online_prune_info()['flagged'] == 0, i
        action, _ = bad.select_action(obs)
        clean.select_action(obs)
        state = obs
    assert bad.pruned()[1:].sum() > 0
    assert not (clean.flags() & FLAG_UNPRUNED).any()
    env.close()
    env = fl.env(n)
    env.reset()
    env.enqueue_step(fl.ia(n))
    _resident_loop(fl, bad, n, 6, graph=True, env=env)       # (synchronize inside: bit 32 is no error)
    assert bad.online_prune_info()['stages'] == steps + 6 and bad.online_prune_info()['flagged'] == 1
    assert (bad.flags() & FLAG_UNPRUNED).tolist() == [FLAG_UNPRUNED, 0, 0, 0]
    diag.append(float(bad.learner(0, 0, with_kinv=True)['kinv'][5, 5]))
    print('Kinv[5][5] of the poisoned dictionary behind every update phase, and at the end:', diag)
    assert diag[-1] < 0.0 and bad.dictionary_sizes()[1:].max() <= target < bad.dictionary_sizes()[0, 0]
    env.close()
    for h in (clean, bad, twin):
        h.close()
