"""VecKBRL: N independent KBRL agents (one per env replica) on one MI355X.

Batched form of the reference's kbrl_control.KBRL_Control (reference kbrl_control.py:23-157): every
agent keeps its own per-slice Projectron dictionaries on the device; update_control / select_action
run as HIP kernels (network-slicing_amd/csrc/kb_kbrl.hip) behind the kb_* C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from .sharding import replica_seeds
from .config import KbConfig, KBRL_ALFA, KBRL_ETA, KBRL_GAMMA

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint64)


VEC_PAGE_BYTES = 30 * 64 * 8   # one shell of an inference-only handle: the vector page of 64 landmarks (KB_VEC doubles)
POOL_PREAMBLE_BYTES = 64 * 8   # pool offset 0 means "no shell": every pool starts with 64 unused doubles
ALGORITHMS = {'projectron': 0, 'projectron_plus': 1}   # KB_ALG_PROJECTRON, KB_ALG_PROJECTRON_PLUS (ranslice.h)


def deploy_pool_bytes(sizes):
    """bytes kb_deploy allocates (and kb_get_pool then reports in use) for dictionaries of these sizes: the 512-byte preamble
    that keeps offset 0 free for "not allocated", plus one 15,360-byte vector page per started 64 landmarks -- no Kinv"""
    m = np.asarray(sizes, dtype=np.int64)
    return POOL_PREAMBLE_BYTES + VEC_PAGE_BYTES * int(((m + 63) // 64).sum())


def deploy_ref_pool_bytes(sizes, index):
    """bytes kb_deploy_ref's handle reports as its pool: deploy_pool_bytes of the DISTINCT agents of `index` (sizes: the
    source's [n_envs, S] dictionary sizes) -- every dictionary somebody references once, whatever the number of replicas"""
    m = np.asarray(sizes, dtype=np.int64)
    return deploy_pool_bytes(m[np.unique(np.asarray(index, dtype=np.int64))])


def fork_pool_bytes(sizes):
    """bytes of pool a learning handle needs to take dictionaries of these sizes through fork_from: per shell b of a
    dictionary one vector page and b + 1 Kinv tiles of 32 KB with their 1 KB partial-sum areas, plus the preamble"""
    nsh = (np.asarray(sizes, dtype=np.int64) + 63) // 64
    return POOL_PREAMBLE_BYTES + int((VEC_PAGE_BYTES * nsh + (32768 + 1024) * nsh * (nsh + 1) // 2).sum())


def shared_pool_bytes(sizes):
    """bytes of pool a shared-dictionary handle needs to take dictionaries of these sizes through to_shared: per shell b of a
    dictionary one vector page and 2 b + 1 Kinv tiles of 32 KB (both block triangles, no partial-sum areas), plus the preamble"""
    nsh = (np.asarray(sizes, dtype=np.int64) + 63) // 64
    return POOL_PREAMBLE_BYTES + int((VEC_PAGE_BYTES * nsh + 32768 * nsh * nsh).sum())


def augmented_samples(state, action, labels, dims, n_prbs):
    """the per-learner sample lists of the reference's sample augmentation (kbrl_control.py:103-112) for a log of control steps,
    on the host (pure numpy): state [steps, sum(dims)], action [steps, S], labels [steps, S] (+1 fulfilled / -1 not) ->
    (X, y), lists over the S learners of arrays [n_s, dims[s] + 1] float64 and [n_s] int8.  Step by step in log order, a step
    with label +1 gives the allocations action .. n_prbs (the same or more PRBs would have fulfilled too), one with -1 the
    allocations 0 .. action, in that order; a sample is (the learner's state variables, allocation / n_prbs) with the step's
    label.  The lists feed VecKBRL.fit, whatever produced the log -- the reference, a deployed fleet, the clairvoyant baseline.
    Limits: fit forms f in predict's summation order, update_control through the binned / MFMA scoring chain, so the two take
    the same decisions except where f is within rounding of zero -- bit-equality with update_control is not claimed; and the
    stop of the augmentation at a full dictionary (build-defined in the oracle) is not reproduced.
    VecKBRL.fit_steps generates exactly these samples on the device from the log itself; this is their statement on the host."""
    state = np.asarray(state, dtype=np.float64)
    state = state.reshape(-1, int(sum(dims)))
    steps = state.shape[0]
    action = np.asarray(action, dtype=np.int64).reshape(steps, len(dims))
    labels = np.asarray(labels, dtype=np.int64).reshape(steps, len(dims))
    if ((labels != 1) & (labels != -1)).any():
        raise ValueError('augmented_samples: labels must be +1 or -1')
    if (action < 0).any() or (action > n_prbs).any():
        raise ValueError('augmented_samples: actions must lie in 0 .. n_prbs')
    X, Y, off = [], [], 0
    for s, d in enumerate(dims):
        xs, ys = [], []
        for t in range(steps):
            a, lab = int(action[t, s]), int(labels[t, s])
            alloc = np.arange(a, n_prbs + 1) if lab == 1 else np.arange(0, a + 1)
            x = np.empty((alloc.size, d + 1))
            x[:, :d] = state[t, off:off + d]
            x[:, d] = alloc / n_prbs
            xs.append(x)
            ys.append(np.full(alloc.size, lab, dtype=np.int8))
        X.append(np.concatenate(xs) if xs else np.zeros((0, d + 1)))
        Y.append(np.concatenate(ys) if ys else np.zeros(0, dtype=np.int8))
        off += d
    return X, Y


class VecKBRL:
    frozen = False   # True on the inference-only objects deploy() returns
    by_reference = False   # True on those deploy(index, by_reference=True) returns: dictionaries stored once per distinct agent

    def __init__(self, n_envs, dims, n_prbs, alfa=KBRL_ALFA, accuracy_range=(0.99, 0.999), gamma=KBRL_GAMMA,
                 eta=KBRL_ETA, capacity=4096, device=0, shared=False, first_env=0, pool_bytes=0, algorithm='projectron',
                 control_plus=False, control_plus_batch=0, control_plus_batch_max=1024, fit_steps_batch=0, fit_steps_batch_max=1024,
                 control_plus_wide=0, control_plus_wide_max=2048, control_plus_wide_rounds=32, online_prune=None,
                 online_prune_rounds=2):
        if algorithm not in ALGORITHMS:
            raise ValueError('algorithm must be one of %s, not %r' % (sorted(ALGORITHMS), algorithm))
        if online_prune is not None and shared:
            raise ValueError('online_prune=%r: shared-dictionary handles hold no budget in the loop (SharedVecKBRL.prune between '
                             'steps is the call there)' % (online_prune,))
        # (kb_set_online_prune wants a reset handle: the keyword is kept and set by the first reset())
        self._online_prune_pending = None if online_prune is None else (int(online_prune), int(online_prune_rounds))
        self.L = _lib.load()
        cfg = KbConfig()
        cfg.n_envs, cfg.n_slices, cfg.n_prbs, cfg.capacity = n_envs, len(dims), n_prbs, capacity
        for i, d in enumerate(dims):
            cfg.dims[i] = int(d)
        cfg.alfa, cfg.acc_lo, cfg.acc_hi = alfa, accuracy_range[0], accuracy_range[1]
        cfg.gamma, cfg.eta = gamma, eta
        cfg.shared_dictionary, cfg.first_env = int(bool(shared)), int(first_env)
        cfg.pool_bytes = int(pool_bytes)
        self.cfg = cfg
        self.n_envs, self.S, self.n_prbs, self.dims = n_envs, len(dims), n_prbs, list(dims)
        self.nv = int(sum(dims))
        self.capacity = capacity
        self.device = int(device)
        self.h = C.c_void_p()
        self._check(self.L.kb_create(C.byref(cfg), int(device), C.byref(self.h)))
        if algorithm != 'projectron':
            self.set_algorithm(algorithm)
        if control_plus:
            self.set_control_plus(True)
        if control_plus_batch:
            self.set_control_plus_batch(control_plus_batch, control_plus_batch_max)
        if fit_steps_batch:
            self.set_fit_steps_batch(fit_steps_batch, fit_steps_batch_max)
        if control_plus_wide:
            self.set_control_plus_wide(control_plus_wide, control_plus_wide_max, control_plus_wide_rounds)

    def set_algorithm(self, algorithm):
        """the update rule of the next update() / fit() (kb_set_algorithm): 'projectron' (the default; projectron.py:39-60) or
        'projectron_plus' (Projectron++, projectron.py:71-107: a sample classified correctly inside the margin 0 < y f < 1 gives
        a scaled projection, never a landmark).  A property of this handle, not of its dictionaries: checkpoints and agent files do
        not hold it, fork_from / deploy / load_agents / unshare_from do not carry it over.  While in 'projectron_plus',
        update_control and the learning resident loop are refused (RS_ESTATE) unless set_control_plus() is on; select_action, score, prune, deploy, export work.
        Refused (RS_ESTATE) on deployed, by-reference and shared-dictionary handles."""
        if algorithm not in ALGORITHMS:
            raise ValueError('algorithm must be one of %s, not %r' % (sorted(ALGORITHMS), algorithm))
        self._check(self.L.kb_set_algorithm(self.h, ALGORITHMS[algorithm]))

    @property
    def algorithm(self):
        """'projectron' or 'projectron_plus' (kb_get_algorithm)"""
        a = C.c_int32()
        self._check(self.L.kb_get_algorithm(self.h, C.byref(a)))
        return {v: k for k, v in ALGORITHMS.items()}[a.value]

    def _check(self, rc):
        if rc != 0:
            msg = self.L.kb_last_error(self.h).decode() if self.h else 'kb_create failed'
            raise _lib.RanSliceError(rc, msg)

    def close(self):
        if getattr(self, 'h', None):
            self.L.kb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, initial_action, security_factor, seeds=None):
        ia = np.ascontiguousarray(initial_action, dtype=np.int32).reshape(self.n_envs, self.S)
        sf = np.ascontiguousarray(security_factor, dtype=np.int32).reshape(self.n_envs, self.S)
        if seeds is None:
            seeds = replica_seeds(0, self.cfg.first_env, self.n_envs)   # tie-break streams (kernel.py:26-27)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self.L.kb_reset(self.h, ia.ctypes.data_as(_ip), sf.ctypes.data_as(_ip), seeds.ctypes.data_as(_up)))
        if getattr(self, '_online_prune_pending', None):   # VecKBRL(online_prune=...): the switch is the handle's from here on
            pending, self._online_prune_pending = self._online_prune_pending, None
            self.set_online_prune(*pending)

    def update_control(self, state, action, labels):
        state = np.ascontiguousarray(state, dtype=np.float32).reshape(self.n_envs, self.nv)
        action = np.ascontiguousarray(action, dtype=np.int32).reshape(self.n_envs, self.S)
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(self.n_envs, self.S)
        hits = np.zeros((self.n_envs, self.S), dtype=np.int32)
        self._check(self.L.kb_update_control(self.h, state.ctypes.data_as(_fp), action.ctypes.data_as(_ip),
                                             labels.ctypes.data_as(_ip), hits.ctypes.data_as(_ip)))
        return hits

    def select_action(self, state):
        state = np.ascontiguousarray(state, dtype=np.float32).reshape(self.n_envs, self.nv)
        action = np.zeros((self.n_envs, self.S), dtype=np.int32)
        adjusted = np.zeros(self.n_envs, dtype=np.int32)
        self._check(self.L.kb_select_action(self.h, state.ctypes.data_as(_fp), action.ctypes.data_as(_ip),
                                            adjusted.ctypes.data_as(_ip)))
        return action, adjusted

    def _same_library(self, env):
        # an agent handle and an environment handle that meet in one call must come from the same image of the library (the test
        # build's structures need not match the production build's: ranslice._lib.load picks per handle)
        if env.L is not self.L:
            raise RuntimeError('the agent and the environment were created from different builds of libranslice '
                               '(RANSLICE_DEV_BUILD changed between the two constructors?)')

    def step_resident(self, env):
        self._same_library(env)
        self._check(self.L.kb_step_resident(self.h, env.h))

    def run_resident(self, env, n_steps, graph=True):
        """n_steps x (step_resident(env); env.step_resident()) from one call (kb_run_resident); graph: two captured steps
        replayed as a hipGraph -- same results, a fraction of the launches"""
        self._same_library(env)
        self._check(self.L.kb_run_resident(self.h, env.h, int(n_steps), 1 if graph else 0))

    def history_begin(self, steps):
        """start recording KBRL_Control.run's per-step histories on the device (one column per step_resident)"""
        self._hist_steps = int(steps)
        self._check(self.L.kb_history_begin(self.h, int(steps)))

    def history_fetch(self):
        """-> dict of the reference's result arrays per replica: reward f64 [N, steps]; resources, adjusted, SLA,
        violation int16 [N, steps]; hits int16 [N, S, steps] (kbrl_control.py:148-155), and `recorded`"""
        n, st = self.n_envs, self._hist_steps
        sp = C.POINTER(C.c_int16)
        out = dict(reward=np.zeros((n, st)), resources=np.zeros((n, st), dtype=np.int16),
                   hits=np.zeros((n, self.S, st), dtype=np.int16), adjusted=np.zeros((n, st), dtype=np.int16),
                   SLA=np.zeros((n, st), dtype=np.int16), violation=np.zeros((n, st), dtype=np.int16))
        rec = C.c_int32()
        self._check(self.L.kb_history_fetch(self.h, out['reward'].ctypes.data_as(_dp), out['resources'].ctypes.data_as(sp),
                                            out['hits'].ctypes.data_as(sp), out['adjusted'].ctypes.data_as(sp),
                                            out['SLA'].ctypes.data_as(sp), out['violation'].ctypes.data_as(sp),
                                            C.byref(rec)))
        out['recorded'] = rec.value
        return out

    def predict(self, e, s, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        y, f = C.c_int32(), C.c_double()
        self._check(self.L.kb_predict(self.h, e, s, x.ctypes.data_as(_dp), C.byref(y), C.byref(f)))
        return y.value, f.value

    def update(self, e, s, x, y):
        """Projectron.update(x, y) on the (f, k) cached by the preceding predict(e, s, x) -> (branch, delta).  branch: 0 nothing,
        1 projection, 2 the dictionary grew; in 'projectron_plus' mode (set_algorithm) also 3 margin update (coefficients moved,
        no landmark added) and 4 margin test that changed nothing.  delta is the projection residual, formed for branches 1-4."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        br, dl = C.c_int32(), C.c_double()
        self._check(self.L.kb_update(self.h, e, s, x.ctypes.data_as(_dp), int(y), C.byref(br), C.byref(dl)))
        return br.value, dl.value

    def _pack_rows(self, learners, X, who):
        """(task [n] int32, first [n + 1] int64, rows [first[n], 16] float64) of per-learner arrays [n_i, dims[s] + 1]"""
        learners = [(int(e), int(s)) for e, s in learners]
        if len(X) != len(learners):
            raise ValueError('%s: %d learners but %d arrays' % (who, len(learners), len(X)))
        for e, s in learners:
            if not (0 <= e < self.n_envs and 0 <= s < self.S):
                raise ValueError('%s: (%d, %d) names no learner' % (who, e, s))
        task = np.array([e * self.S + s for e, s in learners], dtype=np.int32).reshape(-1)
        first = np.zeros(len(learners) + 1, dtype=np.int64)
        arrs = []
        for i, ((e, s), x) in enumerate(zip(learners, X)):
            d = self.dims[s] + 1
            x = np.asarray(x, dtype=np.float64)
            x = x.reshape(-1, d) if x.size else np.zeros((0, d))
            arrs.append(x)
            first[i + 1] = first[i] + x.shape[0]
        rows = np.zeros((int(first[-1]), 16))
        for i, ((e, s), x) in enumerate(zip(learners, arrs)):
            rows[first[i]:first[i + 1], :x.shape[1]] = x
        return task, first, rows

    def fit(self, learners, X, y, chunk=0):
        """teacher-forced online learning of many learners in one call (kb_fit; build-defined): learners = [(e, s), ...] all
        distinct, X[i] = [n_i, dims[s] + 1] samples of learner i in order, y[i] = [n_i] labels +1 / -1.  For every learner and
        sample in order: predict(x_t), then update(x_t, y_t) -- bit for bit what the one-by-one predict / update calls leave,
        one workgroup per learner on the device.  chunk: most samples of one learner per launch (0: the default); no result
        depends on it.  -> dict of per-learner lists of arrays: y_pred, f, branch (0 none, 1 projection, 2 grew; in
        'projectron_plus' mode also 3 margin update, 4 margin test without update -- see update()), delta and m (the dictionary's
        size after the sample).  The cached predict of the touched learners is invalid afterwards."""
        task, first, rows = self._pack_rows(learners, X, 'fit')
        if len(y) != len(task):
            raise ValueError('fit: %d learners but %d label arrays' % (len(task), len(y)))
        lab = np.zeros(int(first[-1]), dtype=np.int8)
        for i, yi in enumerate(y):
            yi = np.asarray(yi).reshape(-1)
            if yi.size != first[i + 1] - first[i]:
                raise ValueError('fit: learner %d has %d samples but %d labels' % (i, first[i + 1] - first[i], yi.size))
            if ((yi != 1) & (yi != -1)).any():
                raise ValueError('fit: labels must be +1 or -1')
            lab[first[i]:first[i + 1]] = yi
        R = int(first[-1])
        yp, br, ma = (np.zeros(R, dtype=np.int32) for _ in range(3))
        f, dl = np.zeros(R), np.zeros(R)
        i64p, i8p = C.POINTER(C.c_int64), C.POINTER(C.c_int8)
        self._check(self.L.kb_fit(self.h, task.ctypes.data_as(_ip), int(task.size), first.ctypes.data_as(i64p),
                                  rows.ctypes.data_as(_dp), lab.ctypes.data_as(i8p), int(chunk), yp.ctypes.data_as(_ip),
                                  f.ctypes.data_as(_dp), br.ctypes.data_as(_ip), dl.ctypes.data_as(_dp), ma.ctypes.data_as(_ip)))
        cut = lambda a: [a[first[i]:first[i + 1]] for i in range(task.size)]
        return dict(y_pred=cut(yp), f=cut(f), branch=cut(br), delta=cut(dl), m=cut(ma))

    def _pack_steps(self, agents, state, action, labels):
        """(agent [n] int32, first [n + 1] int64, state [rows, nv] float32, action, labels [rows, S] int32) of per-agent logs;
        every shape, label and action is checked here (ValueError), before the library is touched"""
        agents = [int(e) for e in agents]
        for name, v in (('state', state), ('action', action), ('labels', labels)):
            if len(v) != len(agents):
                raise ValueError('fit_steps: %d agents but %d %s logs' % (len(agents), len(v), name))
        for e in agents:
            if not 0 <= e < self.n_envs:
                raise ValueError('fit_steps: %d names no agent (0 .. %d)' % (e, self.n_envs - 1))
        first = np.zeros(len(agents) + 1, dtype=np.int64)
        st, ac, lb = [], [], []
        for i, (x, a, l) in enumerate(zip(state, action, labels)):
            x, a, l = np.asarray(x, dtype=np.float32), np.asarray(a), np.asarray(l)
            if x.ndim != 2 or x.shape[1] != self.nv:
                raise ValueError('fit_steps: state of agent %d has shape %s, not [T, %d]' % (agents[i], x.shape, self.nv))
            for name, v in (('action', a), ('labels', l)):
                if v.shape != (x.shape[0], self.S):
                    raise ValueError('fit_steps: %s of agent %d has shape %s, not %s' % (name, agents[i], v.shape, (x.shape[0], self.S)))
            if (a != np.rint(a)).any() or (l != np.rint(l)).any():
                raise ValueError('fit_steps: actions and labels are integers')
            a, l = a.astype(np.int64), l.astype(np.int64)
            if ((l != 1) & (l != -1) & (l != 0)).any():
                raise ValueError('fit_steps: labels must be +1, -1 or 0 (the learner skips the row)')
            if (((a < 0) | (a > self.n_prbs)) & (l != 0)).any():
                raise ValueError('fit_steps: actions must lie in 0 .. n_prbs')
            st.append(x)
            ac.append(a.astype(np.int32))
            lb.append(l.astype(np.int32))
            first[i + 1] = first[i] + x.shape[0]
        cat = lambda v, w, t: np.ascontiguousarray(np.concatenate(v), dtype=t) if v else np.zeros((0, w), dtype=t)
        return (np.array(agents, dtype=np.int32).reshape(-1), first, cat(st, self.nv, np.float32), cat(ac, self.S, np.int32),
                cat(lb, self.S, np.int32))

    def fit_steps(self, agents, state, action, labels, chunk=0):
        """teach agents from logs of control steps, augmented on the device (kb_fit_steps; build-defined): agents = [e, ...] all
        distinct; state / action / labels either lists over the agents of arrays [T_i, nv] float32 / [T_i, S] / [T_i, S], or
        arrays [n, T, ...].  labels: +1 fulfilled, -1 not, 0 = this learner skips the row.  Learner s of agent i is taught, row by
        row, exactly the samples augmented_samples makes of the rows -- bit for bit what fit(..., *augmented_samples(...)) leaves,
        in the handle's algorithm -- while only the log itself is staged (about 250 bytes per agent and step, not 16 doubles per
        sample).  chunk: most log rows of one agent per launch (0: the default); no result depends on it.  -> dict of per-agent
        lists of arrays [T_i, S]: f_at (f at the logged allocation before the row's first sample), y_at (its sign; 0 on a tie or
        an empty dictionary), changed (samples of the row that changed the dictionary), grown (insertions) and m (the size after
        the row).  One workgroup per learner (in 'projectron_plus' mode set_fit_steps_batch lets the candidates of a row share
        their pass over Kinv, with the same bits); set_fit_wide has no effect here.  The cached predict of the learners that
        received samples is invalid afterwards; fit_time_ms() reports the call like a fit."""
        agent, first, st, ac, lb = self._pack_steps(agents, state, action, labels)
        R = int(first[-1])
        f_at = np.zeros((R, self.S))
        y_at, ch, gr, ma = (np.zeros((R, self.S), dtype=np.int32) for _ in range(4))
        self._check(self.L.kb_fit_steps(self.h, agent.ctypes.data_as(_ip), int(agent.size), first.ctypes.data_as(C.POINTER(C.c_int64)),
                                        st.ctypes.data_as(_fp), ac.ctypes.data_as(_ip), lb.ctypes.data_as(_ip), int(chunk),
                                        f_at.ctypes.data_as(_dp), y_at.ctypes.data_as(_ip), ch.ctypes.data_as(_ip),
                                        gr.ctypes.data_as(_ip), ma.ctypes.data_as(_ip)))
        cut = lambda a: [a[first[i]:first[i + 1]] for i in range(agent.size)]
        return dict(f_at=cut(f_at), y_at=cut(y_at), changed=cut(ch), grown=cut(gr), m=cut(ma))

    def score(self, learners, X):
        """read-only scoring of query sets (kb_score; build-defined): learners = [(e, s), ...] (repeats allowed), X[i] =
        [n_i, dims[s] + 1] points -> (f, y_pred), lists of arrays [n_i]: f is bit for bit what predict(e, s, x) returns, y_pred
        its sign and 0 on an exact tie or an empty dictionary (no draw is taken).  Nothing in the handle changes -- no cached
        row, counter or tie stream -- so it works on learning, deployed (copy and by reference), imported and shared handles."""
        task, first, rows = self._pack_rows(learners, X, 'score')
        R = int(first[-1])
        f, yp = np.zeros(R), np.zeros(R, dtype=np.int32)
        self._check(self.L.kb_score(self.h, task.ctypes.data_as(_ip), int(task.size), first.ctypes.data_as(C.POINTER(C.c_int64)),
                                    rows.ctypes.data_as(_dp), f.ctypes.data_as(_dp), yp.ctypes.data_as(_ip)))
        return ([f[first[i]:first[i + 1]] for i in range(task.size)], [yp[first[i]:first[i + 1]] for i in range(task.size)])

    def fit_time_ms(self):
        """of the last fit / score on this handle (kb_fit_time_ms): dict(fit_ms, score_ms = device time of their launches when
        set_kernel_timing was on at the call, else 0; samples, mistakes, insertions of the last fit; kernel_evals = landmarks x
        samples of the last fit plus landmarks x queries of the last score)"""
        ms = (C.c_double * 2)()
        w = (C.c_uint64 * 4)()
        self._check(self.L.kb_fit_time_ms(self.h, ms, w))
        return dict(fit_ms=ms[0], score_ms=ms[1], samples=int(w[0]), mistakes=int(w[1]), insertions=int(w[2]), kernel_evals=int(w[3]))

    def set_fit_wide(self, min_landmarks, window=0):
        """which learners fit() teaches by chip-wide rounds (kb_set_fit_wide): 0 (the default) none -- fit() is one workgroup per
        learner; min_landmarks >= 2: every listed learner whose dictionary holds that many landmarks at the start of a chunk is
        taught that chunk in rounds that spread each mistake's mat-vec and rank-1 update over the whole device.  Every result is
        bit for bit the narrow path's.  window: samples per learner a round scores ahead (1 .. 256; 0: the default, 64).  A
        property of this handle, like the algorithm: not saved, not carried over by fork_from / deploy / load_agents.  Ignored in
        'projectron_plus' mode unless set_fit_wide_plus() is on too.  Refused (RS_ESTATE) on deployed, by-reference and
        shared-dictionary handles; 1 and negative values are refused (RS_EINVAL)."""
        self._check(self.L.kb_set_fit_wide(self.h, int(min_landmarks), int(window)))

    def set_fit_wide_plus(self, on=True):
        """whether the chip-wide rounds of set_fit_wide also teach in 'projectron_plus' mode (kb_set_fit_wide_plus).  Off (the
        default): that mode keeps the one-workgroup path whatever set_fit_wide says.  On: learners that hold set_fit_wide's
        min_landmarks at the start of a chunk are taught by rounds there too -- every mistake AND every sample inside the margin
        has its mat-vec spread over the device, with the narrow path's bits.  No effect in 'projectron' mode or while
        set_fit_wide is off.  A property of this handle: not saved, not carried over.  Refused (RS_ESTATE) on deployed,
        by-reference and shared-dictionary handles."""
        self._check(self.L.kb_set_fit_wide_plus(self.h, int(on)))

    @property
    def fit_wide_plus(self):
        """True while set_fit_wide_plus is on (kb_get_fit_wide_plus)"""
        a = C.c_int32()
        self._check(self.L.kb_get_fit_wide_plus(self.h, C.byref(a)))
        return bool(a.value)

    def set_control_plus(self, on=True):
        """whether the closed control loop learns in 'projectron_plus' mode (kb_set_control_plus).  Off (the default):
        update_control, step_resident and run_resident with learning on are refused in that mode.  On: they run, and every learner
        takes its step's candidates through the margin rule -- per step exactly what fit_steps does with that step's log row in
        'projectron_plus' mode, bit for bit, behind update_control's bookkeeping (hit, accuracy table, security factor).  One
        workgroup per learner: late in learning many times the cost of Projectron's loop.  No effect in 'projectron' mode.  A
        property of this handle: not saved, not carried over by fork_from / deploy / load_agents.  Refused (RS_ESTATE) on
        deployed, by-reference and shared-dictionary handles."""
        self._check(self.L.kb_set_control_plus(self.h, int(bool(on))))

    @property
    def control_plus(self):
        """True while set_control_plus is on (kb_get_control_plus)"""
        a = C.c_int32()
        self._check(self.L.kb_get_control_plus(self.h, C.byref(a)))
        return bool(a.value)

    def set_control_plus_batch(self, width, max_landmarks=1024):
        """how many candidates of a step share one pass over Kinv while the closed loop learns in 'projectron_plus' mode with
        set_control_plus on (kb_set_control_plus_batch): 0 (the default) one by one, or 2, 4, 8.  max_landmarks (a multiple of 64,
        64 .. capacity) is the largest dictionary that is grouped; a larger one takes its candidates one by one.  Bit for bit the
        results of width 0.  The scratch -- min(n_envs x S, 1024) arenas of 2 x width x max_landmarks doubles -- is allocated
        here and freed at width 0.  No effect in 'projectron' mode or while set_control_plus is off.  A property of this handle:
        not saved, not carried over.  Refused (RS_ESTATE) on deployed, by-reference and shared-dictionary handles."""
        self._check(self.L.kb_set_control_plus_batch(self.h, int(width), int(max_landmarks)))

    @property
    def control_plus_batch(self):
        """(width, max_landmarks, scratch_bytes) of set_control_plus_batch (kb_get_control_plus_batch); (0, 0, 0) while it is off"""
        a, b, n = C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self.L.kb_get_control_plus_batch(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def control_plus_batch_work(self):
        """kb_control_plus_batch_info since the width was last set: groups formed, groups skipped (nobody inside the margin), passes
        over Kinv, tiles they read, d* columns formed, columns discarded behind an insertion, candidates taken one by one, of those
        the ones that ran the mat-vec"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_control_plus_batch_info(self.h, w))
        return [int(v) for v in w]

    def set_control_plus_wide(self, min_landmarks, max_landmarks=2048, rounds=32):
        """which learners of the closed loop's 'projectron_plus' update phase have their passes over Kinv spread over the chip
        (kb_set_control_plus_wide): 0 (the default) none -- every row on one workgroup, as set_control_plus_batch leaves it -- else
        those that hold min_landmarks (2 or more) .. max_landmarks (a multiple of 64, 64 .. capacity) at the start of a step, in task
        order the first 1024 of them -- and no more than set_control_plus_batch's max_landmarks, beyond which that walk goes one by one.  They advance in `rounds` (1 .. 256) rounds of chip-wide launches -- the pass of a group of
        candidates, the walk of its members, the rank-1 update of an insertion -- and a finishing launch completes what is left,
        so the results do not depend on `rounds`: bit for bit those of the same width with this switch off.  It has an effect only
        in 'projectron_plus' mode with set_control_plus on and a set_control_plus_batch width of 2, 4 or 8.  The scratch (a record
        and an arena of 2 x 8 x max_landmarks doubles per slot) is allocated here and freed at 0.  A property of this handle: not
        saved, not carried over.  Refused (RS_ESTATE) on deployed, by-reference and shared-dictionary handles."""
        self._check(self.L.kb_set_control_plus_wide(self.h, int(min_landmarks), int(max_landmarks), int(rounds)))

    @property
    def control_plus_wide(self):
        """(min_landmarks, max_landmarks, rounds, scratch_bytes) of set_control_plus_wide (kb_get_control_plus_wide); zeros while off"""
        a, b, r, n = C.c_int32(), C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self.L.kb_get_control_plus_wide(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(n)))
        return a.value, b.value, r.value, n.value

    def control_plus_wide_work(self):
        """kb_control_plus_wide_info since the switch was last set: heavy rows taken, learners turned away because the slots were
        full, learner-rounds that made a spread pass, tiles read in them, rank-1 units spread, rows that reached the finisher
        unfinished, candidates the finisher walked, update phases launched in this mode"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_control_plus_wide_info(self.h, w))
        return [int(v) for v in w]

    def set_fit_steps_batch(self, width, max_landmarks=1024):
        """how many candidates of a log row share one pass over Kinv while fit_steps teaches in 'projectron_plus' mode
        (kb_set_fit_steps_batch): 0 (the default) one by one, or 2, 4, 8.  max_landmarks (a multiple of 64, 64 .. capacity) is the
        largest dictionary that is grouped; a larger one takes its candidates one by one.  Bit for bit the results of width 0,
        the returned summaries included.  The scratch -- min(n_envs x S, 1024) arenas of 2 x width x max_landmarks doubles, its
        own and not set_control_plus_batch's -- is allocated here and freed at width 0.  No effect in 'projectron' mode.  A
        property of this handle: not saved, not carried over.  Refused (RS_ESTATE) on deployed, by-reference and
        shared-dictionary handles."""
        self._check(self.L.kb_set_fit_steps_batch(self.h, int(width), int(max_landmarks)))

    @property
    def fit_steps_batch(self):
        """(width, max_landmarks, scratch_bytes) of set_fit_steps_batch (kb_get_fit_steps_batch); (0, 0, 0) while it is off"""
        a, b, n = C.c_int32(), C.c_int32(), C.c_uint64()
        self._check(self.L.kb_get_fit_steps_batch(self.h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, n.value

    def fit_steps_batch_work(self):
        """kb_fit_steps_batch_info of the last fit_steps (zeros while the width is 0 or the mode 'projectron'): groups formed, groups
        skipped (nobody inside the margin), passes over Kinv, tiles they read, d* columns formed, columns discarded behind an
        insertion, candidates taken one by one, of those the ones that ran the mat-vec"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_fit_steps_batch_info(self.h, w))
        return [int(v) for v in w]

    @property
    def fit_wide(self):
        """(min_landmarks, window) of set_fit_wide (kb_get_fit_wide); (0, 0) while the wide path is off"""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.kb_get_fit_wide(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fit_wide_info(self):
        """what the rounds of the last fit did (kb_fit_wide_info): dict(samples, matvecs, tiles = Kinv tiles of 32,768 bytes those
        mat-vecs read, scan_evals = samples scored x landmarks of the window scans); zeros when nothing went wide"""
        w = (C.c_uint64 * 4)()
        self._check(self.L.kb_fit_wide_info(self.h, w))
        return dict(samples=int(w[0]), matvecs=int(w[1]), tiles=int(w[2]), scan_evals=int(w[3]))

    def learner(self, e, s, with_kinv=False):
        m = C.c_int32()
        self._check(self.L.kb_get_learner(self.h, e, s, C.byref(m), None, None, None))
        m = m.value
        d = self.dims[s] + 1
        L = np.zeros((m, d))
        co = np.zeros(m)
        kinv = np.zeros((m, m)) if with_kinv else None
        if m:
            self._check(self.L.kb_get_learner(self.h, e, s, None, L.ctypes.data_as(_dp), co.ctypes.data_as(_dp),
                                              kinv.ctypes.data_as(_dp) if with_kinv else None))
        return dict(m=m, landmarks=L, coeff=co, kinv=kinv)

    def control(self, with_accuracies=True):
        """margins / security_factors / action [N, S], adjusted [N] and (optionally: it is the big one) the
        accuracy tables [N, S, n_prbs]"""
        T = (self.n_envs, self.S)
        margins, security, action = (np.zeros(T, dtype=np.int32) for _ in range(3))
        adjusted = np.zeros(self.n_envs, dtype=np.int32)
        acc = np.zeros(T + (self.n_prbs,)) if with_accuracies else None
        self._check(self.L.kb_get_control(self.h, margins.ctypes.data_as(_ip), security.ctypes.data_as(_ip),
                                          action.ctypes.data_as(_ip), adjusted.ctypes.data_as(_ip),
                                          acc.ctypes.data_as(_dp) if with_accuracies else None))
        return dict(margins=margins, security_factors=security, action=action, adjusted=adjusted, accuracies=acc)

    def kernel_row(self, e, s):
        """GaussianKernel.k(x) of the last predict(e, s, x) (kernel.py:13-20)"""
        m = C.c_int32()
        self._check(self.L.kb_get_kernel_row(self.h, e, s, C.byref(m), None))
        row = np.zeros(max(m.value, 1))
        if m.value:
            self._check(self.L.kb_get_kernel_row(self.h, e, s, C.byref(m), row.ctypes.data_as(_dp)))
        return row[:m.value] if m.value else np.array([0.0])  # empty dictionary: K_f = [0.0] (projectron.py:35-36)

    def set_adjusted(self, adjusted):
        a = np.ascontiguousarray(adjusted, dtype=np.int32).reshape(self.n_envs)
        self._check(self.L.kb_set_adjusted(self.h, a.ctypes.data_as(_ip)))

    def stats(self):
        s = (C.c_uint64 * 4)()
        self._check(self.L.kb_get_stats(self.h, s))
        return [int(v) for v in s]

    def dictionary_sizes(self):
        """landmarks held by every dictionary: [n_envs, S] (one agent per replica) or [S] (shared)"""
        n = self.S if self.cfg.shared_dictionary else self.n_envs * self.S
        m = np.zeros(n, dtype=np.int32)
        self._check(self.L.kb_get_sizes(self.h, m.ctypes.data_as(_ip)))
        return m if self.cfg.shared_dictionary else m.reshape(self.n_envs, self.S)

    def pool(self):
        """the dictionary pool: dict(used_bytes, total_bytes, saturated = replicas with a dictionary at its capacity,
        pool_full = replicas that found the pool exhausted)"""
        u, t = C.c_uint64(), C.c_uint64()
        ns, nf = C.c_int32(), C.c_int32()
        self._check(self.L.kb_get_pool(self.h, C.byref(u), C.byref(t), C.byref(ns), C.byref(nf)))
        return dict(used_bytes=u.value, total_bytes=t.value, saturated=ns.value, pool_full=nf.value)

    def flagged_replicas(self):
        """replicas whose err word carries 'a dictionary is at its capacity' (bit 8) / 'the pool was exhausted' (bit 16)"""
        e = np.zeros(self.n_envs, dtype=np.int32)
        self._check(self.L.kb_get_flags(self.h, e.ctypes.data_as(_ip)))
        return dict(saturated=[int(k) for k in np.nonzero(e & 8)[0]], pool_full=[int(k) for k in np.nonzero(e & 16)[0]])

    def flags(self):
        """the per-replica flag words int32 [n_envs] (kb_get_flags): bit 8 a dictionary reached its capacity, bit 16 the pool was
        exhausted, bit 32 the budget stage (set_online_prune) left a dictionary of the replica unpruned.  All sticky."""
        e = np.zeros(self.n_envs, dtype=np.int32)
        self._check(self.L.kb_get_flags(self.h, e.ctypes.data_as(_ip)))
        return e

    def repair_work(self):
        """bytes the chip-wide repair rounds streamed since reset: dict(matvec_bytes read, rank1_bytes read + written,
        matvec_launches, rank1_launches) -- counted by the kernels from their work plan (kb_get_repair_work)"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_get_repair_work(self.h, w))
        return dict(matvec_bytes=int(w[0]) * (32768 + 1024), rank1_bytes=int(w[1]) * 16384, matvec_launches=int(w[2]),
                    rank1_launches=int(w[3]), direct_passes=int(w[4]), direct_landmarks=int(w[5]))

    def _repair_raw(self):
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_get_repair_work(self.h, w))
        return list(w)

    def set_kernel_timing(self, enable=True):
        self._check(self.L.kb_set_kernel_timing(self.h, int(bool(enable))))

    def kernel_time_ms(self):
        ms, n = C.c_double(), C.c_int64()
        self._check(self.L.kb_kernel_time_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def phase_times_ms(self):
        """mean device time of the timed launches since the last call: dict(update_ms, select_ms, n_update, n_select) --
        the update phase is update_control_kernel plus the repair kernels"""
        ms = (C.c_double * 2)()
        n = (C.c_int64 * 2)()
        self._check(self.L.kb_phase_times_ms(self.h, ms, n))
        rm = (C.c_double * 2)()
        rn = (C.c_int64 * 2)()
        self._check(self.L.kb_repair_times_ms(self.h, rm, rn))
        km = (C.c_double * 8)()
        kn = (C.c_int64 * 8)()
        self._check(self.L.kb_kernel_times_ms(self.h, km, kn))
        return dict(update_ms=ms[0], select_ms=ms[1], n_update=n[0], n_select=n[1],
                    matvec_launch_ms=rm[0], rank1_launch_ms=rm[1], n_matvec=rn[0], n_rank1=rn[1],
                    select_bin_launch_ms=km[4], n_select_bin=kn[4], finish_launch_ms=km[5], n_finish=kn[5],
                    select_gemm_launch_ms=km[6], n_select_gemm=kn[6], update_small_launch_ms=km[7], n_update_small=kn[7])

    def save_state(self):
        """the handle's whole state as one uint8 array (kb_save_state): feed it to load_state of a handle of the same
        configuration -- this one later, or a fresh one in another process -- and the run goes on bit for bit"""
        n = C.c_uint64()
        self._check(self.L.kb_state_bytes(self.h, C.byref(n)))
        blob = np.empty(n.value, dtype=np.uint8)
        self._check(self.L.kb_save_state(self.h, blob.ctypes.data_as(C.c_void_p), n.value))
        return blob

    def load_state(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self.L.kb_load_state(self.h, blob.ctypes.data_as(C.c_void_p), blob.size))
        self._hist_steps = int(np.frombuffer(blob[32:40].tobytes(), dtype=np.uint64)[0])  # kb_state_header.hist_steps

    def synchronize(self):
        self._check(self.L.kb_synchronize(self.h))

    # ---- agent fork, deployment, inference mode --------------------------------------------
    def fork_from(self, src, index, rebuild=False):
        """agent j of this handle := agent index[j] of `src` (kb_fork): a VecKBRL of the same configuration but n_envs and
        pool_bytes, on the same device.  Dictionaries (Kinv included), control state, tie-break stream and flags travel;
        statistics and caches restart.  Continuing agent j gives, bit for bit, what continuing src agent index[j] would.
        rebuild=True (kb_fork_rebuild): `src` may be an inference-only VecKBRL (deploy(index), load_agents(blob)), which holds
        no Kinv -- it is rebuilt on the device by replaying the insertions in slot order, bit for bit the Kinv of the learning
        handle the agents came from as long as their landmarks were never reordered (rebuild_stats())."""
        index = np.ascontiguousarray(index, dtype=np.int32)
        if index.shape != (self.n_envs,):
            raise ValueError('fork_from: index must have n_envs = %d entries' % self.n_envs)
        if src.L is not self.L:
            raise RuntimeError('the two agents were created from different builds of libranslice')
        fork = self.L.kb_fork_rebuild if rebuild else self.L.kb_fork
        self._check(fork(self.h, src.h, index.ctypes.data_as(_ip)))

    def rebuild_stats(self):
        """of the last fork_from(..., rebuild=True) into this handle: dict(min_delta [n_envs, S] = the smallest delta the replay
        met per dictionary (1.0 below two landmarks; at or below eta: the slot order is not an insertion order -- pruned or
        foreign --, which is legitimate), matvec_tiles, rank1_units, matvec_bytes read, rank1_bytes read + written, rounds,
        dictionaries, replay_ms = device time of the replay when set_kernel_timing was on at the call, else 0)"""
        md = np.zeros((self.n_envs, self.S))
        w = (C.c_uint64 * 4)()
        self._check(self.L.kb_get_rebuild(self.h, md.ctypes.data_as(_dp), w))
        ms = C.c_double()
        self._check(self.L.kb_rebuild_time_ms(self.h, C.byref(ms)))
        return dict(min_delta=md, matvec_tiles=int(w[0]), rank1_units=int(w[1]), matvec_bytes=int(w[0]) * (32768 + 1024),
                    rank1_bytes=int(w[1]) * 16384, rounds=int(w[2]), dictionaries=int(w[3]), replay_ms=ms.value)

    def deploy(self, index, by_reference=False):
        """-> an inference-only VecKBRL (frozen = True) of len(index) agents, agent j := agent index[j] of this one
        (kb_deploy): landmarks and coefficients only, in a pool of exactly deploy_pool_bytes(sizes[index]) bytes.  It selects
        (select_action, step_resident, run_resident) and never learns.
        by_reference=True (kb_deploy_ref): the replicas of an agent share ONE read-only copy of its dictionaries -- the pool is
        deploy_ref_pool_bytes(sizes, index) bytes, the distinct agents once; control state and tie-break streams stay per
        replica and every result equals the copy's bit for bit.  pool(), dictionary_sizes() and learner(e, s) answer per
        replica; predict() and kernel_row() are refused (they would write into a shared page)."""
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        h = C.c_void_p()
        deploy = self.L.kb_deploy_ref if by_reference else self.L.kb_deploy
        self._check(deploy(self.h, index.ctypes.data_as(_ip), int(index.size), C.byref(h)))
        d = object.__new__(type(self))
        d.L, d.h = self.L, h
        cfg = KbConfig.from_buffer_copy(self.cfg)
        cfg.n_envs = int(index.size)
        d.cfg = cfg
        d.n_envs, d.S, d.n_prbs, d.dims, d.nv, d.capacity = int(index.size), self.S, self.n_prbs, list(self.dims), self.nv, self.capacity
        d.frozen = True
        d.device = self.device
        d.by_reference = bool(by_reference)
        cfg.pool_bytes = d.pool()['total_bytes']
        return d

    # ---- agent files --------------------------------------------------------------------------
    def export_agents(self, index):
        """-> the agent file (bytes, ranslice.agent_file) of agents index[0], index[1], ... of this handle (kb_export_agents):
        landmarks, coefficients and control state, no Kinv -- what load_agents turns back into deployed agents, in this process
        or another.  A learning handle or a copy-deployed one; repeats and permutations allowed; the handle is not changed."""
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        n = C.c_uint64()
        self._check(self.L.kb_export_bytes(self.h, index.ctypes.data_as(_ip), int(index.size), C.byref(n)))
        blob = np.empty(n.value, dtype=np.uint8)
        self._check(self.L.kb_export_agents(self.h, index.ctypes.data_as(_ip), int(index.size), blob.ctypes.data_as(C.c_void_p), n.value))
        return blob.tobytes()

    @classmethod
    def load_agents(cls, blob, index=None, by_reference=False, device=0, learning=False, capacity=None, pool_bytes=None):
        """-> an inference-only VecKBRL (frozen = True) holding the agents of an agent file in file order (kb_import_agents):
        bit for bit the handle deploy() would have made of the exported agents.  index: fan out instead -- replica j := agent
        index[j] of the file, through deploy(index, by_reference); the intermediate handle is released.
        learning=True: -> a LEARNING VecKBRL of the file's agents (index: replica j := agent index[j]; default all, in file
        order) whose Kinv is rebuilt on the device (fork_from(..., rebuild=True)): update_control, update, run_resident,
        save_state and fork_from work, and the agents continue as the handle they were exported from would.  capacity: the
        learning handle's limit per dictionary (default: the file's; at least its largest dictionary); pool_bytes: default
        fork_pool_bytes of the chosen dictionaries plus room for each to grow by two shells."""
        if learning and by_reference:
            raise ValueError('load_agents: learning=True builds a handle with dictionaries (and Kinv) of its own; by_reference=True '
                             'shares read-only ones -- choose one')
        L = _lib.load()
        if learning and capacity is not None:
            from . import agent_file
            blob = agent_file.with_capacity(blob, capacity)
        raw = np.frombuffer(bytes(blob), dtype=np.uint8)
        cfg = KbConfig()
        if L.kb_agents_info(raw.ctypes.data_as(C.c_void_p) if raw.size else None, raw.size, C.byref(cfg), None) != 0:
            raise _lib.RanSliceError(_lib.RS_EINVAL, L.kb_last_error(None).decode())
        h = C.c_void_p()
        rc = L.kb_import_agents(raw.ctypes.data_as(C.c_void_p), raw.size, int(device), C.byref(h))
        if rc != 0:
            raise _lib.RanSliceError(rc, L.kb_last_error(None).decode())
        d = object.__new__(cls)
        d.L, d.h, d.cfg = L, h, cfg
        d.n_envs, d.S, d.n_prbs, d.capacity = int(cfg.n_envs), int(cfg.n_slices), int(cfg.n_prbs), int(cfg.capacity)
        d.dims = [int(cfg.dims[s]) for s in range(d.S)]
        d.nv = int(sum(d.dims))
        d.device = int(device)
        d.frozen = True
        if learning:
            try:
                idx = np.arange(d.n_envs, dtype=np.int32) if index is None else np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
                if idx.size == 0 or idx.min() < 0 or idx.max() >= d.n_envs:
                    raise ValueError('load_agents: index must name agents 0 .. %d of the file' % (d.n_envs - 1))
                if pool_bytes is None:
                    sizes = d.dictionary_sizes()[idx]
                    pool_bytes = fork_pool_bytes(np.minimum(sizes + 128, d.capacity))
                ag = cls(int(idx.size), d.dims, d.n_prbs, alfa=cfg.alfa, accuracy_range=(cfg.acc_lo, cfg.acc_hi), gamma=cfg.gamma,
                         eta=cfg.eta, capacity=d.capacity, device=device, pool_bytes=int(pool_bytes))
                try:
                    ag.fork_from(d, idx, rebuild=True)
                except Exception:
                    ag.close()
                    raise
                return ag
            finally:
                d.close()
        if index is None:
            return d
        try:
            return d.deploy(index, by_reference=by_reference)
        finally:
            d.close()

    # ---- the bridge to shared dictionaries ----------------------------------------------------
    def to_shared(self, agent, n_envs, ctl_index=None, budget=64, max_rounds=4, first_env=0, pool_bytes=None):
        """-> a SharedVecKBRL of n_envs replicas whose S dictionaries are those of agent `agent` of this (learning, per-replica)
        handle (kb_share): landmarks, coefficients and Kinv bit for bit, the upper block triangle filled in by transposition.
        Replica j takes the control state, tie-break stream, last observation and flags of agent ctl_index[j] (default: `agent`
        for all).  The fleet goes on learning together from there; an inference-only VecKBRL goes through
        load_agents(..., learning=True) / fork_from(..., rebuild=True) first.  pool_bytes: default the library's own for a
        shared handle (every dictionary at its capacity, bounded)."""
        if ctl_index is not None:
            ctl_index = np.ascontiguousarray(ctl_index, dtype=np.int32).reshape(-1)
            if ctl_index.shape != (int(n_envs),):
                raise ValueError('to_shared: ctl_index must have n_envs = %d entries' % n_envs)
        cfg = self.cfg
        sh = SharedVecKBRL(int(n_envs), self.dims, self.n_prbs, budget=budget, max_rounds=max_rounds, alfa=cfg.alfa,
                           accuracy_range=(cfg.acc_lo, cfg.acc_hi), gamma=cfg.gamma, eta=cfg.eta, capacity=self.capacity,
                           device=self.device, first_env=first_env, pool_bytes=int(pool_bytes or 0))
        try:
            sh.share_from(self, agent, ctl_index)
        except Exception:
            sh.close()
            raise
        return sh

    def bridge_time_ms(self):
        """of the last to_agents / to_shared INTO this handle: dict(ms = device time of the gather when set_kernel_timing was on
        at the call, else 0; read_bytes, written_bytes from its work plan) (kb_bridge_time_ms)"""
        ms = C.c_double()
        b = (C.c_uint64 * 2)()
        self._check(self.L.kb_bridge_time_ms(self.h, C.byref(ms), b))
        return dict(ms=ms.value, read_bytes=int(b[0]), written_bytes=int(b[1]))

    def unshare_from(self, shared, index):
        """agent j of this (learning, per-replica) handle := a private copy of `shared`'s dictionaries with the control state of
        its replica index[j] (kb_unshare); what SharedVecKBRL.to_agents does into a handle it creates"""
        index = np.ascontiguousarray(index, dtype=np.int32)
        if index.shape != (self.n_envs,):
            raise ValueError('unshare_from: index must have n_envs = %d entries' % self.n_envs)
        if shared.L is not self.L:
            raise RuntimeError('the two agents were created from different builds of libranslice')
        self._check(self.L.kb_unshare(self.h, shared.h, index.ctypes.data_as(_ip)))

    def set_learning(self, on):
        """on=False: step_resident / run_resident select only (KBRL_Control.run past learning_time); True resumes learning"""
        self._check(self.L.kb_set_learning(self.h, int(bool(on))))

    # ---- budgeted dictionaries ------------------------------------------------------------------
    def prune(self, target):
        """every dictionary above `target` landmarks is brought down to exactly `target` (kb_prune): one landmark at a time, the
        one whose loss changes the classifier least (smallest coeff^2 / Kinv[j][j]) is folded into the survivors and Kinv
        downdated exactly.  Shells are kept (pool()['used_bytes'] does not move).  Call it between run_resident stretches.
        -> landmarks removed by the call"""
        n = C.c_uint64()
        self._check(self.L.kb_prune(self.h, int(target), C.byref(n)))
        return int(n.value)

    def pruned(self):
        """landmarks removed per dictionary [n_envs, S] since reset / load_state / fork_from (not part of a checkpoint)"""
        n = self.S if self.cfg.shared_dictionary else self.n_envs * self.S
        out = np.zeros(n, dtype=np.int64)
        self._check(self.L.kb_get_pruned(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))))
        return out if self.cfg.shared_dictionary else out.reshape(self.n_envs, self.S)

    def prune_times_ms(self):
        """with set_kernel_timing on: device time summed over the launches of the three prune kernels since the last call, their
        launch counts, and the downdate's bytes (read + written) since reset, counted from its work plan (kb_get_prune_work)"""
        ms = (C.c_double * 3)()
        n = (C.c_int64 * 3)()
        self._check(self.L.kb_prune_time_ms(self.h, ms, n))
        w = (C.c_uint64 * 2)()
        self._check(self.L.kb_get_prune_work(self.h, w))
        return dict(choose_ms=ms[0], downdate_ms=ms[1], move_ms=ms[2], n_choose=n[0], n_downdate=n[1], n_move=n[2],
                    downdate_bytes=int(w[0]) * 16384, downdate_launches=int(w[1]))

    def set_online_prune(self, target, rounds=2):
        """the online budget (kb_set_online_prune): from now on every update phase -- update_control,
        step_resident, run_resident with or without its graph, Projectron or Projectron++ under set_control_plus -- is followed
        on the device by a budget stage: every dictionary above `target` landmarks loses min(excess, rounds) of them by prune()'s
        rule, bit for bit, before select_action reads it; what is left above the target the next stages take.  target None or
        0: off (the default).  64 <= target <= capacity - 64; 1 <= rounds <= 64.  Call it after reset() (the constructor's
        online_prune= is set by the first reset()).  A property of this handle: checkpoints do not hold it; load_state, fork_from,
        unshare_from and load_agents leave it alone.  A dictionary the stage cannot prune (a Kinv diagonal entry that is not
        finite and positive) stays as it is and its replica gets bit 32 of flags().  pruned() counts the removals."""
        self._check(self.L.kb_set_online_prune(self.h, int(target or 0), int(rounds)))

    @property
    def online_prune(self):
        """None while the budget stage is off, else (target, rounds) (kb_get_online_prune)"""
        pending = getattr(self, '_online_prune_pending', None)
        if pending:
            return pending
        t, r = C.c_int32(), C.c_int32()
        self._check(self.L.kb_get_online_prune(self.h, C.byref(t), C.byref(r)))
        return (t.value, r.value) if t.value else None

    def online_prune_info(self):
        """the budget stages since reset / load_state / fork_from, counted on the device (kb_online_prune_info): stages
        enqueued, landmarks removed, carry (dictionary-stages left above the target), the largest excess a stage met, the
        dictionaries flagged, and the downdate's bytes (read + written)"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_online_prune_info(self.h, w))
        return dict(stages=int(w[0]), removed=int(w[1]), carry=int(w[2]), max_excess=int(w[3]), flagged=int(w[4]),
                    downdate_bytes=int(w[5]) * 16384)


PROP_W = 18  # KB_PROP_WIDTH


def merge_proposals(all_counts, all_props, budget):
    """Merge per-rank proposal lists into the list every rank applies: by slice, ascending global replica id,
    truncated to `budget`.  all_counts [W][S], all_props [W][S][budget][PROP_W] -> (counts [S], props
    [S][budget][PROP_W], taken [W][S] = how many of rank w's proposers made it).  Pure host logic (tested on
    CPU with gloo): the result does not depend on how replicas are sharded over ranks."""
    all_counts = np.asarray(all_counts)
    all_props = np.asarray(all_props)
    W, S = all_counts.shape
    out = np.zeros((S, budget, PROP_W))
    counts = np.zeros(S, dtype=np.int32)
    taken = np.zeros((W, S), dtype=np.int32)
    for s in range(S):
        rows = []
        for w in range(W):
            n = min(int(all_counts[w, s]), budget)
            for i in range(n):
                rows.append((all_props[w, s, i, 0], w, i))
        rows.sort()
        rows = rows[:budget]
        for j, (_, w, i) in enumerate(rows):
            out[s, j] = all_props[w, s, i]
            taken[w, s] += 1
        counts[s] = len(rows)
    return counts, out, taken


class SharedVecKBRL(VecKBRL):
    """One KBRL dictionary per slice index, learned from every replica of every rank (build-defined
    extension; the reference trains one independent agent per run).

    Default: the whole learning step runs on the device (kb_shared_step) -- scan, all-gather of the proposal blocks
    over RCCL (bound directly by libranslice.so, on the agent's HIP stream), merge, apply, commit.  One process per
    GPU joins the communicator with `comm_init(unique_id, rank, world)`; `SharedVecKBRL.unique_id()` is generated by
    one rank and distributed by whatever launched the ranks.  Without comm_init the handle is its own world.

    `exchange(counts, props)` (optional) replaces the device exchange by a host callback that must return the lists of
    all ranks stacked on a leading axis ([W][S], [W][S][budget][PROP_W]) and this rank's index: used to run several
    handles side by side in ONE process (tests) and to pin the merge rule on CPU (merge_proposals, gloo test).

    `shared_plus=True` (or set_shared_plus()): the rounds learn by ProjectronPlus.update instead of Projectron.update
    (kb_set_shared_plus).  A replica proposes its first candidate with y f < 1 instead of y f <= 0; a merged
    list is applied in order by the margin rule -- y f >= 1 nothing, y f <= 0 Projectron's projection or insertion, in between the
    scaled projection coeff += alpha y d* when its slack is positive -- and a taken proposer moves past its candidate whichever
    branch the sample took.  Every rank of a group must set the same value before the same step.  stats()[1] then counts
    the samples that changed a dictionary (branches 1-3), kb_get_repair_work's work[6] those whose branch was 1-4.

    `shared_plus_batch=M` (or set_shared_plus_batch()): under the margin rule, a dictionary of M <= m < capacity landmarks takes
    its merged list in segments between insertions, each with the chip-wide passes a full dictionary gets (kb_set_shared_plus_batch,
    DESIGN.md section 8r); None is off.  `shared_plus_segments` segment rounds are enqueued per apply; the results do not depend on it.

    `shared_online_prune=T` (or set_shared_online_prune()): every learning step ends on the device with a budget stage that takes
    up to `shared_online_prune_rounds` landmarks from each dictionary above T by shrink()'s rule (kb_set_shared_online_prune,
    DESIGN.md section 8t); None is off.  The keyword is kept until the first reset(), as VecKBRL(online_prune=) is."""

    def __init__(self, n_envs, dims, n_prbs, budget=64, max_rounds=4, exchange=None, shared_plus=False, shared_plus_batch=None,
                 shared_plus_segments=4, shared_online_prune=None, shared_online_prune_rounds=2, **kw):
        if kw.get('algorithm', 'projectron') != 'projectron':
            raise ValueError("SharedVecKBRL learns through its proposal rounds: algorithm=%r is not supported (the rounds learn by "
                             "the margin rule of 'projectron_plus' with shared_plus=True; or fit a per-replica VecKBRL, then "
                             "to_shared)" % kw['algorithm'])
        if kw.get('online_prune') is not None:
            raise ValueError("SharedVecKBRL holds no budget in the loop: online_prune=%r is not supported (prune() between steps "
                             "brings its dictionaries down to a target; or run a per-replica VecKBRL with online_prune)"
                             "; the shared handle's own switch is shared_online_prune=" % (kw['online_prune'],))
        # (kb_set_shared_online_prune wants a reset handle: the keyword is kept and set by the first reset())
        self._shared_online_prune_pending = ((int(shared_online_prune), int(shared_online_prune_rounds))
                                             if shared_online_prune else None)   # (0 or None: off, nothing pending)
        super().__init__(n_envs, dims, n_prbs, shared=True, **kw)
        self.budget, self.max_rounds = budget, max_rounds
        self.exchange = exchange
        self.rounds_last = 0
        if shared_plus:
            self.set_shared_plus(True)
        if shared_plus_batch:
            self.set_shared_plus_batch(shared_plus_batch, shared_plus_segments)

    def set_shared_plus(self, on=True):
        """whether the proposal rounds learn by the margin rule of Projectron++ (kb_set_shared_plus); off is the default.  Between
        steps only: refused while a host-driven round is open."""
        self._check(self.L.kb_set_shared_plus(self.h, int(bool(on))))

    @property
    def shared_plus(self):
        """True while set_shared_plus is on (kb_get_shared_plus)"""
        a = C.c_int32()
        self._check(self.L.kb_get_shared_plus(self.h, C.byref(a)))
        return bool(a.value)

    def set_shared_plus_batch(self, min_landmarks, segments=4):
        """from how many landmarks on a shared dictionary that can still grow takes a merged list in segments under the margin
        rule (kb_set_shared_plus_batch): 0 or None (the default) never, else 2 .. capacity; `segments` (0 .. 16) segment rounds are
        enqueued per apply and a finishing launch takes the rest.  Remembered, but it acts only while set_shared_plus is on.
        Between steps only; every rank of a group sets the same min_landmarks."""
        self._check(self.L.kb_set_shared_plus_batch(self.h, int(min_landmarks or 0), int(segments)))

    @property
    def shared_plus_batch(self):
        """(min_landmarks, segments) of set_shared_plus_batch (kb_get_shared_plus_batch); min_landmarks 0 while off"""
        a, b = C.c_int32(), C.c_int32()
        self._check(self.L.kb_get_shared_plus_batch(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def shared_plus_batch_work(self):
        """kb_shared_plus_batch_info since reset: engaged lists, segments walked, proposals covered by the segments' wide passes,
        segments ended by a stop, segments run by the finishing launch; the rest 0"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_shared_plus_batch_info(self.h, w))
        return [int(v) for v in w]

    def reset(self, initial_action, security_factor, seeds=None):
        super().reset(initial_action, security_factor, seeds)
        if getattr(self, '_shared_online_prune_pending', None):   # SharedVecKBRL(shared_online_prune=...): the handle's from here on
            pending, self._shared_online_prune_pending = self._shared_online_prune_pending, None
            self.set_shared_online_prune(*pending)

    def set_shared_online_prune(self, target, rounds=2):
        """the online budget of the shared handle (kb_set_shared_online_prune): from now on every learning
        step -- update_control, step_resident -- ends on the device with a budget stage: every dictionary above `target` landmarks
        loses min(excess, rounds) of them by shrink()'s rule, bit for bit, before select_action reads it; what is left above the
        target the next stages take.  target None or 0: off (the default).  64 <= target <= capacity - 1; 1 <= rounds <= 64.
        Call it after reset() (the constructor's shared_online_prune= is set by the first reset()), between steps.  A property of
        this handle: checkpoints do not hold it, reset() and load_state() leave it alone, to_shared() makes a handle with it off.
        Every rank of a group sets the same value before the same step; nothing checks it across ranks.  A dictionary the stage
        cannot prune (a Kinv diagonal entry that is not finite and positive) stays as it is and every replica gets bit 32 of
        flags().  pruned() counts the removals.  With `exchange` given, update_control enqueues the stage behind its rounds."""
        self._check(self.L.kb_set_shared_online_prune(self.h, int(target or 0), int(rounds)))

    @property
    def shared_online_prune(self):
        """None while the budget stage is off, else (target, rounds) (kb_get_shared_online_prune)"""
        pending = getattr(self, '_shared_online_prune_pending', None)
        if pending:
            return pending
        t, r = C.c_int32(), C.c_int32()
        self._check(self.L.kb_get_shared_online_prune(self.h, C.byref(t), C.byref(r)))
        return (t.value, r.value) if t.value else None

    def shared_online_prune_info(self):
        """the budget stages since reset / load_state, counted on the device (kb_shared_online_prune_info): online_prune_info()'s
        entries -- stages enqueued, landmarks removed, carry (dictionary-stages left above the target), the largest excess a stage
        met, the dictionaries flagged, and the downdate's bytes (read + written)"""
        w = (C.c_uint64 * 8)()
        self._check(self.L.kb_shared_online_prune_info(self.h, w))
        return dict(stages=int(w[0]), removed=int(w[1]), carry=int(w[2]), max_excess=int(w[3]), flagged=int(w[4]),
                    downdate_bytes=int(w[5]) * 16384)

    def fit(self, learners, X, y, chunk=0):
        """refused: the replicas' learners map to ONE dictionary per slice, so their sample lists are not independent sequences
        (kb_fit answers RS_ESTATE); score() works.  Teach a per-replica VecKBRL and to_shared() it instead."""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'fit: shared-dictionary handles are not supported: several learners map to one '
                                 'dictionary (fit a per-replica VecKBRL, then to_shared)')

    def fit_steps(self, agents, state, action, labels, chunk=0):
        """refused, as fit() is and for its reason (kb_fit_steps answers RS_ESTATE): teach a per-replica VecKBRL from the log and
        to_shared() it instead"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'fit_steps: shared-dictionary handles are not supported: several learners map to '
                                 'one dictionary (teach a per-replica VecKBRL, then to_shared)')

    def set_fit_wide(self, min_landmarks, window=0):
        """refused, as kb_set_fit_wide refuses it: a shared-dictionary handle does not learn through fit()"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_fit_wide: a shared-dictionary handle does not learn through fit')

    def set_control_plus(self, on=True):
        """refused, as kb_set_control_plus refuses it: a shared-dictionary handle does not learn through update_control"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_control_plus: a shared-dictionary handle does not learn through update_control')

    def set_control_plus_batch(self, width, max_landmarks=1024):
        """refused, as kb_set_control_plus_batch refuses it"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_control_plus_batch: a shared-dictionary handle does not learn through update_control')

    def set_control_plus_wide(self, min_landmarks, max_landmarks=2048, rounds=32):
        """refused, as kb_set_control_plus_wide refuses it"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_control_plus_wide: a shared-dictionary handle does not learn through update_control')

    def set_fit_steps_batch(self, width, max_landmarks=1024):
        """refused, as kb_set_fit_steps_batch refuses it"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_fit_steps_batch: a shared-dictionary handle does not learn through fit_steps')

    def set_fit_wide_plus(self, on=True):
        """refused, as kb_set_fit_wide_plus refuses it: a shared-dictionary handle does not learn through fit()"""
        raise _lib.RanSliceError(_lib.RS_ESTATE, 'set_fit_wide_plus: a shared-dictionary handle does not learn through fit')

    @staticmethod
    def unique_id():
        """128 opaque bytes (ncclGetUniqueId) for comm_init; call on ONE rank"""
        buf = C.create_string_buffer(128)
        rc = _lib.load().kb_comm_unique_id(buf)
        if rc != 0:
            raise _lib.RanSliceError(rc, 'kb_comm_unique_id failed (librccl.so missing?)')
        return buf.raw

    def comm_info(self):
        """(rank, world) as the live RCCL communicator reports them; (0, 1) without one"""
        r, w = C.c_int(), C.c_int()
        self._check(self.L.kb_comm_info(self.h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_init(self, unique_id, rank, world):
        if self.cfg.first_env != rank * self.n_envs:
            raise ValueError('first_env must be rank * n_envs (contiguous replica shards)')
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self.L.kb_comm_init(self.h, buf, int(rank), int(world)))

    def share_from(self, src, agent, ctl_index=None):
        """the S dictionaries of this (shared, learning) handle := those of agent `agent` of the per-replica learning handle
        `src`, replica j's control state := that of src agent ctl_index[j] (default: `agent`) (kb_share); what VecKBRL.to_shared
        does into a handle it creates"""
        if ctl_index is not None:
            ctl_index = np.ascontiguousarray(ctl_index, dtype=np.int32)
            if ctl_index.shape != (self.n_envs,):
                raise ValueError('share_from: ctl_index must have n_envs = %d entries' % self.n_envs)
        if src.L is not self.L:
            raise RuntimeError('the two agents were created from different builds of libranslice')
        self._check(self.L.kb_share(self.h, src.h, int(agent), ctl_index.ctypes.data_as(_ip) if ctl_index is not None else None))

    def to_agents(self, index, capacity=None, pool_bytes=None, device=None):
        """-> a learning VecKBRL of len(index) agents (kb_unshare): each holds a private copy of the S shared dictionaries --
        landmarks, coefficients and Kinv bit for bit -- and the control state, tie-break stream, last observation and flags of
        replica index[j] of this handle.  From there every per-replica tool applies: .deploy(...), .export_agents(...),
        .prune(...), .fork_from(...), .set_learning(...), or learning on per replica.  capacity: the new handle's limit per
        dictionary (default: this handle's; at least its largest dictionary); pool_bytes: default fork_pool_bytes of the copied
        dictionaries plus room for each to grow by two shells; device: default this handle's (it must be the same one)."""
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
        if index.size == 0:
            raise ValueError('to_agents: index names no replica')
        capacity = self.capacity if capacity is None else int(capacity)
        if pool_bytes is None:
            sizes = np.tile(self.dictionary_sizes().astype(np.int64), (index.size, 1))
            pool_bytes = fork_pool_bytes(np.minimum(sizes + 128, max(capacity, 64)))
        cfg = self.cfg
        ag = VecKBRL(int(index.size), self.dims, self.n_prbs, alfa=cfg.alfa, accuracy_range=(cfg.acc_lo, cfg.acc_hi), gamma=cfg.gamma,
                     eta=cfg.eta, capacity=capacity, device=self.device if device is None else int(device), pool_bytes=int(pool_bytes))
        try:
            ag.unshare_from(self, index)
        except Exception:
            ag.close()
            raise
        return ag

    def shrink(self, target):
        """every shared dictionary above `target` landmarks is brought down to exactly `target` (kb_shared_prune): VecKBRL.prune's
        rule on this handle's own storage, in place -- one dictionary comes out bit for bit as prune() leaves its to_agents() copy.
        Control state, shells (pool()['used_bytes']) and the communicator stay; ranks that call it with the same target at the
        same step keep identical dictionaries.  Call it between steps, never inside a host-driven round.  pruned() and
        prune_times_ms() report it.  (prune() itself keeps refusing a shared handle.)  -> landmarks removed by the call"""
        n = C.c_uint64()
        self._check(self.L.kb_shared_prune(self.h, int(target), C.byref(n)))
        return int(n.value)

    def step_resident(self, env, count_rounds=False):
        """one closed-loop agent step on the device: the shared learning step on the simulator's buffers, then
        select_action into them (kb_shared_step_resident).  count_rounds: wait for the number of exchange rounds
        that had proposals (rounds_last); without it the host does not wait for the last permitted round at all"""
        self._same_library(env)
        if count_rounds:
            rounds = C.c_int32()
            self._check(self.L.kb_shared_step_resident(self.h, env.h, self.budget, self.max_rounds, C.byref(rounds)))
            self.rounds_last = rounds.value
        else:
            self._check(self.L.kb_shared_step_resident(self.h, env.h, self.budget, self.max_rounds, None))
            self.rounds_last = None

    def update_control(self, state, action, labels):
        state = np.ascontiguousarray(state, dtype=np.float32).reshape(self.n_envs, self.nv)
        action = np.ascontiguousarray(action, dtype=np.int32).reshape(self.n_envs, self.S)
        labels = np.ascontiguousarray(labels, dtype=np.int32).reshape(self.n_envs, self.S)
        hits = np.zeros((self.n_envs, self.S), dtype=np.int32)
        if self.exchange is None:
            rounds = C.c_int32()
            self._check(self.L.kb_shared_step(self.h, state.ctypes.data_as(_fp), action.ctypes.data_as(_ip),
                                              labels.ctypes.data_as(_ip), self.budget, self.max_rounds,
                                              hits.ctypes.data_as(_ip), C.byref(rounds)))
            self.rounds_last = rounds.value
            return hits
        counts = np.zeros(self.S, dtype=np.int32)
        props = np.zeros((self.S, self.budget, PROP_W))
        self.rounds_last = 0
        for rnd in range(self.max_rounds):
            first = rnd == 0
            self._check(self.L.kb_shared_scan(
                self.h, state.ctypes.data_as(_fp) if first else None, action.ctypes.data_as(_ip) if first else None,
                labels.ctypes.data_as(_ip) if first else None, rnd, self.budget, hits.ctypes.data_as(_ip),
                counts.ctypes.data_as(_ip), props.ctypes.data_as(_dp)))
            all_counts, all_props, me = self.exchange(counts, props)
            if int(np.asarray(all_counts).sum()) == 0:
                break
            mc, mp, taken = merge_proposals(all_counts, all_props, self.budget)
            mc = np.ascontiguousarray(mc, dtype=np.int32)
            mp = np.ascontiguousarray(mp, dtype=np.float64)
            self._check(self.L.kb_shared_apply(self.h, mc.ctypes.data_as(_ip), mp.ctypes.data_as(_dp), self.budget))
            acc = np.ascontiguousarray(taken[me], dtype=np.int32)
            self._check(self.L.kb_shared_commit(self.h, acc.ctypes.data_as(_ip)))
            self.rounds_last = rnd + 1
        if self.shared_online_prune:   # (only the caller of the host-driven rounds knows that the step's rounds are over)
            self._check(self.L.kb_shared_online_prune_stage(self.h))
        return hits
