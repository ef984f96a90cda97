"""VecRanSlice: N independent RanSlice environments advanced together on one MI355X.

This is the batched form of the reference's gym surface (reference
gym-ran_slice/gym_ran_slice/ran_slice.py:15-54): `reset()` and `step(actions)` with a leading
replica axis.  `gym_ran_slice.RanSlice` is its N=1 view.  All simulation runs in the HIP kernels
behind libranslice.so; this module only moves numpy buffers across the C ABI.
"""
import ctypes as C

import numpy as np

from . import _lib
from .config import RsAllocRec, make_config, n_vars
from .device_io import DeviceArray, describe
from .fading import synth_fading
from .sharding import replica_seeds

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)
_up = C.POINTER(C.c_uint64)


def default_fading(n_cols=10000, seed=20240):
    """The build's seeded stand-in for the three absent ns-3 traces."""
    return [synth_fading(t, n_cols, seed=seed) for t in range(3)]


class VecRanSlice:
    def __init__(self, n_envs=1, scenario=0, seed=0, device=0, fading=None, cfg=None, **cfg_kw):
        self.L = _lib.load()
        self.cfg = cfg if cfg is not None else make_config(scenario, n_envs=n_envs, **cfg_kw)
        self.cfg.n_envs = n_envs
        self.n_envs = n_envs
        self.n_ran = self.cfg.n_embb + self.cfg.n_mmtc
        # action / label entries per replica: one per L1 slice (with L1_level=False all eMBB RAN slices share one L1
        # slice and all mMTC ones another, scenario_creator.py:168-177)
        self.multiplexed = bool(self.cfg.l1_multiplex)
        self.n_slices = ((self.cfg.n_embb > 0) + (self.cfg.n_mmtc > 0)) if self.multiplexed else self.n_ran
        self.n_variables = n_vars(self.cfg)
        self.n_prbs = self.cfg.n_prbs
        self.penalty = self.cfg.penalty
        self.device = int(device)
        self.h = C.c_void_p()
        rc = self.L.rs_create(C.byref(self.cfg), int(device), C.byref(self.h))
        self._check(rc)
        if self.cfg.n_embb > 0:
            if fading is None:
                fading = default_fading()
            for t, tab in enumerate(fading):
                tab = np.ascontiguousarray(tab, dtype=np.float64)
                self._check(self.L.rs_load_fading(self.h, t, tab.ctypes.data_as(_dp), tab.shape[0], tab.shape[1]))
        self.base_seed = int(seed)
        self._obs = np.zeros((n_envs, self.n_variables), dtype=np.float32)
        self._reward = np.zeros(n_envs, dtype=np.float64)
        self._labels = np.zeros((n_envs, self.n_slices), dtype=np.int32)
        self._viol = np.zeros((n_envs, self.n_slices), dtype=np.int32)

    def _check(self, rc):
        if rc != 0:
            msg = self.L.rs_last_error(self.h).decode() if self.h else 'rs_create failed'
            raise _lib.RanSliceError(rc, msg)

    def close(self):
        if getattr(self, 'h', None):
            self.L.rs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- gym-like surface -------------------------------------------------------------
    def reset(self, seeds=None):
        """seeds: per-replica 64-bit stream seeds; default sharding.replica_seeds(base_seed, 0, n_envs), a mix of
        the batch seed and the replica index (the reference seeds run i with default_rng(seed=i),
        experiments_kbrl.py:46)."""
        if seeds is None:
            seeds = replica_seeds(self.base_seed, 0, self.n_envs)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        assert seeds.shape == (self.n_envs,)
        self._check(self.L.rs_reset(self.h, seeds.ctypes.data_as(_up), self._obs.ctypes.data_as(_fp)))
        return self._obs.copy()

    def step(self, actions):
        actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.n_envs, self.n_slices)
        self._check(self.L.rs_step(self.h, actions.ctypes.data_as(_ip), self._obs.ctypes.data_as(_fp),
                                   self._reward.ctypes.data_as(_dp), self._labels.ctypes.data_as(_ip),
                                   self._viol.ctypes.data_as(_ip)))
        info = {'SLA_labels': self._labels.copy(), 'violations': self._viol.copy(),
                'total_violations': self._viol.sum(axis=1), 'n_prbs': actions.copy()}
        return self._obs.copy(), self._reward.copy(), np.zeros(self.n_envs, dtype=bool), info

    def enqueue_step(self, actions):
        """step(actions) without reading anything back: the outputs stay on the device for step_resident / VecKBRL.step_resident
        (the first step of a closed loop, taken under the agents' initial or last selected action)"""
        actions = np.ascontiguousarray(actions, dtype=np.int32).reshape(self.n_envs, self.n_slices)
        self._check(self.L.rs_step(self.h, actions.ctypes.data_as(_ip), None, None, None, None))

    # ---- device-resident path (bench) --------------------------------------------------
    def random_actions(self, seed, step_index):
        self._check(self.L.rs_random_actions(self.h, int(seed), int(step_index)))

    def step_resident(self):
        self._check(self.L.rs_step_resident(self.h))

    def run_random(self, seed, step_index0, n_steps, graph=False):
        """n_steps x (random_actions(seed, step_index0 + i); step_resident()) enqueued by one call; with
        graph=True the loop body is replayed from a captured hipGraph (same results)."""
        self._check(self.L.rs_run_random(self.h, int(seed), int(step_index0), int(n_steps), 1 if graph else 0))

    def fetch(self):
        actions = np.zeros((self.n_envs, self.n_slices), dtype=np.int32)
        self._check(self.L.rs_fetch(self.h, actions.ctypes.data_as(_ip), self._obs.ctypes.data_as(_fp),
                                    self._reward.ctypes.data_as(_dp), self._labels.ctypes.data_as(_ip),
                                    self._viol.ctypes.data_as(_ip)))
        return dict(actions=actions, obs=self._obs.copy(), reward=self._reward.copy(),
                    labels=self._labels.copy(), violations=self._viol.copy())

    def save_state(self):
        """the handle's whole state as one uint8 array (rs_save_state): feed it to load_state of a handle of the same
        configuration -- this one later, or a fresh one in another process -- and the run goes on bit for bit"""
        n = C.c_uint64()
        self._check(self.L.rs_state_bytes(self.h, C.byref(n)))
        blob = np.empty(n.value, dtype=np.uint8)
        self._check(self.L.rs_save_state(self.h, blob.ctypes.data_as(C.c_void_p), n.value))
        return blob

    def load_state(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self.L.rs_load_state(self.h, blob.ctypes.data_as(C.c_void_p), blob.size))

    def synchronize(self):
        self._check(self.L.rs_synchronize(self.h))

    # ---- device-resident policy interface (rs_policy_io.hip) ---------------------------------
    def device_view(self):
        """dict of DeviceArrays over the handle's own device buffers (rs_get_device_view), valid until close(): the inputs
        in_prbs / in_shares / in_index, the executed `actions` and their row sums `resources`, and the outputs of the last step
        obs, obs_norm, reward, labels, violations, total_violations; `rejected` is the one-word refusal counter.  Also
        'stream': the handle's hipStream_t as an int."""
        v = _lib.RsDeviceView()
        self._check(self.L.rs_get_device_view(self.h, C.byref(v)))
        N, S, V = self.n_envs, self.n_slices, self.n_variables
        spec = dict(in_prbs=((N, S), np.int32), in_shares=((N, S + 1), np.float32), in_index=((N,), np.int64),
                    actions=((N, S), np.int32), resources=((N,), np.int32), obs=((N, V), np.float32),
                    obs_norm=((N, V), np.float32), reward=((N,), np.float64), labels=((N, S), np.int32),
                    violations=((N, S), np.int32), total_violations=((N,), np.int32), rejected=((1,), np.int64))
        out = {k: DeviceArray(getattr(v, k), shape, dt, owner=self) for k, (shape, dt) in spec.items()}
        out['stream'] = int(v.stream or 0)
        return out

    def _action_kind(self, shape, dtype):
        N, S = self.n_envs, self.n_slices
        if dtype == np.int32 and shape in ((N, S), (N * S,)):
            return _lib.RS_ACT_PRBS
        if dtype == np.float32 and shape in ((N, S + 1), (N * (S + 1),)):
            return _lib.RS_ACT_SHARES
        if dtype == np.int64 and shape in ((N,), (N, 1)):
            return _lib.RS_ACT_INDEX
        raise ValueError('step_device: %s %s fits no action kind (int32 [%d, %d] PRBs, float32 [%d, %d] shares, int64 [%d] '
                         'table rows)' % (dtype, shape, N, S, N, S + 1, N))

    def step_device(self, actions, kind=None, stream=0):
        """One step with the actions read from device memory and every output left there (rs_step_device): nothing crosses
        PCIe and the host does not wait.  actions: a DeviceArray, anything with __cuda_array_interface__ or data_ptr() (a torch
        tensor), or an int device pointer (then `kind` is required).  kind: RS_ACT_PRBS / RS_ACT_SHARES / RS_ACT_INDEX, inferred
        from dtype and shape when None.  stream: the hipStream_t (int) the actions were produced on and the outputs will be
        read on; 0 is the null stream, torch's default.  Rows that rs_step would reject are replaced by zeros and counted
        (rejected_rows)."""
        ptr, shape, dtype = describe(actions)
        if shape is not None and dtype is not None:
            fits = self._action_kind(shape, dtype)
            if kind is None:
                kind = fits
            elif int(kind) != fits:
                raise ValueError('step_device: %s %s is not the layout of action kind %d' % (dtype, shape, int(kind)))
        elif kind is None:
            raise ValueError('step_device: a bare pointer needs an explicit kind')
        self._check(self.L.rs_step_device(self.h, int(kind), C.c_void_p(ptr), C.c_void_p(int(stream) or None)))

    def stream_join(self, stream=0):
        """`stream` waits for everything queued on the handle so far (rs_stream_join); the host does not"""
        self._check(self.L.rs_stream_join(self.h, C.c_void_p(int(stream) or None)))

    def set_action_table(self, table):
        """the rows RS_ACT_INDEX picks from: int [n_actions, n_slices] (report.dqn_action_table)"""
        table = np.ascontiguousarray(table, dtype=np.int32)
        if table.ndim != 2 or table.shape[1] != self.n_slices or table.shape[0] == 0:
            raise ValueError('set_action_table: expected [n_actions, %d], got %s' % (self.n_slices, table.shape))
        self._check(self.L.rs_set_action_table(self.h, table.ctypes.data_as(_ip), table.shape[0]))

    def rejected_rows(self):
        """action rows step_device refused since reset(); waits for the handle's stream"""
        return int(self.device_view()['rejected'].get()[0])

    # ---- replica fork and the clairvoyant step -------------------------------------------
    def fork_from(self, src, index):
        """replica j of this env := replica index[j] of `src` (rs_fork): a VecRanSlice of the same configuration but n_envs,
        the same fading tables and device, reset.  This env takes src's clock; stepping replica j with action a gives, bit for
        bit, what stepping src replica index[j] with a would.  Enqueued on the device; the host does not wait."""
        index = np.ascontiguousarray(index, dtype=np.int32)
        if index.shape != (self.n_envs,):
            raise ValueError('fork_from: index must have n_envs = %d entries' % self.n_envs)
        self._check(self.L.rs_fork(self.h, src.h, index.ctypes.data_as(_ip)))

    def set_lookahead(self, max_branches=None):
        """capacity of the clairvoyant search: forked replicas per search launch (0 frees the branch handle).  Default: as
        many as a quarter of the free device memory holds at this env's bytes per replica, at most what one launch for the
        whole batch needs (n_envs x (n_prbs + 1)), at least n_prbs + 1."""
        if max_branches is None:
            n = C.c_uint64()
            self._check(self.L.rs_state_bytes(self.h, C.byref(n)))
            per_replica = max(1, n.value // self.n_envs)
            free, _ = _lib.device_mem_info(self.device)
            cand = self.n_prbs + 1
            max_branches = int(min(self.n_envs * cand, max(cand, (free // 4) // per_replica)))
        self._check(self.L.rs_set_lookahead(self.h, int(max_branches)))
        self._lookahead = int(max_branches)

    def set_clairvoyant_fallback(self, mode):
        """what a slice with no SLA-meeting candidate gets: 'cheapest' (0, default) or 'widest' (1) of the least-violating"""
        mode = {'cheapest': 0, 'widest': 1}.get(mode, mode)
        self._check(self.L.rs_set_clairvoyant_fallback(self.h, int(mode)))

    def step_clairvoyant(self):
        """one step of every replica under the clairvoyant rule (rs_step_clairvoyant): per replica, slice by slice, the
        cheapest allocation that meets the SLA in a fork stepped once (else the cheapest least-violating one), then the
        real step.  Returns (actions, obs, reward, labels, violations)."""
        if not getattr(self, '_lookahead', 0):
            self.set_lookahead()
        actions = np.zeros((self.n_envs, self.n_slices), dtype=np.int32)
        self._check(self.L.rs_step_clairvoyant(self.h, actions.ctypes.data_as(_ip), self._obs.ctypes.data_as(_fp),
                                               self._reward.ctypes.data_as(_dp), self._labels.ctypes.data_as(_ip),
                                               self._viol.ctypes.data_as(_ip)))
        return actions, self._obs.copy(), self._reward.copy(), self._labels.copy(), self._viol.copy()

    # ---- introspection ------------------------------------------------------------------
    def l1_info(self):
        info = np.zeros((self.n_envs, self.n_ran, 10), dtype=np.float64)   # one row per RAN slice
        self._check(self.L.rs_get_info(self.h, info.ctypes.data_as(_dp)))
        return info

    def set_group_size(self, lanes):
        """lanes per task of the primary step launch (8, 16, 32); results do not depend on it"""
        self._check(self.L.rs_set_group_size(self.h, int(lanes)))

    def set_lanes(self, n):
        """lanes of the step loop (rs_set_lanes): 0 automatic, 1 off, n >= 2 that many replica ranges stepped on streams of
        their own by random_actions / step_resident / run_random, not joined between steps; same results"""
        self._check(self.L.rs_set_lanes(self.h, int(n)))

    def lane_info(self):
        """(lanes in use, sum of the lanes' step-kernel times per step in ms, union of their intervals per step in ms,
        1 - union / sum) over the last window of kernel timing (rs_get_lane_info)"""
        out = (C.c_double * 4)()
        self._check(self.L.rs_get_lane_info(self.h, out))
        return int(out[0]), out[1], out[2], out[3]

    def set_schedule_hint(self, mode):
        """1: allocations are agent-made (few wide slices), 0: plain instance, -1: automatic; same results"""
        self._check(self.L.rs_set_schedule_hint(self.h, int(mode)))

    def set_alloc_trace(self, enable=True):
        self._check(self.L.rs_set_alloc_trace(self.h, int(bool(enable))))

    def alloc_trace(self):
        shape = ((self.n_envs, self.cfg.slots_per_step, 64) if self.multiplexed   # the one shared UE list; type >> 8 = RAN slice
                 else (self.n_envs, self.cfg.n_embb, self.cfg.slots_per_step, 32))
        tr = np.zeros(shape, dtype=np.dtype(RsAllocRec))
        self._check(self.L.rs_get_alloc_trace(self.h, tr.ctypes.data_as(C.c_void_p)))
        return tr

    def counters(self):
        c = (C.c_uint64 * 4)()
        self._check(self.L.rs_get_counters(self.h, c))
        return [int(x) for x in c]

    def rx_stats(self):
        """(reception tests, of which evaluated the exact probability, short test available) since reset()"""
        c = (C.c_uint64 * 3)()
        self._check(self.L.rs_get_rx_stats(self.h, c))
        return int(c[0]), int(c[1]), bool(c[2])

    def set_kernel_timing(self, enable=True):
        self._check(self.L.rs_set_kernel_timing(self.h, int(bool(enable))))

    def kernel_time_stats_ms(self):
        """((mean, min, max) ms of the dominant step kernel over the launches since the last call, launches)"""
        st = (C.c_double * 3)()
        n = C.c_int64()
        self._check(self.L.rs_kernel_time_stats_ms(self.h, st, C.byref(n)))
        return (st[0], st[1], st[2]), n.value

    def kernel_time_ms(self):
        ms = C.c_double()
        n = C.c_int64()
        self._check(self.L.rs_kernel_time_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value
