"""VecReportWrapper: the reference's ReportWrapper interface (reference wrapper.py:24-138) over the batched
simulator -- float action simplex in, normalised observations out, per-replica history arrays.

  action  a in R^{S+1} (S slices + "unused")  ->  PRBs_i = floor(n_prbs * |a_i| / sum|a|)      (wrapper.py:77-82)
  obs                                          ->  clip(obs, -0.5, 1.5) - 0.5                   (wrapper.py:87-89)
  history: violation (int16), reward (float64), resources (int16) per step, saved as npz with the
  reference's keys (wrapper.py:120-123).
The mapping is elementwise host arithmetic on [N, S] arrays; the simulation itself stays on the GPU.
"""
import ctypes as C
import itertools

import numpy as np


def simplex_to_prbs(action, n_prbs, n_slices):
    """wrapper.py:77-82 for a batch [N, S+1] (or [N, S]: already integer PRBs, passed through)"""
    action = np.asarray(action)
    if action.shape[-1] > n_slices:
        a = np.abs(action.astype(np.float64))
        t = a.sum(axis=-1, keepdims=True)
        t = np.where(t == 0, 1.0, t)
        return np.floor(n_prbs * a[..., :n_slices] / t).astype(np.int32)
    return action.astype(np.int32)


def normalise_obs(obs):
    """wrapper.py:87-89"""
    return np.clip(obs, -0.5, 1.5) - 0.5


class VecReportWrapper:
    def __init__(self, env, steps=2000, control_steps=500, env_id=1, path='./logs/', verbose=False):
        self.env = env
        self.n_envs, self.n_slices, self.n_prbs = env.n_envs, env.n_slices, env.n_prbs
        self.n_variables = env.n_variables
        self.steps, self.control_steps, self.env_id, self.path, self.verbose = steps, control_steps, env_id, path, verbose
        self.file_path = '{}history_{}.npz'.format(path, env_id)
        self.step_counter = 0
        self.reset_history()

    def reset_history(self):
        self.violation_history = np.zeros((self.n_envs, self.steps), dtype=np.int16)
        self.reward_history = np.zeros((self.n_envs, self.steps), dtype=np.float64)
        self.action_history = np.zeros((self.n_envs, self.steps), dtype=np.int16)

    def reset(self, seeds=None):
        self.step_counter = 0
        self.obs = self.env.reset(seeds=seeds)
        return self.obs

    def step(self, action):
        prbs = simplex_to_prbs(action, self.n_prbs, self.n_slices)
        obs, reward, done, info = self.env.step(prbs)
        self.obs = normalise_obs(obs)
        if self.step_counter < self.steps:
            self.violation_history[:, self.step_counter] = info['total_violations']
            self.reward_history[:, self.step_counter] = reward
            self.action_history[:, self.step_counter] = prbs.sum(axis=1)
        self.step_counter += 1
        if self.step_counter % self.control_steps == 0:
            self.save_results()
        return self.obs, reward, done, {0: 0}

    def save_results(self):
        import os
        os.makedirs(self.path, exist_ok=True)
        np.savez(self.file_path, violation=self.violation_history, reward=self.reward_history,
                 resources=self.action_history)

    def set_evaluation(self, eval_steps, new_path=None, change_name=False):
        """wrapper.py:125-134"""
        self.step_counter = self.steps
        self.steps += eval_steps
        pad = [(0, 0), (0, eval_steps)]
        self.violation_history = np.pad(self.violation_history, pad)
        self.reward_history = np.pad(self.reward_history, pad)
        self.action_history = np.pad(self.action_history, pad)
        if new_path:
            self.path = new_path
        if change_name:
            self.file_path = '{}evaluation_{}.npz'.format(self.path, self.env_id)


def dqn_action_table(n_prbs, n_slices=2, granularity=2, max_prbs=51):
    """DQNWrapper's discrete actions (wrapper.py:140-149) for any number of slices: every tuple over
    range(0, max_prbs, granularity) in itertools.product order whose sum is at most n_prbs; int32 [n_actions, n_slices]"""
    levels = list(range(0, max_prbs, granularity))
    rows = [a for a in itertools.product(levels, repeat=n_slices) if sum(a) <= n_prbs]
    return np.array(rows, dtype=np.int32).reshape(len(rows), n_slices)


class DeviceReportWrapper:
    """VecReportWrapper with everything left on the device: step() takes a device array of float32 shares [N, S+1] (a
    DeviceArray, a torch tensor, ...) and returns DeviceArrays of the normalised observation and the reward; the simplex
    mapping, the normalisation and the three histories are done by the kernels around the step (rs_step_device,
    rs_report_*), bit for bit what VecReportWrapper computes on the host.  Only save_results() reads anything back.
    `stream`: the hipStream_t the caller's policy runs on (0: the null stream, torch's default)."""

    def __init__(self, env, steps=2000, control_steps=500, env_id=1, path='./logs/', verbose=False, stream=0):
        self.env = env
        self.n_envs, self.n_slices, self.n_prbs = env.n_envs, env.n_slices, env.n_prbs
        self.n_variables = env.n_variables
        self.steps, self.control_steps, self.env_id, self.path, self.verbose = steps, control_steps, env_id, path, verbose
        self.file_path = '{}history_{}.npz'.format(path, env_id)
        self.step_counter = 0
        self.stream = int(stream)
        self.view = env.device_view()
        self._done = np.zeros(self.n_envs, dtype=bool)
        self.reset_history()

    def reset_history(self):
        self.env._check(self.env.L.rs_report_begin(self.env.h, int(self.steps)))

    def reset(self, seeds=None):
        """returns the obs_norm DeviceArray.  Its memory holds the last step's normalised observation; the observation of
        a reset environment is all zeros (what VecReportWrapper.reset returns, un-normalised), so it is zeroed here."""
        self.step_counter = 0
        self.env.reset(seeds=seeds)
        self.obs = self.view['obs_norm']
        self.obs.set(np.zeros(self.obs.shape, dtype=np.float32))
        self.env.stream_join(self.stream)
        return self.obs

    def step(self, action):
        self.env.step_device(action, kind=1, stream=self.stream)
        self.step_counter += 1
        if self.step_counter % self.control_steps == 0:
            self.save_results()
        return self.obs, self.view['reward'], self._done, {0: 0}

    def histories(self):
        """(violation int16, reward float64, resources int16) [N, steps] from the device, and the columns recorded"""
        env = self.env
        v = np.zeros((self.n_envs, self.steps), dtype=np.int16)
        r = np.zeros((self.n_envs, self.steps), dtype=np.float64)
        a = np.zeros((self.n_envs, self.steps), dtype=np.int16)
        n = C.c_int32()
        sp = C.POINTER(C.c_int16)
        env._check(env.L.rs_report_fetch(env.h, v.ctypes.data_as(sp), r.ctypes.data_as(C.POINTER(C.c_double)),
                                         a.ctypes.data_as(sp), C.byref(n)))
        return v, r, a, int(n.value)

    def save_results(self):
        import os
        os.makedirs(self.path, exist_ok=True)
        v, r, a, _ = self.histories()
        np.savez(self.file_path, violation=v, reward=r, resources=a)

    def set_evaluation(self, eval_steps, new_path=None, change_name=False):
        """wrapper.py:125-134"""
        self.env._check(self.env.L.rs_report_extend(self.env.h, int(eval_steps)))
        self.step_counter = self.steps
        self.steps += eval_steps
        if new_path:
            self.path = new_path
        if change_name:
            self.file_path = '{}evaluation_{}.npz'.format(self.path, self.env_id)
