#!/usr/bin/env python3
"""A torch policy on the same GPU as the simulator, with nothing crossing PCIe inside the loop.

A fixed-seed MLP maps the normalised observation of every replica (the handle's own obs_norm buffer, wrapped in place
as a tensor) to ReportWrapper's action simplex; DeviceReportWrapper.step reads the shares tensor from device memory and
leaves observation, reward and the three histories on the device.  The host only enqueues; the histories are read
once, at the end, into history_<id>.npz (the reference's keys and dtypes).

  python examples/torch_device_policy.py --envs 4096 --steps 200
  python examples/torch_device_policy.py --envs 64 --steps 20 --check 20     # replay through VecReportWrapper on a twin

torch is imported BEFORE the simulator's library: a torch wheel brings a HIP runtime of its own, and a process must end
up with one runtime for both ("Device-resident policy interface").
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
import numpy as np  # noqa: E402
from ranslice.config import make_config  # noqa: E402
from ranslice.report import DeviceReportWrapper, VecReportWrapper  # noqa: E402
from ranslice.vec_env import VecRanSlice, default_fading  # noqa: E402


def make_policy(n_in, n_out, seed):
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(n_in, 64), torch.nn.Tanh(), torch.nn.Linear(64, n_out),
                              torch.nn.Softmax(dim=-1))
    return net.to('cuda').eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--envs', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--scenario', type=int, default=0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--check', type=int, default=0, help='replay the first K steps on a twin through VecReportWrapper')
    ap.add_argument('--fading', default=None, help='npz with t0, t1, t2 (default: the seeded synthetic traces)')
    ap.add_argument('--path', default='./logs/')
    a = ap.parse_args()
    if a.fading:
        g = np.load(a.fading)
        fading = [g['t0'], g['t1'], g['t2']]
    else:
        fading = default_fading()
    mk = lambda: VecRanSlice(n_envs=a.envs, cfg=make_config(a.scenario, n_envs=a.envs), fading=fading, seed=a.seed)
    env = mk()
    w = DeviceReportWrapper(env, steps=a.steps, control_steps=10 ** 9, env_id=1, path=a.path)
    obs = torch.as_tensor(w.reset(), device='cuda')          # the handle's obs_norm buffer, in place
    assert obs.data_ptr() == env.device_view()['obs_norm'].ptr
    policy = make_policy(env.n_variables, env.n_slices + 1, a.seed)
    keep = a.check > 0
    log = torch.empty((min(a.check, a.steps), a.envs, env.n_slices + 1), device='cuda') if keep else None
    with torch.no_grad():
        for i in range(a.steps):                             # nothing in this loop leaves the device or waits for it
            shares = policy(obs)
            if keep and i < a.check:
                log[i] = shares
            w.step(shares)
    w.save_results()
    v, r, res, n_rec = w.histories()
    print('%d replicas x %d steps: mean reward %.3f, violations per step %.4f, refused rows %d' %
          (a.envs, n_rec, r.mean(), v.mean(), env.rejected_rows()))
    if a.check:
        k = min(a.check, a.steps)
        host_shares = log.cpu().numpy()
        twin = mk()
        hw = VecReportWrapper(twin, steps=a.steps, control_steps=10 ** 9, env_id=2, path=a.path)
        hw.reset()
        for i in range(k):
            hw.step(host_shares[i])
        assert v[:, :k].tobytes() == hw.violation_history[:, :k].tobytes(), 'violation history differs'
        assert r[:, :k].tobytes() == hw.reward_history[:, :k].tobytes(), 'reward history differs'
        assert res[:, :k].tobytes() == hw.action_history[:, :k].tobytes(), 'resources history differs'
        print('check ok: %d steps equal the host wrapper on a twin' % k)
        twin.close()
    env.close()


if __name__ == '__main__':
    main()
