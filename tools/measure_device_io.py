#!/usr/bin/env python3
"""Per-step wall time of the two ReportWrapper paths under a fixed shares array, scenario 0:
  (a) VecReportWrapper.step     -- host numpy mapping, rs_step: actions up, obs / reward / labels / violations down, a wait;
  (b) DeviceReportWrapper.step  -- rs_step_device: shares read from device memory, everything left there (the stream is
                                   waited for once, after the last timed step).
Each (leg, replicas, repeat) runs in a child process of its own under `timeout`; the record holds the median of the
repeats.  Leg (a) uses nothing newer than VecReportWrapper, so `--tree DIR` runs it from another checkout (the parent
commit, built) and records that figure as the baseline beside this tree's.

  python tools/measure_device_io.py                        # writes profiles/device_io_record.json
  python tools/measure_device_io.py --tree ../parent       # the same, plus leg (a) from that checkout
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(leg, n, steps, burn, tree):
    sys.path.insert(0, os.path.join(tree, 'network-slicing_amd'))
    import numpy as np
    from ranslice.config import make_config
    from ranslice.fading import synth_fading
    from ranslice.vec_env import VecRanSlice
    from ranslice import report
    env = VecRanSlice(n_envs=n, cfg=make_config(0, n_envs=n), fading=[synth_fading(t, 10000) for t in range(3)])
    rng = np.random.default_rng(0)
    shares = rng.random((n, env.n_slices + 1)).astype(np.float32)
    if leg == 'host':
        w = report.VecReportWrapper(env, steps=steps, control_steps=10 ** 9, path='/tmp/')
        arg = shares
    else:
        w = report.DeviceReportWrapper(env, steps=steps, control_steps=10 ** 9, path='/tmp/')
        arg = env.device_view()['in_shares'].set(shares)
    w.reset()
    for i in range(burn):                                   # to the stationary population (tools/measure_host_path.py)
        env.random_actions(2024, i)
        env.step_resident()
    env.synchronize()
    for i in range(10):
        w.step(arg)
    env.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        w.step(arg)
    env.synchronize()
    t1 = time.perf_counter()
    print(json.dumps(dict(leg=leg, n_envs=n, steps=steps, ms_per_step=1e3 * (t1 - t0) / steps)))


def run(leg, n, steps, burn, tree, limit):
    cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--child', leg, '--envs', str(n),
           '--steps', str(steps), '--burn', str(burn), '--tree', tree]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])['ms_per_step']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--envs', type=int, nargs='*', default=[4096, 65536])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--burn', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--tree', default=None, help='another built checkout to take the baseline of leg (a) from')
    ap.add_argument('--timeout', type=int, default=240)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'device_io_record.json'))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.envs[0], a.steps, a.burn, a.tree or ROOT)
    rec = dict(scenario=0, timed_steps=a.steps, burn_in_steps=a.burn, repeats=a.repeats, statistic='median', rows=[])
    for n in a.envs:
        row = dict(n_envs=n)
        legs = [('host_ms_per_step', 'host', ROOT), ('device_ms_per_step', 'device', ROOT)]
        if a.tree:
            legs.insert(0, ('host_ms_per_step_baseline_tree', 'host', os.path.abspath(a.tree)))
        for key, leg, tree in legs:
            xs = [run(leg, n, a.steps, a.burn, tree, a.timeout) for _ in range(a.repeats)]
            row[key] = statistics.median(xs)
            row[key + '_runs'] = xs
        row['host_over_device'] = row['host_ms_per_step'] / row['device_ms_per_step']
        rec['rows'].append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
