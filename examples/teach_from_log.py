#!/usr/bin/env python3
"""Teach agents from a log of control steps, with the sample augmentation done on the device (VecKBRL.fit_steps).

1. A small fleet learns in the resident closed loop while (state, action, SLA labels) of every control step are logged --
   some 250 bytes per agent and step.  --teacher-algorithm projectron_plus makes that loop a Projectron++ loop
   (VecKBRL(..., control_plus=True)): a pupil taught from its log in the same algorithm ends with the teacher's sizes.
2. A fresh handle, in either algorithm, is taught from the log alone: fit_steps stages the log as it is and the kernel
   generates each step's up to n_prbs + 1 samples next to the loop that consumes them.  (In 'projectron' mode the sizes it
   reaches are printed beside the closed loop's: the two take the same decisions except within rounding of zero.)
3. The taught agents are deployed on a fresh fleet and stepped.

  python examples/teach_from_log.py --agents 8 --steps 40 --algorithm projectron_plus
  python examples/teach_from_log.py --agents 8 --steps 40 --algorithm projectron_plus --batch 8    # 8 candidates of a row per pass over Kinv
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'network-slicing_amd'))
import numpy as np  # noqa: E402
from ranslice.config import make_config  # noqa: E402
from ranslice.kbrl_dev import VecKBRL  # noqa: E402
from ranslice.vec_env import VecRanSlice, default_fading  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=8)
    ap.add_argument('--steps', type=int, default=40)
    ap.add_argument('--eval-steps', type=int, default=20)
    ap.add_argument('--scenario', type=int, default=0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--algorithm', choices=['projectron', 'projectron_plus'], default='projectron')
    ap.add_argument('--teacher-algorithm', choices=['projectron', 'projectron_plus'], default='projectron',
                    help='the rule of the closed loop that produces the log (projectron_plus turns set_control_plus on)')
    ap.add_argument('--batch', type=int, choices=[0, 2, 4, 8], default=0,
                    help="with --algorithm projectron_plus: that many candidates of a log row share one pass over Kinv "
                         '(VecKBRL.set_fit_steps_batch; same results)')
    a = ap.parse_args()
    if a.batch and a.algorithm != 'projectron_plus':
        ap.error('--batch groups the candidates of the projectron_plus rule: it needs --algorithm projectron_plus')
    cfg = make_config(a.scenario, n_envs=a.agents)
    dims, n_prbs, n = [10] * cfg.n_embb + [3] * cfg.n_mmtc, cfg.n_prbs, a.agents
    fading = default_fading()
    ia, sf = np.full((n, len(dims)), n_prbs // (2 * len(dims)), dtype=np.int32), np.full((n, len(dims)), 3, dtype=np.int32)

    # 1. the closed loop learns; the host keeps what update_control is given: the state an action was chosen in, the action, the labels
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=fading, seed=a.seed)
    teacher = VecKBRL(n, dims, n_prbs, capacity=1024, pool_bytes=256 << 20, algorithm=a.teacher_algorithm,
                      control_plus=a.teacher_algorithm == 'projectron_plus')
    teacher.reset(ia, sf)
    state = env.reset()
    env.enqueue_step(ia)
    log_state, log_action, log_labels = [], [], []
    for i in range(a.steps):
        f = env.fetch()                      # the step that executed f['actions'], chosen in `state`
        log_state.append(state)
        log_action.append(f['actions'])
        log_labels.append(f['labels'])
        teacher.step_resident(env)           # update_control(state, action, labels); select_action(f['obs'])
        state = f['obs']
        env.step_resident()
    teacher.synchronize()
    env.close()
    log = [np.stack(v, axis=1) for v in (log_state, log_action, log_labels)]     # [agents, steps, ...]
    print('logged %d steps of %d agents: %d bytes' % (a.steps, n, n * a.steps * (4 * sum(dims) + 8 * len(dims))))

    # 2. a fresh handle, taught from the log
    pupil = VecKBRL(n, dims, n_prbs, capacity=1024, pool_bytes=256 << 20, algorithm=a.algorithm, fit_steps_batch=a.batch)
    pupil.reset(ia, sf)
    out = pupil.fit_steps(np.arange(n), *log)
    w = pupil.fit_time_ms()
    print('fit_steps (%s): %d samples generated on the device, %d changed a dictionary, %d insertions'
          % (a.algorithm, w['samples'], w['mistakes'], w['insertions']))
    if a.batch:
        b = pupil.fit_steps_batch_work()
        print('groups of up to %d candidates: %d formed, %d skipped, %d passes over Kinv for %d columns of d*' % (a.batch, b[0], b[1], b[2], b[4]))
    print('agreement of the sign of f at the logged allocation with the label, last 10 steps: %.3f'
          % np.mean([(o[-10:] == l[-10:]).mean() for o, l in zip(out['y_at'], log[2])]))
    print('dictionary sizes of agent 0: taught from the log %s, the closed loop %s'
          % (pupil.dictionary_sizes()[0].tolist(), teacher.dictionary_sizes()[0].tolist()))
    teacher.close()

    # 3. deploy on a fresh fleet, and step
    deployed = pupil.deploy(np.arange(n, dtype=np.int32))
    fleet = VecRanSlice(n_envs=n, cfg=cfg, fading=fading, seed=a.seed + 1)
    fleet.reset()
    deployed.history_begin(a.eval_steps)
    fleet.enqueue_step(deployed.control(with_accuracies=False)['action'])
    for i in range(a.eval_steps - 1):
        deployed.step_resident(fleet)
        fleet.step_resident()
    deployed.step_resident(fleet)
    h = deployed.history_fetch()
    fleet.fetch()
    print('deployed for %d steps: mean reward %.3f, SLA violations per step %.3f'
          % (h['recorded'], h['reward'][:, :h['recorded']].mean(), h['violation'][:, :h['recorded']].mean()))
    for x in (fleet, deployed, pupil):
        x.close()


if __name__ == '__main__':
    main()
