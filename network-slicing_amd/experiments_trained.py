#!/usr/bin/env python3
"""The paper's "inference phase" (the reference's plot_trained_results.py: steps 40,000-49,500 of the training runs) done the
way a trained agent is used: train, freeze, fan out, evaluate.

For each (scenario, accuracy range):
  1. train --runs KBRL agents for --train-steps steps, run i as replica i of one VecRanSlice + VecKBRL pair (the machinery of
     experiments_kbrl.BatchedEvaluator: same seeds, same device-resident loop);
  2. deploy every trained agent --eval-replicas times (VecKBRL.deploy: landmarks and coefficients only, learning off) against
     fresh environment seeds -- one VecRanSlice of runs x eval-replicas replicas;
  3. run --eval-steps closed-loop steps in inference mode with the histories on the device;
  4. write results/scenario_N/KBRL_xx_deployed/evaluation_K.npz per trained run K: violation, resources (int16) and reward
     (float64), [eval_replicas, eval_steps] -- the keys and dtypes of ranslice.report.VecReportWrapper;
  5. print mean violations per stage and mean resource occupation with the 95 % t-interval of plot_trained_results.py over the
     trained agents (each agent's figure is the mean over its replicas), next to the same two numbers from the training runs'
     own last window -- the reference's method: one trajectory per agent, the agent still learning in the window.

  python experiments_trained.py [--scenarios 0] [--runs 30] [--train-steps 40000] [--eval-replicas 64] [--eval-steps 9500]
                                [--learning-control] [--save-agents DIR | --load-agents DIR]

--save-agents DIR writes the trained agents of every cell to DIR/scenario_N_KBRL_xx.kbagent (an agent file: landmarks,
coefficients and control state, ranslice.agent_file) right after training; --load-agents DIR skips step 1 and evaluates the
fleet from that file -- in another process, on another day -- with the evaluation arrays of steps 2-4 equal number for number.
--load-agents DIR --learning-control runs the control leg from the file as well: the agents come back as LEARNING agents
(VecKBRL.load_agents(blob, index, learning=True): Kinv is rebuilt on the device) and go on learning on the fleet.
"""
import argparse
import os
import time
from itertools import product

import numpy as np
from numpy.random import default_rng

import scenario_creator as sc
from experiments_kbrl import BatchedEvaluator, CHUNK, GRAPH, accuracy_list, name

RUNS = 30
TRAIN_STEPS = 40000
EVAL_REPLICAS = 64
EVAL_STEPS = 9500
EVAL_SEED0 = 1 << 20   # evaluation replica j is seeded as run EVAL_SEED0 + j would be: disjoint from the training runs' seeds


def mean_confidence_radius(data, confidence=0.95):
    """(mean, half-width of the two-sided Student-t interval) of a sample -- the figure plot_trained_results.py draws its
    error bars from: t quantile at n - 1 degrees of freedom times the standard error of the mean"""
    from scipy.stats import t as student_t
    x = np.asarray(data, dtype=np.float64).ravel()
    n = x.size
    radius = student_t.ppf(0.5 + confidence / 2.0, df=n - 1) * x.std(ddof=1) / np.sqrt(n)
    return float(x.mean()), float(radius)


def window_statistics(violation, resources, n_prbs, start=0, end=None, confidence=0.95):
    """violation, resources: [agents, steps] (a trajectory per agent) or [agents, replicas, steps] (several per agent, averaged
    first).  -> dict(violations=(mean, radius), occupation=(mean, radius)) over the agents, of the per-agent means over
    steps start:end -- violations per stage, and resources / n_prbs (plot_trained_results.py:57-62)."""
    v = np.asarray(violation, dtype=np.float64)[..., start:end]
    r = np.asarray(resources, dtype=np.float64)[..., start:end]
    per_agent_v = v.reshape(v.shape[0], -1).mean(axis=1)
    per_agent_r = r.reshape(r.shape[0], -1).mean(axis=1) / n_prbs
    return dict(violations=mean_confidence_radius(per_agent_v, confidence), occupation=mean_confidence_radius(per_agent_r, confidence))


def eval_seeds(n):
    return np.array([int(default_rng(seed=EVAL_SEED0 + j).integers(0, 2 ** 63 - 1)) for j in range(n)], dtype=np.uint64)


def _fleet_run(agent, scenario, n_replicas, eval_steps, device, graph):
    """`agent` (one per replica) steers a fresh fleet of n_replicas environments for eval_steps closed-loop steps, the first one
    under the action the agents last selected; -> the histories.  The fleet's seeds depend on its size alone, so two agents
    handles run against the same traffic realisations."""
    from ranslice import config as _c
    from ranslice.vec_env import VecRanSlice, default_fading
    fading = sc._FADING if sc._FADING is not None else default_fading()
    fleet = VecRanSlice(n_envs=n_replicas, cfg=_c.make_config(scenario, n_envs=n_replicas), fading=fading, device=device)
    fleet.reset(seeds=eval_seeds(n_replicas))
    agent.history_begin(eval_steps)
    fleet.enqueue_step(agent.control(with_accuracies=False)['action'])
    for i in range(0, eval_steps - 1, CHUNK):
        agent.run_resident(fleet, min(CHUNK, eval_steps - 1 - i), graph=graph)
    agent.step_resident(fleet)
    h = agent.history_fetch()
    fleet.fetch()        # surfaces simulator capacity errors
    fleet.close()
    assert h['recorded'] == eval_steps
    return h


def agents_path(directory, scenario, a_range):
    """the agent file of one (scenario, accuracy range) under --save-agents / --load-agents"""
    return os.path.join(directory, 'scenario_{}_{}_{}.kbagent'.format(scenario, name, int(a_range[0] * 100)))


def _write_evaluation(h, scenario, a_range, runs, R, eval_steps, out_dir):
    """the fleet's histories -> one evaluation_K.npz per trained run; -> (path, violation, resources [n, R, steps], statistics)"""
    path = '{}/scenario_{}/{}_{}_deployed/'.format(out_dir, scenario, name, int(a_range[0] * 100))
    os.makedirs(path, exist_ok=True)
    shape = (len(runs), R, eval_steps)
    viol, res, rew = h['violation'].reshape(shape), h['resources'].reshape(shape), h['reward'].reshape(shape)
    for k, i in enumerate(runs):
        np.savez('{}evaluation_{}.npz'.format(path, i), violation=viol[k], resources=res[k], reward=rew[k])
    return path, viol, res, window_statistics(viol, res, sc.scenarios[scenario]['n_prbs'])


def _evaluate_loaded(scenario, a_range, runs, R, eval_steps, out_dir, device, graph, verbose, by_reference, directory,
                     learning_control=False, pool_bytes=32 << 30, algorithm='projectron', control_plus_batch=0,
                     control_plus_wide=0):
    """steps 2-4 of a cell whose agents come from their file: agent k of the file is trained run runs[k].  learning_control: the
    same agents loaded once more with learning left on (their Kinv rebuilt on the device), against the same fleet"""
    from ranslice import agent_file
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    n = len(runs)
    if control_plus_wide and not (control_plus_batch and algorithm == 'projectron_plus'):
        raise ValueError('control_plus_wide needs a control_plus_batch width and the projectron_plus algorithm')
    t1 = time.perf_counter()
    with open(agents_path(directory, scenario, a_range), 'rb') as f:
        blob = f.read()
    sizes = agent_file.info(blob)['m']
    if sizes.shape[0] != n:
        raise ValueError('{} holds {} agents, the cell has {} runs'.format(agents_path(directory, scenario, a_range), sizes.shape[0], n))
    index = np.repeat(np.arange(n, dtype=np.int32), R)
    deployed = VecKBRL.load_agents(blob, index, by_reference=by_reference, device=device)
    pool = deployed.pool()
    h = _fleet_run(deployed, scenario, n * R, eval_steps, device, graph)
    t_eval = time.perf_counter() - t1
    deployed.close()
    path, viol, res, dep = _write_evaluation(h, scenario, a_range, runs, R, eval_steps, out_dir)
    lc = None
    if learning_control:
        t2 = time.perf_counter()
        control = VecKBRL.load_agents(blob, index, device=device, learning=True, pool_bytes=fork_pool_bytes(sizes[index]) + pool_bytes)
        if algorithm != 'projectron':   # (neither the algorithm nor the switch is in an agent file)
            control.set_algorithm(algorithm)
            control.set_control_plus(True)
            control.set_control_plus_batch(control_plus_batch)
            if control_plus_wide:
                control.set_control_plus_wide(control_plus_wide, min(2048, control.capacity // 64 * 64))
        rebuilt = control.rebuild_stats()
        hc = _fleet_run(control, scenario, n * R, eval_steps, device, graph)
        shape = (n, R, eval_steps)
        lc = dict(window_statistics(hc['violation'].reshape(shape), hc['resources'].reshape(shape), sc.scenarios[scenario]['n_prbs']),
                  wall_s=time.perf_counter() - t2, pool=control.pool(), rebuild_rounds=rebuilt['rounds'],
                  rebuild_min_delta=float(rebuilt['min_delta'].min()))
        control.close()
    if verbose:
        fmt = '{:.4f} +- {:.4f}'
        print('scenario {} KBRL {}: {} agents loaded from their file, {} replicas each for {} steps in inference mode ({:.1f} s)'
              .format(scenario, a_range[0], n, R, eval_steps, t_eval))
        print('  deployed (frozen, {} unseen traffic realisations per agent): violations per stage {}, resource occupation {}'
              .format(R, fmt.format(*dep['violations']), fmt.format(*dep['occupation'])))
        if lc is not None:
            print('  the same agents on the same fleet with learning left on (loaded with Kinv rebuilt): violations per stage {}, resource '
                  'occupation {}'.format(fmt.format(*lc['violations']), fmt.format(*lc['occupation'])))
    out = dict(scenario=scenario, accuracy_range=list(a_range), runs=n, train_steps=None, eval_replicas=R, eval_steps=eval_steps,
               window=None, train_wall_s=0.0, eval_wall_s=t_eval, deployed=dep, training_window=None, max_dictionary=int(sizes.max()),
               mean_dictionary=float(sizes.mean()), deployed_pool_bytes=int(pool['used_bytes']), by_reference=bool(by_reference),
               path=path, loaded=True)
    if lc is not None:
        out['learning_control'] = lc
    return out


def train_and_deploy(scenario, a_range, runs=range(RUNS), train_steps=TRAIN_STEPS, eval_replicas=EVAL_REPLICAS, eval_steps=EVAL_STEPS,
                     out_dir='./results', device=0, capacity=16384, pool_bytes=32 << 30, graph=GRAPH, verbose=True,
                     learning_control=False, by_reference=False, save_agents=None, load_agents=None, algorithm='projectron',
                     control_plus_batch=0, control_plus_wide=0):
    """one (scenario, accuracy range): writes the evaluation files and returns a summary with both pairs of numbers.
    learning_control: also run FULL forks of the same agents, learning left on, against the same fresh fleet -- what separates
    "the agent is frozen" from "the environment is new" in the difference between the two pairs (summary['learning_control'];
    no files).  by_reference: the fleet shares each agent's dictionaries (VecKBRL.deploy(index, by_reference=True)): the pool is
    the trained agents', not the replicas'; the results are the copy's bit for bit.
    save_agents / load_agents: a directory; the cell's agent file (agents_path) is written after training, or read INSTEAD of
    training -- the evaluation arrays are the same either way (summary['training_window'] is None for a loaded cell; its
    learning_control leg loads the agents with their Kinv rebuilt, which continues exactly as full forks of the trained handle
    would).
    algorithm='projectron_plus': the agents train, and the learning_control leg goes on learning, by ProjectronPlus's margin rule
    in the closed loop (VecKBRL.set_control_plus); the deployed leg only selects and is indifferent to it.
    control_plus_batch = 2, 4 or 8: in that mode that many candidates of a step share one pass over Kinv (same results).
    control_plus_wide = M (with a control_plus_batch width): learners of M landmarks or more have their passes over Kinv spread over
    the chip (same results)."""
    from ranslice.kbrl_dev import VecKBRL, fork_pool_bytes
    runs = list(runs)
    n, R = len(runs), int(eval_replicas)
    n_prbs = sc.scenarios[scenario]['n_prbs']
    if load_agents is not None:
        return _evaluate_loaded(scenario, a_range, runs, R, eval_steps, out_dir, device, graph, verbose, by_reference, load_agents,
                                learning_control=learning_control, pool_bytes=pool_bytes, algorithm=algorithm,
                                control_plus_batch=control_plus_batch, control_plus_wide=control_plus_wide)
    if control_plus_wide and not (control_plus_batch and algorithm == 'projectron_plus'):
        raise ValueError('control_plus_wide needs a control_plus_batch width and the projectron_plus algorithm')
    t0 = time.perf_counter()
    ev = BatchedEvaluator(scenario, a_range, steps=train_steps, out_dir=out_dir, algorithm=algorithm,
                          control_plus_batch=control_plus_batch if algorithm == 'projectron_plus' else 0,
                          control_plus_wide=control_plus_wide if algorithm == 'projectron_plus' else 0)
    agent, env = ev.train(runs, device=device, capacity=capacity, pool_bytes=pool_bytes, graph=graph)
    hist = agent.history_fetch()
    assert hist['recorded'] == train_steps
    env.fetch()
    window = min(eval_steps, train_steps)
    trained = window_statistics(hist['violation'], hist['resources'], n_prbs, start=train_steps - window)
    sizes = agent.dictionary_sizes()
    t_train = time.perf_counter() - t0
    if save_agents is not None:
        os.makedirs(save_agents, exist_ok=True)
        with open(agents_path(save_agents, scenario, a_range), 'wb') as f:
            f.write(agent.export_agents(np.arange(n, dtype=np.int32)))
    # freeze and fan out: replicas k * R .. k * R + R - 1 carry trained run k
    t1 = time.perf_counter()
    index = np.repeat(np.arange(n, dtype=np.int32), R)
    deployed = agent.deploy(index, by_reference=by_reference)
    pool = deployed.pool()
    control = None
    if learning_control:
        control = VecKBRL(n * R, agent.dims, agent.n_prbs, alfa=sc.alfa, accuracy_range=tuple(a_range), capacity=capacity,
                          device=device, pool_bytes=fork_pool_bytes(sizes[index]) + pool_bytes,
                          **(dict(algorithm=algorithm, control_plus=True, control_plus_batch=control_plus_batch,
                                  control_plus_wide=control_plus_wide, control_plus_wide_max=min(2048, capacity // 64 * 64))
                             if algorithm != 'projectron' else {}))
        control.fork_from(agent, index)
        control.synchronize()
    ev.release()
    h = _fleet_run(deployed, scenario, n * R, eval_steps, device, graph)
    t_eval = time.perf_counter() - t1
    deployed.close()
    path, viol, res, dep = _write_evaluation(h, scenario, a_range, runs, R, eval_steps, out_dir)
    shape = (n, R, eval_steps)
    summary = dict(scenario=scenario, accuracy_range=list(a_range), runs=n, train_steps=train_steps, eval_replicas=R,
                   eval_steps=eval_steps, window=window, train_wall_s=t_train, eval_wall_s=t_eval, deployed=dep, training_window=trained,
                   max_dictionary=int(sizes.max()), mean_dictionary=float(sizes.mean()), deployed_pool_bytes=int(pool['used_bytes']),
                   by_reference=bool(by_reference), path=path)
    fmt = '{:.4f} +- {:.4f}'
    if verbose:
        print('scenario {} KBRL {}: {} agents trained {} steps ({:.1f} s), {} replicas each for {} steps in inference mode ({:.1f} s)'
              .format(scenario, a_range[0], n, train_steps, t_train, R, eval_steps, t_eval))
        print('  deployed (frozen, {} unseen traffic realisations per agent): violations per stage {}, resource occupation {}'
              .format(R, fmt.format(*dep['violations']), fmt.format(*dep['occupation'])))
        print('  training runs, last {} steps (one trajectory per agent, still learning): violations per stage {}, resource occupation {}'
              .format(window, fmt.format(*trained['violations']), fmt.format(*trained['occupation'])))
    if control is not None:
        t2 = time.perf_counter()
        hc = _fleet_run(control, scenario, n * R, eval_steps, device, graph)
        lc = window_statistics(hc['violation'].reshape(shape), hc['resources'].reshape(shape), n_prbs)
        summary['learning_control'] = dict(lc, wall_s=time.perf_counter() - t2, pool=control.pool())
        control.close()
        if verbose:
            print('  the same agents on the same fleet with learning left on (full forks): violations per stage {}, resource occupation {}'
                  .format(fmt.format(*lc['violations']), fmt.format(*lc['occupation'])))
    return summary


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenarios', type=int, nargs='*', default=[0, 1, 2])
    ap.add_argument('--runs', type=int, default=RUNS)
    ap.add_argument('--train-steps', type=int, default=TRAIN_STEPS)
    ap.add_argument('--eval-replicas', type=int, default=EVAL_REPLICAS)
    ap.add_argument('--eval-steps', type=int, default=EVAL_STEPS)
    ap.add_argument('--out', default='./results')
    ap.add_argument('--learning-control', action='store_true',
                    help='also run full forks of the agents, learning left on, against the same fresh environments')
    ap.add_argument('--by-reference', action='store_true',
                    help="the replicas of an agent share one read-only copy of its dictionaries (kb_deploy_ref): same results, the agents' pool")
    ap.add_argument('--save-agents', metavar='DIR', help='write the trained agents of every cell to DIR (one agent file per cell)')
    ap.add_argument('--load-agents', metavar='DIR', help='skip training: evaluate the agents --save-agents wrote to DIR')
    ap.add_argument('--algorithm', choices=['projectron', 'projectron_plus'], default='projectron',
                    help='the update rule of the agents; projectron_plus turns the closed loop\'s margin-rule update phase on')
    ap.add_argument('--control-plus-batch', type=int, choices=[0, 2, 4, 8], default=0, metavar='W',
                    help='with --algorithm projectron_plus: W candidates of a step share one pass over Kinv (same results; 0: one by one)')
    ap.add_argument('--control-plus-wide', type=int, default=0, metavar='M',
                    help='with --control-plus-batch: learners of M landmarks or more have their passes over Kinv spread over the chip '
                         '(same results; 0: every row on one workgroup)')
    args = ap.parse_args()
    if args.control_plus_batch and args.algorithm != 'projectron_plus':
        ap.error('--control-plus-batch needs --algorithm projectron_plus')
    if args.control_plus_wide and not args.control_plus_batch:
        ap.error('--control-plus-wide needs --control-plus-batch')
    if args.load_agents and args.save_agents:
        ap.error('--load-agents evaluates agents from their files: it neither trains nor saves')
    for scenario, a_range in product(args.scenarios, accuracy_list):
        train_and_deploy(scenario, a_range, range(args.runs), train_steps=args.train_steps, eval_replicas=args.eval_replicas,
                         eval_steps=args.eval_steps, out_dir=args.out, learning_control=args.learning_control,
                         by_reference=args.by_reference, save_agents=args.save_agents, load_agents=args.load_agents,
                         algorithm=args.algorithm, control_plus_batch=args.control_plus_batch,
                         control_plus_wide=args.control_plus_wide)
