#!/usr/bin/env python3
"""The clairvoyant allocation baseline (the paper's ORACLE curve, which the reference ships as results only:
results/scenario_3/ORACLE/results_K.npz, read by its plot_oracle_results.py).  Every run of a scenario is one replica of
ONE VecRanSlice, advanced by VecRanSlice.step_clairvoyant: per replica and step, slice by slice, the fewest PRBs that meet the
slice's SLA in a fork of the replica stepped once (else, here by default, the widest least-violating one), then the real step
("Clairvoyant baseline").  Run i is seeded as Evaluator.evaluate(i) / BatchedEvaluator seed it (the first draw of
default_rng(seed=i)), and results/scenario_N/ORACLE/results_i.npz holds, per step, the reference's keys:
  SLA        sum of the step's SLA labels (+1 / -1 per slice)
  violation  total violations of the step
  resources  PRBs of the applied action

  python experiments_clairvoyant.py [--scenarios 3] [--runs 30] [--steps 5000] [--out ./results] [--fallback widest]
"""
import argparse
import os
import time

import numpy as np
from numpy.random import default_rng

import scenario_creator as sc

STEPS = 5000
RUNS = 30
scenarios = [3]
name = 'ORACLE'   # the directory the reference's plot script reads
# A slice that no allocation serves within one step gets the widest of its least-violating candidates here.  The rule's
# default (the cheapest) starves an mMTC slice once its backlog is too old for one step to bring the mean delay under the
# SLA: it keeps getting 0 PRBs, and its queue outgrows the build's capacity within a few hundred steps.
FALLBACK = 'widest'


def run_seeds(runs):
    """environment seeds of runs `runs`, drawn as Evaluator.evaluate(i) draws them (create_env's one draw)"""
    return np.array([int(default_rng(seed=i).integers(0, 2 ** 63 - 1)) for i in runs], dtype=np.uint64)


class StepRecord:
    """per-run histories of the three keys, one column per step"""

    def __init__(self, n_runs, steps):
        self.sla = np.zeros((n_runs, steps), dtype=np.int64)
        self.violation = np.zeros((n_runs, steps), dtype=np.int64)
        self.resources = np.zeros((n_runs, steps), dtype=np.int64)

    def add(self, t, actions, labels, violations):
        self.sla[:, t] = labels.sum(axis=1)
        self.violation[:, t] = violations.sum(axis=1)
        self.resources[:, t] = actions.sum(axis=1)

    def results(self, k):
        return dict(SLA=self.sla[k], violation=self.violation[k], resources=self.resources[k])


def evaluate(scenario, runs=range(RUNS), steps=STEPS, out_dir='./results', device=0, max_branches=None, fallback=FALLBACK,
             verbose=True):
    """all runs of `scenario` as one batch; writes the results files and returns a summary"""
    from ranslice import config as _c
    from ranslice.vec_env import VecRanSlice, default_fading
    runs = list(runs)
    n = len(runs)
    fading = sc._FADING if sc._FADING is not None else default_fading()
    env = VecRanSlice(n_envs=n, cfg=_c.make_config(scenario, n_envs=n), fading=fading, device=device)
    env.set_lookahead(max_branches)
    env.set_clairvoyant_fallback(fallback)
    env.reset(seeds=run_seeds(runs))
    rec = StepRecord(n, steps)
    t0 = time.perf_counter()
    for t in range(steps):
        actions, _, _, labels, violations = env.step_clairvoyant()
        rec.add(t, actions, labels, violations)
    wall = time.perf_counter() - t0
    env.close()
    path = '{}/scenario_{}/{}/'.format(out_dir, scenario, name)
    os.makedirs(path, exist_ok=True)
    for k, i in enumerate(runs):
        np.savez('{}results_{}.npz'.format(path, i), **rec.results(k))
    summary = dict(scenario=scenario, runs=n, steps=steps, wall_s=wall, max_branches=env._lookahead, fallback=fallback,
                   mean_prbs_per_step=float(rec.resources.mean()), total_violations=int(rec.violation.sum()),
                   violations_per_step=float(rec.violation.mean()), path=path)
    if verbose:
        print('scenario {}: {} runs x {} steps in {:.1f} s, {:.2f} PRBs per step, {} violations -> {}'.format(
            scenario, n, steps, wall, summary['mean_prbs_per_step'], summary['total_violations'], path))
    return summary


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=STEPS)
    ap.add_argument('--runs', type=int, default=RUNS)
    ap.add_argument('--scenarios', type=int, nargs='*', default=scenarios)
    ap.add_argument('--out', default='./results')
    ap.add_argument('--max-branches', type=int, default=None, help='forked replicas per search launch (default: from free memory)')
    ap.add_argument('--fallback', choices=['widest', 'cheapest'], default=FALLBACK,
                    help='what a slice that no allocation serves gets: the widest or the cheapest least-violating one')
    args = ap.parse_args()
    for scenario in args.scenarios:
        evaluate(scenario, range(args.runs), steps=args.steps, out_dir=args.out, max_branches=args.max_branches,
                 fallback=args.fallback)
