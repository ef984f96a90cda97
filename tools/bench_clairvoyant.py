#!/usr/bin/env python3
"""Cost of the clairvoyant baseline (VecRanSlice.step_clairvoyant, DESIGN.md "Clairvoyant baseline"):
  search  wall time of one clairvoyant step of `--replicas` replicas of `--scenario` (default 4096 of scenario 0: 5 rounds x
          201 candidates = 4.1 M branch env-steps), after one untimed step that builds the branch handle;
  run     experiments_clairvoyant.evaluate(--exp-scenario, --runs, --steps): wall time, mean PRBs per step, total
          violations, next to the reference's shipped ORACLE results (scenario 3: 19 runs x 5,000 steps, 12.08 PRBs per
          step, 0 violations).
Writes one JSON record (--out, default profiles/clairvoyant_record.json).  --skip-run / --skip-search leave a part out.

  python tools/bench_clairvoyant.py [--replicas 4096] [--scenario 0] [--runs 30] [--steps 5000] [--search-steps 3]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'network-slicing_amd')]

REFERENCE = dict(source='reference results/scenario_3/ORACLE (19 runs x 5,000 steps; its rule is not published)',
                 mean_prbs_per_step=12.08, total_violations=0)


def fork_bytes_per_replica(cfg):
    """bytes the search's gather copies per branch replica (rs_fork.hip: fork_table without the action row)"""
    e, m = cfg.n_embb, cfg.n_mmtc
    cap = cfg.max_mtc_queue if cfg.max_mtc_queue > 0 else 1024
    s_act = ((e > 0) + (m > 0)) if cfg.l1_multiplex else e + m
    embb = e * (5 * 4 + 32 * (3 * 8 + 9 * 4) + 32 * 16 * 2)
    mmtc = m * (4 + 8 + 8 + 3 * 4 * 1024 + 2 * 4 * cap)
    outputs = 4 * (10 * e + 3 * m) + 8 + 2 * 4 * s_act + 80 * (e + m)
    return embb + mmtc + 8 + 4 + outputs


def search(scenario, n, steps, max_branches=None):
    from ranslice.config import make_config
    from ranslice.vec_env import VecRanSlice, default_fading
    cfg = make_config(scenario, n_envs=n)
    env = VecRanSlice(n_envs=n, cfg=cfg, fading=default_fading(), seed=17)
    env.set_lookahead(max_branches)
    env.reset()
    for _ in range(3):   # UEs arrive before the first timed search
        env.step_clairvoyant()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        acts = env.step_clairvoyant()[0]
        times.append(time.perf_counter() - t0)
    C = cfg.n_prbs + 1
    rounds = env.n_slices
    chunk = min(env._lookahead // C, n)
    launches = rounds * -(-n // chunk)
    env.close()
    bpr = fork_bytes_per_replica(cfg)
    return dict(scenario=scenario, replicas=n, max_branches=env._lookahead, branch_replicas=chunk * C, rounds=rounds,
                search_launches=launches, branch_env_steps=launches * chunk * C,
                fork_bytes_per_branch=bpr, fork_bytes_per_step=2 * bpr * launches * chunk * C,
                step_s=times, step_s_min=min(times), mean_prbs=float(acts.sum(axis=1).mean()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--replicas', type=int, default=4096)
    ap.add_argument('--scenario', type=int, default=0)
    ap.add_argument('--search-steps', type=int, default=3)
    ap.add_argument('--exp-scenario', type=int, default=3)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--steps', type=int, default=5000)
    ap.add_argument('--max-branches', type=int, default=None)
    ap.add_argument('--fallback', choices=['widest', 'cheapest'], default='widest')
    ap.add_argument('--skip-search', action='store_true')
    ap.add_argument('--skip-run', action='store_true')
    ap.add_argument('--results', default=None, help='where the experiment writes its ORACLE directory (default: a temporary one)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'clairvoyant_record.json'))
    a = ap.parse_args()
    rec = dict(tool='tools/bench_clairvoyant.py', argv=sys.argv[1:])
    if not a.skip_search:
        rec['search'] = search(a.scenario, a.replicas, a.search_steps, a.max_branches)
        print(json.dumps(rec['search']), flush=True)
    if not a.skip_run:
        import experiments_clairvoyant as ec
        out_dir = a.results or tempfile.mkdtemp(prefix='clairvoyant_')
        s = ec.evaluate(a.exp_scenario, range(a.runs), steps=a.steps, out_dir=out_dir, max_branches=a.max_branches,
                        fallback=a.fallback)
        rec['run'] = dict(s, reference=REFERENCE if a.exp_scenario == 3 else None)
        print(json.dumps(rec['run']), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=1)
    print('record ->', a.out)


if __name__ == '__main__':
    main()
