#!/usr/bin/env python3
"""Measures kb_fit / kb_update in Projectron++ mode and writes profiles/plus_record.json.  No threshold is attached
to any figure; every figure is ONE run.  Kernel timing is on throughout (kb_set_kernel_timing): device times are HIP events
through kb_fit_time_ms, wall times time.perf_counter around the call (which waits for the device).

  rev     G18's `rev` stream (2,500 samples; tests/golden/g18_projectron_plus.npz) through ONE kb_fit in Projectron++ mode and, for
          orientation, in Projectron mode on the same build, with both final dictionary sizes; the same stream one sample at a
          time (kb_predict, kb_update) in Projectron++ mode.
  fleet   --agents (4096) learners, each fitted with G18's `d4` stream (1,200 samples) in one call, in both modes.

  python tools/plus_record.py [--agents 4096] [--out profiles/plus_record.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
for p in (ROOT, os.path.join(ROOT, 'network-slicing_amd'), os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)
MODES = ('projectron_plus', 'projectron')


def _kernel_resources():
    """registers / scratch of the two fit instances from the build's remarks (csrc/build/resources.log), if it is there"""
    import check_resources as cr
    if not os.path.exists(cr.LOG):
        return None
    res, out = cr.parse(), {}
    for key in ('fit_kernel', 'fit_plus_kernel'):
        hit = [k for k in res if key in k and 'kb' in k]
        if hit:
            r = res[hit[0]]
            out[key] = dict(vgprs=r.get('VGPRs'), scratch_bytes_per_lane=r.get('ScratchSize'), occupancy=r.get('Occupancy'),
                            lds_bytes=r.get('LDS Size'))
    return out


def _handle(n, d, mode, pool_bytes):
    import numpy as np
    from ranslice.kbrl_dev import VecKBRL
    ag = VecKBRL(n, [d - 1], 200, capacity=1024, pool_bytes=pool_bytes, algorithm=mode)
    ag.reset(np.full((n, 1), 10), np.full((n, 1), 3))
    ag.set_kernel_timing(True)
    return ag


def _fit_leg(ag, learners, X, Y):
    import numpy as np
    t0 = time.perf_counter()
    out = ag.fit(learners, X, Y)
    wall = time.perf_counter() - t0
    w = ag.fit_time_ms()
    br = np.concatenate(out['branch'])
    sizes = ag.dictionary_sizes()
    return dict(wall_ms=wall * 1e3, device_ms=w['fit_ms'], samples=w['samples'], mistakes=w['mistakes'], insertions=w['insertions'],
                kernel_evals=w['kernel_evals'], branches=np.bincount(br, minlength=5).tolist(),
                landmarks_max=int(sizes.max()), landmarks_mean=float(sizes.mean()), flagged=sum(len(v) for v in ag.flagged_replicas().values()))


def main():
    import numpy as np
    ap = argparse.ArgumentParser()
    ap.add_argument('--agents', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'plus_record.json'))
    args = ap.parse_args()
    g = np.load(os.path.join(GOLDEN, 'g18_projectron_plus.npz'))
    for mode in MODES:   # first launches load code objects
        warm = _handle(1, 11, mode, 64 << 20)
        warm.fit([(0, 0)], [g['rev_x'][:40]], [g['rev_y'][:40]])
        for x, y in zip(g['rev_x'][:40], g['rev_y'][:40]):
            warm.predict(0, 0, x)
            warm.update(0, 0, x, int(y))
        warm.close()
    rec = dict(what='kb_fit / kb_update in Projectron++ mode; one run per figure, no threshold attached', kernels=_kernel_resources())
    rev = {}
    for mode in MODES:
        ag = _handle(1, 11, mode, 256 << 20)
        rev[mode] = _fit_leg(ag, [(0, 0)], [g['rev_x']], [g['rev_y']])
        ag.close()
    ag = _handle(1, 11, 'projectron_plus', 256 << 20)
    t0 = time.perf_counter()
    for x, y in zip(g['rev_x'], g['rev_y']):
        ag.predict(0, 0, x)
        ag.update(0, 0, x, int(y))
    ag.synchronize()
    rev['projectron_plus_one_by_one'] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, round_trips=2 * len(g['rev_x']),
                                             landmarks=int(ag.dictionary_sizes()[0, 0]))
    ag.close()
    rec['rev'] = dict(samples=len(g['rev_x']), **rev)
    n = args.agents
    fleet = {}
    learners = [(e, 0) for e in range(n)]
    X, Y = [g['d4_x']] * n, [g['d4_y']] * n
    for mode in MODES:
        ag = _handle(n, 4, mode, 2 << 30)
        fleet[mode] = _fit_leg(ag, learners, X, Y)
        fleet[mode]['samples_per_s_device'] = fleet[mode]['samples'] / (fleet[mode]['device_ms'] * 1e-3) if fleet[mode]['device_ms'] else None
        ag.close()
    rec['fleet'] = dict(agents=n, samples_per_learner=len(g['d4_x']), **fleet)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
