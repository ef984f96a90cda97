#!/usr/bin/env python3
"""Measures kb_fit's chip-wide rounds (kb_set_fit_wide) against the PARENT commit's library and writes
profiles/fit_wide_record.json.  No threshold is attached to any figure.  Kernel timing is on throughout: device times are HIP
events through kb_fit_time_ms, wall times time.perf_counter around the one kb_fit call.  Every run is a child process of its own
under `timeout`, with a fresh handle and a warm-up fit before the measured call.

  --parent-root DIR   a checkout of the parent commit whose library is built (DIR/network-slicing_amd/csrc/build/libranslice.so):
                      the parent's runs import its Python package and load its library; the fixtures come from this tree.

Legs:
  compare   G17 (12,400 samples to 3,143 landmarks) and G14 (7,000 to 790) through ONE kb_fit: the parent build (narrow) and this
            build with min_landmarks = KB_BIG_M (320), three rounds alternating the two; wall and device time as median and range;
            the dictionaries' bytes compared through a digest.
  sweep     this build on both recordings, min_landmarks in {64, 128, 256, 320, 512, 1024} at the default window, and window in
            {8, 64, 256} at 320; one run each.  recommended_min_landmarks: the smallest swept value from which every swept value,
            on both recordings, beats the parent's fastest run by more than the spread of the compare leg (the two ranges added).
  eight     eight copies of G17 as eight learners of one call: parent (eight lone workgroups) against this build (one work line).
  fleet     G9's d4 stream to 4,096 learners of one call on this build, the setting off and on at 320 (everything stays narrow:
            what the classification and its one look per chunk cost), three rounds alternating.

  plus      Projectron++ mode (kb_set_algorithm; kb_set_fit_wide_plus): G17's sample stream with min_landmarks = 320 and G18's rev
            stream (2,500 samples to 318 landmarks) with min_landmarks = 64, default window; the parent build (narrow: it has no
            switch) against this build with both settings on, three rounds alternating; per row the branch counts 0-4, the
            rounds' mat-vecs and tiles, and the dictionaries' digests, which must be equal between the two builds.

  python tools/fit_wide_record.py --parent-root DIR [--only compare|sweep|eight|fleet|plus]
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
KB_BIG_M = 320
MINS = (64, 128, 256, 320, 512, 1024)
WINDOWS = (8, 64, 256)
PLUS_STREAMS = (('g17_projectron_3000', KB_BIG_M), ('g18_projectron_plus:rev', 64))   # (recording, min_landmarks) of the Projectron++ leg


def _paths(root):
    for p in (root, os.path.join(root, 'network-slicing_amd')):
        if p not in sys.path:
            sys.path.insert(0, p)


def _stream(name):
    import numpy as np
    if ':' in name:   # a tagged recording, e.g. g18_projectron_plus:rev
        name, tag = name.split(':')
        g = np.load(os.path.join(GOLDEN, name + '.npz'))
        return g[tag + '_x'], g[tag + '_y']
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    if 'x' in g.files:
        return g['x'], g['y']
    if 'd4_x' in g.files:
        return g['d4_x'], g['d4_y']
    return np.concatenate([g['state'].astype(np.float64), (g['a'].astype(np.float64) / 200)[:, None]], axis=1), g['y']


def child(root, name, copies, min_landmarks, window, plus=False):
    """one measured kb_fit of `copies` learners, each taught the recording -> one JSON line.  plus: in Projectron++ mode, and with
    kb_set_fit_wide_plus on wherever the wide path is (min_landmarks != 0: a build that has the switch)"""
    import numpy as np
    _paths(root)
    from ranslice.kbrl_dev import VecKBRL
    xs, ys = _stream(name)
    d = xs.shape[1] - 1

    def handle(n):
        ag = VecKBRL(n, [d], 200, capacity=4096, pool_bytes=2 << 30, **(dict(algorithm='projectron_plus') if plus else {}))
        ag.reset(np.full((n, 1), 10), np.full((n, 1), 3))
        ag.set_kernel_timing(True)
        if min_landmarks:
            ag.set_fit_wide(min_landmarks, window)
            if plus:
                ag.set_fit_wide_plus(True)
        return ag
    warm = handle(1)   # first launches load code objects: both paths, when the setting is on
    if min_landmarks:
        warm.set_fit_wide(2, window)
    warm.fit([(0, 0)], [xs[:64]], [ys[:64]], chunk=16)
    warm.close()
    ag = handle(copies)
    learners = [(e, 0) for e in range(copies)]
    X, Y = [xs] * copies, [ys] * copies
    t0 = time.perf_counter()
    res = ag.fit(learners, X, Y)
    wall = time.perf_counter() - t0
    w = ag.fit_time_ms()
    h = hashlib.sha256()
    for e in sorted({0, copies - 1}):
        L = ag.learner(e, 0, with_kinv=True)
        for k in ('landmarks', 'coeff', 'kinv'):
            h.update(L[k].tobytes())
    out = dict(wall_ms=1e3 * wall, device_ms=w['fit_ms'], samples=w['samples'], mistakes=w['mistakes'],
               landmarks=int(ag.dictionary_sizes().max()), digest=h.hexdigest())
    if min_landmarks:
        out['wide'] = ag.fit_wide_info()
    if plus:
        out['branches'] = np.bincount(res['branch'][0], minlength=5).tolist()
    ag.close()
    print(json.dumps(out))


def run(root, name, copies=1, min_landmarks=0, window=0, timeout=300, plus=False):
    cmd = ['timeout', '-k', '10', str(timeout), sys.executable, os.path.abspath(__file__), '--child', name, '--root', root,
           '--copies', str(copies), '--min', str(min_landmarks), '--window', str(window)] + (['--plus'] if plus else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit('%s failed with status %d\n%s' % (' '.join(cmd), p.returncode, p.stderr[-2000:]))
    return json.loads(p.stdout.strip().splitlines()[-1])


def _summary(runs):
    out = {}
    for k in ('wall_ms', 'device_ms'):
        v = [r[k] for r in runs]
        out[k] = dict(median=statistics.median(v), min=min(v), max=max(v))
    out['digests'] = sorted({r['digest'] for r in runs})
    for k in ('samples', 'mistakes', 'landmarks', 'wide', 'branches'):
        if k in runs[-1]:
            out[k] = runs[-1][k]
    return out


def pair(parent_root, name, copies, min_landmarks, rounds=3, timeout=300, plus=False):
    """`rounds` alternating runs of the parent build (narrow) and this build (wide)"""
    a, b = [], []
    for _ in range(rounds):
        a.append(run(parent_root, name, copies, 0, 0, timeout, plus))
        b.append(run(ROOT, name, copies, min_landmarks, 0, timeout, plus))
    pa, th = _summary(a), _summary(b)
    spread = (pa['wall_ms']['max'] - pa['wall_ms']['min']) + (th['wall_ms']['max'] - th['wall_ms']['min'])
    return dict(parent_narrow=pa, this_wide=th, min_landmarks=min_landmarks, rounds=rounds,
                dictionary_bytes_equal=pa['digests'] == th['digests'] and len(pa['digests']) == 1,
                wall_ratio_parent_over_wide=pa['wall_ms']['median'] / th['wall_ms']['median'], spread_wall_ms=spread,
                wide_faster_beyond_spread=pa['wall_ms']['min'] - th['wall_ms']['max'] > spread)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child')
    ap.add_argument('--root', default=ROOT)
    ap.add_argument('--copies', type=int, default=1)
    ap.add_argument('--min', type=int, default=0)
    ap.add_argument('--window', type=int, default=0)
    ap.add_argument('--plus', action='store_true')
    ap.add_argument('--parent-root')
    ap.add_argument('--only', choices=['compare', 'sweep', 'eight', 'fleet', 'plus'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fit_wide_record.json'))
    a = ap.parse_args()
    if a.child:
        return child(a.root, a.child, a.copies, a.min, a.window, a.plus)
    if not a.parent_root:
        raise SystemExit('--parent-root: a checkout of the parent commit with its library built')
    rec = dict(statistic='median and range of three alternating runs (compare, eight, fleet); one run per sweep point',
               default_window=64, default_chunk=256, KB_BIG_M=KB_BIG_M)
    if os.path.exists(a.out):
        with open(a.out) as f:
            rec.update(json.load(f))
    names = ('g17_projectron_3000', 'g14_projectron_long')

    def save():
        with open(a.out, 'w') as f:
            json.dump(rec, f, indent=1)
            f.write('\n')
    if a.only in (None, 'compare'):
        rec['compare'] = {n: pair(a.parent_root, n, 1, KB_BIG_M) for n in names}
        print(json.dumps(rec['compare']), flush=True)
        save()
    if a.only in (None, 'sweep'):
        sw = {}
        for n in names:
            sw[n] = dict(min_landmarks={str(m): run(ROOT, n, 1, m, 0) for m in MINS},
                         window_at_320={str(w): run(ROOT, n, 1, KB_BIG_M, w) for w in WINDOWS})
        rec['sweep'] = sw
        if 'compare' in rec:
            good = []
            for m in MINS:
                ok = True
                for n in names:
                    c = rec['compare'][n]
                    ok = ok and c['parent_narrow']['wall_ms']['min'] - sw[n]['min_landmarks'][str(m)]['wall_ms'] > c['spread_wall_ms']
                    ok = ok and sw[n]['min_landmarks'][str(m)]['digest'] in c['parent_narrow']['digests']
                good.append(ok)
            rec['recommended_min_landmarks'] = next((m for i, m in enumerate(MINS) if all(good[i:])), None)
        print(json.dumps(rec['sweep']), flush=True)
        save()
    if a.only in (None, 'eight'):
        rec['eight_copies_of_g17'] = pair(a.parent_root, names[0], 8, KB_BIG_M, rounds=1, timeout=600)
        print(json.dumps(rec['eight_copies_of_g17']), flush=True)
        save()
    if a.only in (None, 'fleet'):
        off, on = [], []
        for _ in range(3):
            off.append(run(ROOT, 'g9_projectron', 4096, 0, 0))
            on.append(run(ROOT, 'g9_projectron', 4096, KB_BIG_M, 0))
        rec['fleet_d4_x_4096'] = dict(setting_off=_summary(off), setting_on_at_320=_summary(on))
        print(json.dumps(rec['fleet_d4_x_4096']), flush=True)
        save()
    if a.only in (None, 'plus'):
        rec['projectron_plus'] = {n: pair(a.parent_root, n, 1, m, timeout=600, plus=True) for n, m in PLUS_STREAMS}
        print(json.dumps(rec['projectron_plus']), flush=True)
        save()


if __name__ == '__main__':
    main()
