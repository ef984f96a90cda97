#!/usr/bin/env python3
"""G18: golden sequences of the reference's ProjectronPlus (projectron.py:66-107), recorded as G9 / G14 record Projectron.

Run from the repo root:  python tools/gen_golden_plus.py
Writes tests/golden/g18_projectron_plus.npz and nothing else.  Two tags:
  d4   G9's `d4` stream verbatim (same seeds, the two far-away tie samples included), 1,200 samples
  rev  G14's revisit stream with its seeds, cut to 2,500 samples (a dictionary past the 64 -> 65 shell and past 256)
Per sample: x, y, f, ypred, branch (0 nothing, 1 projection, 2 insertion, 3 margin update, 4 margin test without update),
delta (NaN for branch 0), slack = loss - delta / eta (NaN outside the margin case), m after the sample; the tie tape; the final
dictionary; Kinv (whole for d4, G14's digest for rev); for d4 the coefficient vector after every margin update.
The archive is written with fixed member dates, so a second run gives the same bytes.
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import gen_golden as gg  # noqa: E402
from gen_golden_kbrl import _kinv_digest  # noqa: E402

NAME = 'g18_projectron_plus'


def _stream_d4(n=1200, d=4):
    """G9's `d4` stream (gen_golden_kbrl._g9), sample by sample"""
    rng = np.random.default_rng(90 + d)
    for i in range(n):
        x = np.append(rng.random(d - 1).astype(np.float32), rng.integers(0, 201) / 200)
        score = x[:-1].mean() * 0.8 + 0.35 - x[-1]
        y = -1 if score + rng.normal(0, 0.05) > 0 else 1
        if i in (3, 4):
            x = x + (30.0 if i == 3 else 60.0)
        yield x, y


def _stream_rev(n=2500, d=11, spread=1.3, noise=0.12):
    """G14's stream (gen_golden_kbrl._g14), cut to n samples"""
    rng = np.random.default_rng(140)
    states = []
    for i in range(n):
        if states and rng.random() < 0.5:
            s = states[rng.integers(len(states))]
            if rng.random() < 0.5:
                s = (s + rng.normal(0, 0.02, d - 1)).astype(np.float32)
        else:
            s = (rng.random(d - 1) * spread).astype(np.float32)
        states.append(s)
        x = np.append(s, rng.integers(0, 201) / 200)
        score = x[:-1].mean() * 0.8 / spread + 0.35 - x[-1]
        y = -1 if score + rng.normal(0, noise) > 0 else 1
        yield x, y


def _record(tape, stream, np_seed, keep_coeff):
    from algorithms.kernel import GaussianKernel
    from algorithms.projectron import SVvariable, ProjectronPlus
    np.random.seed(np_seed)
    tape.clear()
    alg = ProjectronPlus(GaussianKernel(SVvariable(), 1))
    xs, ys, fs, ypred, branch, delta, slack, ms, after = [], [], [], [], [], [], [], [], []
    alpha_case = [0, 0, 0]     # which term of the min gave alpha: loss / norm, 1, 2 slack / norm
    margin_at_one = 0          # margin tests while a single landmark is held
    for x, y in stream:
        yp = alg.predict(x)
        f = float(alg.f)
        m0 = alg.counter
        dl = sl = np.nan
        br = 0
        margin = y * alg.f     # the expressions of projectron.py:72-84 / 88-92, evaluated on the reference's arrays
        if margin < 1 and margin > 0:
            loss = 1 - margin
            d_star = alg.Kinv @ alg.K_f
            if np.ndim(d_star) == 0:
                d_star = np.array([d_star], dtype=np.float32)
            kii = alg.kernel.k_eval(x, x)
            dl = max(kii - d_star @ alg.K_f, 0)
            norm = max(kii - dl, 0)
            sl = loss - dl / alg.eta
            br = 3 if sl > 0 else 4
            margin_at_one += m0 == 1
            if br == 3:
                with np.errstate(divide='ignore'):
                    terms = [loss / norm, 1, 2 * sl / norm]
                alpha_case[int(np.argmin(terms))] += 1
            dl, sl = float(dl), float(sl)
        elif margin <= 0:
            d_star = alg.Kinv @ alg.K_f
            if np.ndim(d_star) == 0:
                d_star = np.array([d_star], dtype=np.float32)
            dl = float(max(alg.kernel.k_eval(x, x) - d_star @ alg.K_f, 0))
        alg.update(x, y)
        if margin <= 0:
            br = 2 if alg.counter > m0 else 1
        if br == 3 and keep_coeff:
            after.append(np.asarray(alg.sv.coeff, dtype=np.float64).copy())
        xs.append(x); ys.append(y); fs.append(f); ypred.append(int(yp)); branch.append(br)
        delta.append(dl); slack.append(sl); ms.append(alg.counter)
    _, ties = tape.arrays()
    out = dict(x=np.asarray(xs), y=np.asarray(ys, dtype=np.int8), f=np.asarray(fs), ypred=np.asarray(ypred, dtype=np.int8),
               branch=np.asarray(branch, dtype=np.int8), delta=np.asarray(delta), slack=np.asarray(slack),
               m=np.asarray(ms, dtype=np.int32), ties=ties, landmarks=np.atleast_2d(alg.sv.landmarks),
               coeff=np.asarray(alg.sv.coeff, dtype=np.float64))
    if keep_coeff:
        pad = np.zeros((len(after), alg.counter))
        for i, c in enumerate(after):
            pad[i, :len(c)] = c
        out['coeff_after'] = pad
    return out, alg, alpha_case, margin_at_one


def _conditions(tag, rec, eta=0.1):
    """the conditions on the recording under which every branch can be asserted exactly"""
    br, dl, sl = rec['branch'], rec['delta'], rec['slack']
    assert (br == 3).sum() >= 100, '%s: only %d margin updates' % (tag, (br == 3).sum())
    margin = (br == 3) | (br == 4)
    mistake = (br == 1) | (br == 2)
    assert np.abs(sl[margin]).min() > 1e-6, '%s: a margin decision within 1e-6 of its threshold' % tag
    assert np.abs(dl[mistake] - eta).min() > 1e-6, '%s: a projection / insertion decision within 1e-6 of eta' % tag
    print('%s: %d samples, branches 0-4: %s, %d landmarks, min |slack| %.3g, min |delta - eta| %.3g' % (
        tag, len(br), np.bincount(br, minlength=5).tolist(), rec['m'][-1], np.abs(sl[margin]).min(),
        np.abs(dl[mistake] - eta).min()))


def save_fixed(path, arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    gg.rh.setup(tempfile.mkdtemp(prefix='refwork_g18_'), gg.fading_tables())
    tape = gg.rh.Tape()
    gg.rh.install_tape(tape)
    out = {}
    d4, alg, _, at_one = _record(tape, _stream_d4(), 9, keep_coeff=True)
    assert at_one >= 1, 'd4: no margin test while a single landmark is held'
    _conditions('d4', d4)
    print('d4: %d margin tests with one landmark' % at_one)
    d4['kinv'] = np.atleast_2d(np.asarray(alg.Kinv, dtype=np.float64))
    out.update({'d4_' + k: v for k, v in d4.items()})
    rev, alg, cases, _ = _record(tape, _stream_rev(), 14, keep_coeff=False)
    assert min(cases) >= 1, 'rev: alpha outcomes (loss / norm, 1, 2 slack / norm) = %s' % cases
    _conditions('rev', rev)
    print('rev: alpha outcomes (loss / norm, 1, 2 slack / norm) = %s' % cases)
    dg = _kinv_digest(alg.Kinv)
    rev.update(kinv_rows=dg['rows'], kinv_diag=dg['diag'], kinv_probes=dg['probes'], kinv_kp=dg['kp'])
    out.update({'rev_' + k: v for k, v in rev.items()})
    path = os.path.join(gg.GOLD, NAME + '.npz')
    save_fixed(path, out)
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
