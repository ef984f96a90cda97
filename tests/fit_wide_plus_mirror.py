"""The round structure of kb_fit's wide path in Projectron++ mode (kb_set_fit_wide_plus; csrc/kb_fit_wide.hip)
restated in NumPy over tests/plus_mirror.py's PlusMirror(plus=True).  Used by tests/test_fit_wide_plus_mirror.py (CPU: the rounds
leave exactly the sequential result) and tests/test_gpu_fit_wide_plus.py (device: kb_fit_wide_info equals `counters`).  Not a test
module; tests/fit_wide_mirror.py stays what it is, the Projectron rounds.

A learner's samples are cut into chunks of `chunk`.  A chunk that starts with the dictionary at min_landmarks (>= 2) or more is
taught by rounds, any other sample by sample.  A round scores the next min(window, samples left in the chunk) samples against the
dictionary as it stands, writing nothing.  The samples before the first one with not (y f >= 1) are final (branch 0); that one is
predicted and updated as the sequential path does it -- a mistake y f <= 0 projects or inserts (branches 1, 2), a sample inside
the margin gets the scaled projection (3) or, when its slack is not positive, nothing (4) -- and the cursor moves past it; without
such a sample the cursor moves past the window.  When the chunk's last sample needed no update, it is predicted once more so that
the cached kernel column is its own.

AFTER BRANCH 4 the dictionary is what it was, so the rest of the window's scores would still be the sequential ones; the rounds do
NOT reuse them.  Every round scans again from its cursor, after branch 4 as after branches 1-3: the round keeps no window origin.
Counter [3] below defines that choice: every round adds its whole window, whatever the branch that ended the round before.

The four counters of kb_fit_wide_info: [0] samples taught by rounds, [1] mat-vecs (the samples of branches 1-4 taught there:
every one of them needs d* = Kinv K_f), [2] Kinv tiles those mat-vecs read, n_b (n_b + 1) / 2 with n_b = ceil(m / 64) of the
dictionary BEFORE the update, [3] kernel evaluations of the window scans, samples scored x m."""
import numpy as np

from plus_mirror import PlusMirror

KB_FIT_WINDOW = 64
KB_FIT_CHUNK = 256


def _tiles(m):
    nb = (m + 63) >> 6
    return nb * (nb + 1) // 2


def _score(mir, x):
    """f of predict(x) with nothing kept: the scan writes no kernel column and draws no tie"""
    keep = mir.f, mir.kf
    _, f = mir.predict(x, tie=None)
    mir.f, mir.kf = keep
    return f


def fit(x, y, chunk=0, min_landmarks=0, window=0, tie=None, gamma=1.0, eta=0.1, mir=None):
    """teach the stream through the chunks, by rounds where the setting says so -> (mirror, per-sample dict f, ypred, branch, delta,
    m, counters [4]).  min_landmarks = 0: plus_mirror.replay's loop.  tie(): the draw of an exact tie."""
    assert min_landmarks == 0 or min_landmarks >= 2
    chunk = chunk or KB_FIT_CHUNK
    window = window or KB_FIT_WINDOW
    mir = mir or PlusMirror(gamma=gamma, eta=eta, plus=True)
    assert mir.plus
    n = len(x)
    out = dict(f=np.zeros(n), ypred=np.zeros(n, dtype=np.int64), branch=np.zeros(n, dtype=np.int64), delta=np.zeros(n),
               m=np.zeros(n, dtype=np.int64))
    info = [0, 0, 0, 0]

    def one(r):
        """the sequential path's sample: predict, then update"""
        out['ypred'][r], out['f'][r] = mir.predict(x[r], tie=tie)
        m = mir.m
        br, dl, _ = mir.update(x[r], y[r])
        out['branch'][r], out['delta'][r], out['m'][r] = br, (0.0 if br == 0 else dl), mir.m
        return br, m

    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        if not (min_landmarks >= 2 and mir.m >= min_landmarks):
            for r in range(r0, r1):
                one(r)
            continue
        cur = r0
        while cur < r1:
            cnt = min(window, r1 - cur)
            info[3] += cnt * mir.m       # (after branch 4 too: no score of the round before is used again)
            fs = [_score(mir, x[cur + t]) for t in range(cnt)]
            k = next((t for t in range(cnt) if not (float(y[cur + t]) * fs[t] >= 1.0)), cnt)
            for t in range(k):
                r = cur + t
                out['ypred'][r], out['f'][r], out['m'][r] = (1 if fs[t] > 0 else -1), fs[t], mir.m
            info[0] += k
            if k < cnt:
                br, m = one(cur + k)
                assert br in (1, 2, 3, 4) and m >= 2
                assert br != 2 or mir.m == m + 1     # (these streams never saturate)
                assert br == 2 or mir.m == m         # the margin rule never inserts
                info[0] += 1
                info[1] += 1
                info[2] += _tiles(m)
                cur += k + 1
            else:
                cur += cnt
                if cur == r1:
                    mir.predict(x[r1 - 1], tie=None)
    return mir, out, info


def counters(branch, m_after, m0=0, chunk=0, min_landmarks=0, window=0):
    """kb_fit_wide_info of ONE learner from what a fit returned for it (its branch codes and sizes; m0 = its size before the call):
    the rounds' cursor depends on the data only through where the samples of branches 1-4 are"""
    chunk = chunk or KB_FIT_CHUNK
    window = window or KB_FIT_WINDOW
    branch, m_after = np.asarray(branch), np.asarray(m_after)
    n = len(branch)
    info = [0, 0, 0, 0]
    if min_landmarks < 2:
        return info
    before = np.concatenate([[m0], m_after[:-1]]) if n else np.zeros(0, dtype=np.int64)   # the size each sample was predicted against
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        if before[r0] < min_landmarks:
            continue
        info[0] += r1 - r0
        cur = r0
        while cur < r1:
            cnt = min(window, r1 - cur)
            m = int(before[cur])
            info[3] += cnt * m
            hit = np.nonzero(branch[cur:cur + cnt] != 0)[0]   # branches 1-4: each ends its round, 4 included
            if len(hit):
                info[1] += 1
                info[2] += _tiles(m)
                cur += int(hit[0]) + 1
            else:
                cur += cnt
    return info
