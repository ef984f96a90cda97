"""The segmented apply of a growing shared dictionary under the margin rule (kb_set_shared_plus_batch, DESIGN.md section 8r;
csrc/kb_shared_plus_batch.hip) restated on the existing mirrors.  Used by tests/test_shared_plus_batch_mirror.py (CPU) and
tests/test_gpu_shared_plus_batch.py (device).  Not a test module.

  segmented_apply_plus   a merged list against a dictionary of min_landmarks <= m < capacity landmarks, in segments:
                           1. shared_mirror.full_batch's KF, DS, F0 and A of the REMAINING proposals against the dictionary as it
                              stands, rows and columns counted from the segment's first proposal;
                           2. the walk f_p = F0_p + g_p with g = 0 at the segment's start, decided by shared_plus_mirror.margin_weight;
                              a mistake whose max(1 - A[p][p], 0) > eta below the capacity STOPS the walk before it is applied; a
                              mistake that does not stop projects with w_p = y_p (the saturation flag only at the capacity);
                           3. the coefficients take c + w_p DS[p] of the applied proposals in list order;
                           4. the stopping sample goes through update_mirror.step_plus(order='col')'s mistake arm, which decides for itself
                              (branch 1 or 2); the next segment starts behind it.
                         A list that is not engaged (m < min_landmarks, m >= capacity, no proposal) goes as it does without the
                         switch: growing_apply_plus / full_batch_plus.
  batch_list             a list of update_mirror's picked cases with inserting samples at given places.

Two deliberately WRONG variants for the tests of the tests: 'stale_f0' keeps the previous segment's F0 after an insertion,
'carry_g' does not reset g at a segment's start."""
import numpy as np

import shared_mirror as shm
import shared_plus_mirror as spm
import update_mirror as um

WRONG = ('stale_f0', 'carry_g')


def _near(dec, margin, eta, below_capacity, clearance):
    """whether the walk's decision lies within `clearance` of one of its thresholds"""
    if abs(margin) < clearance or abs(margin - 1.0) < clearance:
        return True
    if dec['branch'] == 0:
        return False
    if dec['branch'] == 1:
        return below_capacity and abs(dec['delta'] - eta) < clearance
    if abs(dec['slack']) < clearance:
        return True
    if dec['branch'] == 4 or dec['norm'] == 0.0:
        return False
    t = sorted(dec['terms'])
    return t[1] - t[0] < clearance


def segmented_apply_plus(Kinv, coeff, landmarks, props, gamma, n_prbs, d, eta=0.1, capacity=None, min_landmarks=2, count=None,
                         wrong=None, clearance=um.CLEARANCE):
    """-> dict(engaged, f [np] = the f_p decided on, branch [np] in 0 .. 4, seg [np] = the segment that took the proposal, kinv,
    coeff, landmarks, m, n_changed (branches 1-3), n_grow (insertions), n_work (branches 1-4), sat, work = [engaged lists,
    segments walked, proposals covered by the segments' passes, segments ended by a stop], near = the applied samples within
    `clearance` of a threshold, terms [np])"""
    assert wrong is None or wrong in WRONG
    coeff = np.asarray(coeff, dtype=np.float64).copy()
    m = len(coeff)
    n = len(props) if count is None else count
    P = np.asarray(props, dtype=np.float64)[:n]
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m).copy()
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d).copy()
    cap = capacity if capacity is not None else 1 << 30
    if not (n > 0 and min_landmarks <= m < cap):
        if m >= cap and m >= 2 and n > 0:
            r = spm.full_batch_plus(Kinv, coeff, L, P, gamma, n_prbs, eta, count=n)
            out = dict(f=r['f'], branch=r['branch'], kinv=Kinv, coeff=r['coeff'], landmarks=L, m=m, sat=r['sat'], terms=r['terms'])
        else:
            r = spm.growing_apply_plus(Kinv, coeff, L, P, gamma, n_prbs, d, eta, capacity, count=n)
            out = dict(f=r['f'], branch=r['branch'], kinv=r['kinv'], coeff=r['coeff'], landmarks=r['landmarks'], m=r['m'], sat=False,
                       terms=[None] * n)
        br = np.asarray(out['branch'])
        out.update(engaged=False, seg=np.full(n, -1), n_changed=int(((br >= 1) & (br <= 3)).sum()), n_grow=int((br == 2).sum()),
                   n_work=int((br > 0).sum()), work=[0, 0, 0, 0], near=0)
        return out
    f, branch, seg = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    terms = [None] * n
    work = [1, 0, 0, 0]
    sat, near, frm, k = False, 0, 0, 0
    F0_prev = g_prev = None
    while frm < n:
        m = len(coeff)
        base = shm.full_batch(Kinv, coeff, L, P[frm:], gamma, n_prbs, eta)
        DS, F0, A, y = base['DS'], base['F0'], base['A'], base['y']
        nn = n - frm
        if wrong == 'stale_f0' and F0_prev is not None:
            F0 = F0_prev
        g = g_prev.copy() if (wrong == 'carry_g' and g_prev is not None) else np.zeros(nn)
        work[1] += 1
        work[2] += nn
        stop = -1
        for r in range(nn):
            p = frm + r
            f[p] = F0[r] + g[r]
            yp = float(y[r])
            dec = spm.margin_weight(yp * f[p], A[r, r], eta)
            near += int(_near(dec, yp * f[p], eta, m < cap, clearance))
            if dec['branch'] == 1 and dec['delta'] > eta:
                if m < cap:
                    stop = r
                    break
                sat = True
            branch[p], terms[p], seg[p] = dec['branch'], dec['terms'], k
            if dec['branch'] in (1, 3):
                w = dec['alpha'] * yp
                if r + 1 < nn:
                    g[r + 1:] = um.fma(w, A[r + 1:, r], g[r + 1:])
                coeff = coeff + w * DS[r]
        if stop < 0:
            break
        p = frm + stop
        word = int(P[p, 1])
        yp = 1 if word & 1 else -1
        x = np.append(P[p, 2:2 + d - 1], float(word >> 2) / float(n_prbs))
        # um.step_plus(order='col') entered with the walk's f_p, as the device enters apply_update_plus: y f_p <= 0, so its mistake
        # arm, um.step(order='col'), which decides branch 1 or 2 by its own residual.  (step_plus forms a fresh K_f . coeff; for the
        # right walk it must fall on the same side of 0 -- an input within rounding of the threshold otherwise.)
        if wrong is None:
            assert float(yp) * um.score(um.column(L, x, gamma), coeff) <= 0.0, 'the stopping sample is no mistake for a fresh f'
        st = um.step(Kinv, coeff, L, x, yp, gamma, eta, capacity, order='col')
        near += int(abs(st['delta'] - eta) < clearance)
        branch[p], seg[p] = st['branch'], k
        Kinv, coeff, L = st['kinv'], st['coeff'], st['landmarks']
        work[3] += 1
        F0_prev, g_prev = F0[stop + 1:], g[stop + 1:]
        frm = p + 1
        k += 1
    return dict(engaged=True, f=f, branch=branch, seg=seg, kinv=Kinv, coeff=coeff, landmarks=L, m=len(coeff),
                n_changed=int(((branch >= 1) & (branch <= 3)).sum()), n_grow=int((branch == 2).sum()), n_work=int((branch > 0).sum()),
                sat=bool(sat), work=work, near=near, terms=terms)


# ------------------------------------------------------------------ the inputs of the tests (CPU and device use the same)
BATCH_CASES = [    # (landmarks, state variables, proposals, the places of the inserting samples, capacity - landmarks)
    (2, 10, 1, (), 8), (2, 10, 17, (4,), 8), (63, 10, 17, (), 8), (64, 10, 17, (0,), 8), (65, 10, 17, (16,), 8), (65, 3, 17, (7, 8), 8),
    (63, 10, 64, (5, 20, 40), 8),       # 63 -> 66 landmarks: a shell is added, the mat-vec goes column walk, matrix cores, column walk
    (130, 10, 256, (30, 100), 8),
    (64, 10, 17, (3, 9), 1)]            # the capacity is reached at the first insertion: the second projects and raises the flag


def _inserting(mir, n_prbs, rng, eta, clearance):
    """a sample the learner `mir` misclassifies with delta > eta: a landmark's state shifted far enough, labelled against the sign"""
    d = mir.L.shape[1]
    for _ in range(400):
        j = int(rng.integers(mir.m))
        t = float(rng.uniform(0.15, 0.5)) * (1 if rng.integers(2) else -1)
        a = int(np.clip(int(round(mir.L[j, d - 1] * n_prbs)) + int(rng.integers(-30, 31)), 0, n_prbs))
        x = np.append((mir.L[j, :d - 1] + t).astype(np.float32).astype(np.float64), a / float(n_prbs))
        _, f = mir.predict(x)
        _, delta = mir._project()
        if abs(f) >= 1e-3 and delta >= eta + 1e-3:
            return x, (-1 if f > 0 else 1)
    raise AssertionError('no inserting sample found')


def batch_list(Kinv, coeff, landmarks, n_prbs, n, insert_at, capacity, gamma=1.0, eta=0.1, seed=0, clearance=um.CLEARANCE):
    """a merged list of n proposals [n, 18] against a dictionary that can grow to `capacity`: shared_plus_mirror.plus_list's
    rotation of update_mirror's picked cases under the coefficients the sequential learner beside it holds when the proposal's turn
    comes, a projected mistake every sixth proposal, and at the places of `insert_at` a sample that asks for an insertion (at the
    capacity it projects and raises the saturation flag) -> (props, branches [n] the sequential learner took)"""
    L = np.asarray(landmarks, dtype=np.float64)
    m, d = L.shape
    mir = spm.CappedPlusMirror(capacity=capacity, gamma=gamma, eta=eta)
    mir.L, mir.c, mir.P = L.copy(), np.asarray(coeff, dtype=np.float64).copy(), np.asarray(Kinv, dtype=np.float64).reshape(m, m).copy()
    rng = np.random.default_rng(seed)
    props, branches = np.zeros((n, 18)), []
    inp = None
    for i in range(n):
        if inp is None:      # (Kinv and the landmarks changed: the candidates are formed anew)
            inp = um.PlusInputs(mir.P, mir.L, gamma, eta, n_prbs, tries=min(mir.m, 24))
            want = list(um.cases_required(mir.m)) or ['branch4']
        if i in insert_at:
            x, y = _inserting(mir, n_prbs, rng, eta, clearance)
        else:
            mistake = i % 6 == 5
            order = (['branch0'] if mistake else []) + [want[i % len(want)]] + want
            x = None
            for case in order:
                got = inp.pick(mir.c, case)
                if got is None:
                    continue
                x, y = got
                if mistake:      # the case's sample with the other label, where the learner projects it
                    mir.predict(x)
                    if mir.m < capacity and mir._project()[1] > eta - 1e-3:
                        x = None
                        continue
                    y = -y
                break
            if x is None:
                j = int(rng.integers(mir.m))
                x = mir.L[j].copy()
                x[:d - 1] = x[:d - 1].astype(np.float32)
                _, f = mir.predict(x)
                y = 1 if f > 0 else -1
        c = int(round(x[d - 1] * n_prbs))
        props[i, 0], props[i, 1] = 7 * i + 3, shm.proposal_word(c, y)
        props[i, 2:2 + d - 1] = x[:d - 1]
        xs = np.append(x[:d - 1], float(c) / float(n_prbs))
        mir.predict(xs)
        m0 = mir.m
        branches.append(int(mir.update(xs, y)[0]))
        if mir.m != m0:
            inp = None
    return props, branches
