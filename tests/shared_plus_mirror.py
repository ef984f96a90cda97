"""The shared-dictionary learning step under the margin rule (kb_set_shared_plus; csrc/kb_kbrl.hip:
shared_scan_plus_kernel, apply_full_batch<true>, shared_apply_plus_kernel) restated beside tests/shared_mirror.py, whose stages it
reuses where the switch changes nothing (KF, DS, F0, A, collect, commit).  Used by tests/test_shared_plus_mirror.py (CPU) and
tests/test_gpu_shared_plus.py (device).  Not a test module.

  scan_plus           shared_mirror.scan with the proposal rule f y < 1 in the place of f y <= 0; the hit of round 0 is the sign's.
  full_batch_plus     a list against a dictionary at its capacity: shared_mirror.full_batch's KF, DS, F0 and A, and the walk
                        f_p = F0_p + g_p (one rounded sum), margin = y_p f_p (exact)
                        margin >= 1                      branch 0
                        margin <= 0                      branch 1: w_p = y_p; saturation when max(1 - A[p][p], 0) > eta
                        else  delta = max(1 - A[p][p], 0), norm = max(1 - delta, 0), loss = 1 - margin, slack = loss - delta / eta
                              not slack > 0              branch 4
                              else                       branch 3: alpha = loss / norm, then 1.0 where 1.0 < alpha, then
                                                         (2 slack) / norm where that is < alpha; w_p = alpha y_p (exact)
                        applied (1, 3): g_q <- fma(w_p, A[q][p], g_q) for q > p; coeff <- coeff + w_p DS[p] (product, then sum)
  growing_apply_plus  a list against a dictionary that can still grow, one by one: f = um.score(column, coeff); where f y < 1 the
                      margin step with d* by the column walk (um.step_plus's statements; its mistakes are um.step(order='col')).
  PlusRounds          shared_mirror.OracleRounds' protocol with one plus_mirror.PlusMirror per slice as the sequential learner.

Two deliberately WRONG walks for the tests of the tests (full_batch_plus(wrong=...)): 'weight_y' weights a margin step with y
instead of alpha y; 'loss_f0' forms the loss from F0_p alone, without g_p."""
import numpy as np

import plus_mirror
import shared_mirror as shm
import update_mirror as um

WRONG = ('weight_y', 'loss_f0')


def scan_plus(f, y, a_i, cursor, rnd, n_prbs, m=1):
    """as shared_mirror.scan -> dict(cstar, cursor, hit): cstar = the first candidate of the range with f y < 1"""
    c_to = n_prbs if y == 1 else a_i
    c_from = (a_i if y == 1 else 0) if rnd == 0 else cursor
    hit = None
    if rnd == 0:
        f0 = f[a_i] if m > 0 else 0
        assert m == 0 or f0 != 0, 'f(a_i) == 0 draws from the tie-break stream: not a case of these tests'
        hit = int(m > 0 and (1 if f0 > 0 else -1) == y)
    elif not (0 <= c_from <= c_to):
        return dict(cstar=-1, cursor=-1, hit=None)
    cstar = -1
    for c in range(c_from, c_to + 1):
        if f[c] * y < 1:
            cstar = c
            break
    return dict(cstar=cstar, cursor=cstar if cstar >= 0 else -1, hit=hit)


def margin_weight(margin, dg, eta, loss32=False):
    """the walk's decision on margin = y f and the Gram block's diagonal dg = A[p][p] -> dict(branch, alpha (the weight is alpha y),
    delta, norm, loss, slack, terms, sat); what a branch does not form is NaN.  loss32: the float32 loss of the single-landmark
    regime (the one-by-one path only; a dictionary at its capacity holds two landmarks at least)"""
    nan = float('nan')
    out = dict(branch=0, alpha=0.0, delta=nan, norm=nan, loss=nan, slack=nan, terms=None, sat=False)
    if margin >= 1.0:
        return out
    delta = 1.0 - dg
    delta = delta if delta > 0.0 else 0.0
    out['delta'] = delta
    if margin <= 0.0:
        out.update(branch=1, alpha=1.0, sat=delta > eta)
        return out
    norm = 1.0 - delta
    norm = norm if norm > 0.0 else 0.0
    loss = float(np.float32(1.0) - np.float32(margin)) if loss32 else 1.0 - margin
    slack = loss - delta / eta
    out.update(norm=norm, loss=loss, slack=slack)
    if not slack > 0.0:
        out['branch'] = 4
        return out
    with np.errstate(divide='ignore', invalid='ignore'):
        by_loss, by_slack = float(um.div(loss, norm)), float(um.div(2.0 * slack, norm))
    alpha = by_loss
    if 1.0 < alpha:
        alpha = 1.0
    if by_slack < alpha:
        alpha = by_slack
    out.update(branch=3, alpha=alpha, terms=(by_loss, 1.0, by_slack))
    return out


def full_batch_plus(Kinv, coeff, landmarks, props, gamma, n_prbs, eta=0.1, count=None, wrong=None):
    """-> dict(KF, DS, F0, A, f [np] = the f_p the walk decided on, branch [np] in 0 .. 4, w [np] = the weights (0.0 where nothing
    was applied), n_changed, n_work (branches 1-4), sat, coeff, y, terms [np] (branch 3: the three terms of alpha))"""
    assert wrong is None or wrong in WRONG
    base = shm.full_batch(Kinv, coeff, landmarks, props, gamma, n_prbs, eta, count=count)
    KF, DS, F0, A, y = base['KF'], base['DS'], base['F0'], base['A'], base['y']
    n = len(F0)
    g, f, w = np.zeros(n), np.zeros(n), np.zeros(n)
    branch = np.zeros(n, dtype=np.int32)
    terms = [None] * n
    c = np.asarray(coeff, dtype=np.float64).copy()
    sat = False
    for p in range(n):
        f[p] = F0[p] + g[p]
        yp = float(y[p])
        d = margin_weight(yp * f[p], A[p, p], eta)
        if wrong == 'loss_f0' and d['branch'] in (3, 4):
            d = margin_weight(yp * F0[p], A[p, p], eta)
            if d['branch'] not in (3, 4):      # (F0 alone falls outside the margin: keep the right decision, weight as a mistake)
                d = dict(d, branch=3, alpha=1.0)
        branch[p], terms[p] = d['branch'], d['terms']
        sat = sat or d['sat']
        if d['branch'] in (1, 3):
            w[p] = yp if (wrong == 'weight_y') else d['alpha'] * yp
            if p + 1 < n:
                g[p + 1:] = um.fma(w[p], A[p + 1:, p], g[p + 1:])
            c = c + w[p] * DS[p]
    return dict(KF=KF, DS=DS, F0=F0, A=A, f=f, branch=branch, w=w, n_changed=int(((branch == 1) | (branch == 3)).sum()),
                n_work=int((branch > 0).sum()), sat=bool(sat), coeff=c, y=y, terms=terms)


def exact_f_plus(coeff, KF, w, ex):
    """the walk's f_p of the SAME doubles in longdouble with the walk's own weights w (full_batch_plus's; 0.0 where nothing was
    applied): f_p = k_p . coeff_0 + sum_{q < p} w_q A[p][q], and the bound of the device's f_p as shared_mirror.exact_full_batch
    derives it for weights of +-1 -- the fused multiply-add rounds once whatever w_q is, and |w_q| <= 1 scales every term of the
    bound down, so it carries over with |w_q| in the place of 1.  ex: exact_full_batch's result for the same list (A, EA).
    -> (f [np], Ef [np]) as longdouble"""
    ld = np.longdouble
    KF = np.asarray(KF, dtype=np.float64)
    n, m = KF.shape
    ue = ld(shm.U * (1.0 + 2.0 ** -10))
    F = um.f_units(m) + um.exact_units(m)
    kl, c0 = KF.astype(ld), np.asarray(coeff, dtype=np.float64).astype(ld)
    f0 = kl @ c0
    E0 = ld(F) * ue * (np.abs(kl) @ np.abs(c0))
    wl = np.asarray(w, dtype=np.float64).astype(ld)
    f, Ef = np.zeros(n, dtype=ld), np.zeros(n, dtype=ld)
    for p in range(n):
        q = np.nonzero(wl[:p] != 0)[0]
        g = (wl[q] * ex['A'][p, q]).sum()
        aw = np.abs(wl[q])
        Eg = (aw * ex['EA'][p, q]).sum() + ld(len(q)) * ue * (aw * (np.abs(ex['A'][p, q]) + ex['EA'][p, q])).sum()
        f[p] = f0[p] + g
        Ef[p] = E0[p] + Eg + ue * (abs(f[p]) + E0[p] + Eg)
    return f, Ef


def step_plus_col(Kinv, coeff, landmarks, x, y, gamma=1.0, eta=0.1, capacity=None):
    """um.step_plus as a handle that stores both triangles of Kinv runs it: d* by the column walk in the margin case as well ->
    dict(f, branch, delta, coeff, kinv, landmarks, m, alpha, terms)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    m = len(coeff)
    x = np.asarray(x, dtype=np.float64)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, len(x))
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    kf = um.column(L, x, gamma) if m else np.zeros(0)
    f = um.score(kf, coeff)
    margin = float(y) * f
    if margin >= 1.0 or margin <= 0.0:
        st = um.step_plus(Kinv, coeff, L, x, y, gamma, eta, capacity, order='col')
        return dict(f=f, branch=st['branch'], delta=st['delta'], coeff=st['coeff'], kinv=st['kinv'], landmarks=st['landmarks'],
                    m=st['m'], alpha=float('nan'), terms=None)
    if m == 1:
        ds = np.array([float(np.float32(1.0) * np.float32(kf[0]))])
        dt = float(np.float32(ds[0]) * np.float32(kf[0]))
    else:
        ds = um.dstar_col(Kinv, kf)
        dt = um.dot(ds, kf)
    d = margin_weight(margin, dt, eta, loss32=m == 1)
    nc = coeff.copy()
    if d['branch'] == 3:
        nc = coeff + (d['alpha'] * float(y)) * ds
        if m == 1:
            nc = nc.astype(np.float32).astype(np.float64)
    return dict(f=f, branch=d['branch'], delta=d['delta'], coeff=nc, kinv=Kinv.copy(), landmarks=L.copy(), m=m, alpha=d['alpha'],
                terms=d['terms'])


def growing_apply_plus(Kinv, coeff, landmarks, props, gamma, n_prbs, d, eta=0.1, capacity=None, count=None):
    """the list applied one by one under the margin rule -> dict(f [np], branch [np] in 0 .. 4, kinv, coeff, landmarks, m)"""
    coeff = np.asarray(coeff, dtype=np.float64)
    m = len(coeff)
    n = len(props) if count is None else count
    P = np.asarray(props, dtype=np.float64)
    f, branch = np.zeros(n), np.zeros(n, dtype=np.int32)
    Kinv = np.asarray(Kinv, dtype=np.float64).reshape(m, m)
    L = np.asarray(landmarks, dtype=np.float64).reshape(m, d)
    for p in range(n):
        w = int(P[p, 1])
        y = 1 if w & 1 else -1
        x = np.append(P[p, 2:2 + d - 1], float(w >> 2) / float(n_prbs))
        st = step_plus_col(Kinv, coeff, L, x, y, gamma, eta, capacity)
        f[p], branch[p] = st['f'], st['branch']
        Kinv, coeff, L = st['kinv'], st['coeff'], st['landmarks']
    return dict(f=f, branch=branch, kinv=Kinv, coeff=coeff, landmarks=L, m=len(coeff))


def near_threshold(mir, x, y, clearance):
    """whether the sequential learner `mir` (a PlusMirror) decides sample (x, y) within `clearance` of one of the rule's thresholds:
    the margin against 0 and 1, the slack against 0, the terms of alpha against each other.  Leaves the learner as it was."""
    _, f = mir.predict(x)
    margin = y * f
    if abs(margin) < clearance or abs(margin - 1.0) < clearance:
        return True
    if not 0.0 < margin < 1.0:
        return False
    _, delta = mir._project()
    norm = max(1.0 - delta, 0.0)
    loss = 1.0 - margin
    slack = loss - delta / mir.eta
    if abs(slack) < clearance:
        return True
    if slack <= 0.0 or norm == 0.0:
        return False
    t = sorted([loss / norm, 1.0, 2.0 * slack / norm])
    return t[1] - t[0] < clearance


class CappedPlusMirror(plus_mirror.PlusMirror):
    """PlusMirror with the fixed-budget reading of the device: at `capacity` landmarks a mistake is projected whatever its delta"""

    def __init__(self, capacity=None, **kw):
        super().__init__(**kw)
        self.capacity = capacity

    def update(self, x, y):
        if self.capacity is not None and self.m >= self.capacity and int(y) * self.f <= 0:
            ds, delta = self._project()
            self.c = self.c + int(y) * ds
            return 1, delta, np.nan
        return super().update(x, y)


class PlusRounds:
    """ONE sequential PlusMirror per slice beside the rounds of a shared step under the margin rule (shared_mirror.OracleRounds'
    protocol): the scan is taken from the learners' dictionaries as they stand (shm.plain_scores, scan_plus), the merged lists are
    fed in order through predict and update.  `open` counts the (replica, slice) pairs a scan left out because a candidate at or
    before the proposal scored within 1e-9 (1 + scale) of 0 or of y (an empty dictionary scores exactly 0.0: every candidate is
    proposed); `near` counts the applied samples near_threshold() names."""

    def __init__(self, dims, n_prbs, n_envs, gamma, eta, clearance=um.CLEARANCE):
        self.dims, self.n_prbs, self.N, self.gamma = list(dims), n_prbs, n_envs, gamma
        self.off = np.cumsum([0] + self.dims)[:-1]
        self.oa = [plus_mirror.PlusMirror(gamma=gamma, eta=eta, plus=True) for _ in dims]
        self.clearance = clearance
        self.open = self.pairs = self.near = self.samples = 0

    def begin(self, states, actions, labels):
        self.states = np.asarray(states, dtype=np.float32)
        self.actions, self.labels = np.asarray(actions), np.asarray(labels)
        self.cursor = np.zeros((self.N, len(self.dims)), dtype=np.int64)
        self.round = 0

    def scan(self):
        """-> (cstar [N, S], hits [N, S] (round 0; else None), left_out [N, S] bool); self.n_pred as OracleRounds counts it"""
        self.n_pred = 0
        S = len(self.dims)
        cstar = np.full((self.N, S), -1, dtype=np.int64)
        hits = np.zeros((self.N, S), dtype=np.int64) if self.round == 0 else None
        out = np.zeros((self.N, S), dtype=bool)
        for s in range(S):
            o = self.oa[s]
            m = o.m
            L, co = (o.L, o.c) if m else (np.zeros((0, self.dims[s] + 1)), np.zeros(0))
            for e in range(self.N):
                x = self.states[e, self.off[s]:self.off[s] + self.dims[s]]
                f, sc = shm.plain_scores(L, co, x, self.n_prbs, self.gamma)
                y, a_i = int(self.labels[e, s]), int(self.actions[e, s])
                c_from = (a_i if y == 1 else 0) if self.round == 0 else int(self.cursor[e, s])
                r = scan_plus(f, y, a_i, int(self.cursor[e, s]), self.round, self.n_prbs, m)
                cstar[e, s], self.cursor[e, s] = r['cstar'], r['cursor']
                c_to = self.n_prbs if y == 1 else a_i
                if 0 <= c_from <= c_to:
                    self.n_pred += (r['cstar'] if r['cstar'] >= 0 else c_to) - c_from + 1
                if self.round == 0:
                    hits[e, s] = r['hit']
                    self.n_pred += 1
                if m and (self.round == 0 or 0 <= c_from <= c_to):
                    tol = 1e-9 * (1.0 + sc)
                    last = r['cstar'] if r['cstar'] >= 0 else c_to
                    near1 = np.abs(f * y - 1.0) <= tol
                    out[e, s] = bool(near1[max(c_from, 0):last + 1].any()) or (self.round == 0 and bool(abs(f[a_i]) <= tol[a_i]))
                self.pairs += 1
        self.open += int(out.sum())
        self.cstar = cstar
        return cstar, hits, out

    def apply(self, lists):
        """lists: per slice [(replica, candidate)] in order -> per slice [(f, branch)]"""
        res = []
        for s, lst in enumerate(lists):
            o, rows = self.oa[s], []
            for e, c in lst:
                x = np.append(self.states[e, self.off[s]:self.off[s] + self.dims[s]].astype(np.float64), float(c) / float(self.n_prbs))
                y = int(self.labels[e, s])
                self.samples += 1
                self.near += int(o.m > 0 and near_threshold(o, x, y, self.clearance))
                _, f = o.predict(x)
                rows.append((f, o.update(x, y)[0]))
            res.append(rows)
        return res

    def commit(self, taken):
        self.cursor = shm.commit(self.cstar, taken, self.cursor)
        self.round += 1


# ------------------------------------------------------------------ the inputs of the tests (CPU and device use the same)
PLUS_CASES = [    # (landmarks of the full dictionary, state variables, proposals)
    (2, 10, 1), (63, 10, 15), (64, 10, 16), (65, 10, 17), (128, 10, 64), (256, 10, 256), (65, 3, 65)]


def plus_list(Kinv, coeff, landmarks, n_prbs, n, gamma=1.0, eta=0.1, seed=0):
    """a merged list of n proposals [n, 18] against a dictionary at its capacity, taken from update_mirror's case picker
    (um.PlusInputs: every case at least um.CLEARANCE from its thresholds) under the coefficients as the walk will hold them when
    the proposal's turn comes (the sequential PlusMirror beside it): the cases of um.cases_required in rotation, a mistake (a
    case's sample with the other label) every sixth proposal -> (props, cases [n] = the case's name, 'mistake', or 'any' where the
    picker found none and a landmark's own sample stands in)"""
    L = np.asarray(landmarks, dtype=np.float64)
    m, d = L.shape
    mir = CappedPlusMirror(capacity=m, gamma=gamma, eta=eta)
    mir.L, mir.c, mir.P = L.copy(), np.asarray(coeff, dtype=np.float64).copy(), np.asarray(Kinv, dtype=np.float64).reshape(m, m).copy()
    inp = um.PlusInputs(mir.P, L, gamma, eta, n_prbs, tries=min(m, 24))
    want = list(um.cases_required(m)) or ['branch4']
    props, cases = np.zeros((n, 18)), []
    rng = np.random.default_rng(seed)
    for i in range(n):
        case = want[i % len(want)]
        got = inp.pick(mir.c, case)
        if got is None:
            for case in want:
                got = inp.pick(mir.c, case)
                if got is not None:
                    break
        if got is None:
            j = int(rng.integers(m))
            x, y, case = L[j].copy(), 1, 'any'
            x[:d - 1] = x[:d - 1].astype(np.float32)
        else:
            x, y = got
        if i % 6 == 5:
            y, case = -y, 'mistake'
        c = int(round(x[d - 1] * n_prbs))
        props[i, 0], props[i, 1] = 7 * i + 3, shm.proposal_word(c, y)
        props[i, 2:2 + d - 1] = x[:d - 1]
        xs = np.append(x[:d - 1], float(c) / float(n_prbs))
        mir.predict(xs)
        mir.update(xs, y)
        cases.append(case)
    return props, cases
