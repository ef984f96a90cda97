"""A float64 restatement of the reference's KBRL_Control.select_action (kbrl_control.py:41-73 over algorithms/kernel.py:13-28)
on FINISHED dictionaries, with every sum in longdouble: the yardstick of tests/test_agent_file.py (which holds it to what the
reference itself recorded) and of tests/test_gpu_agent_file.py (which holds imported agents on the device to it).

Per candidate c = 0 .. n_prbs and learner s:  x = (state[indexes_s], c / n_prbs),  k_j = exp(-gamma |l_j - x|^2),
f(c) = sum_j k_j coeff_j,  and the tolerance of that number, TOL = 1e-9 (1 + sum_j |k_j coeff_j|).  The first candidate with
f > 0 is taken (an exact zero would draw, kernel.py:26-27: nothing here can restate a draw, the margin check excludes it)."""
import os

import numpy as np

FIXTURES = ('g10_kbrl_s0', 'g10_kbrl_s2', 'g15_kbrl_long_s0', 'g16_kbrl_long_tdl_s0')
GAMMA, ETA, ALFA = 1.0, 0.1, 0.05   # scenario_creator.py:218, projectron.py:25, scenario_creator.py:187
TOL = 1e-9


class Fixture:
    """a recorded run of the reference: final dictionaries, the control state of its last step, the recorded states"""

    def __init__(self, golden_dir, name):
        g = np.load(os.path.join(golden_dir, name + '.npz'), allow_pickle=True)
        self.name = name
        self.S = int(g['action_out'].shape[1])
        self.landmarks = [np.asarray(g['landmarks%d' % s], dtype=np.float64) for s in range(self.S)]
        self.coeff = [np.asarray(g['coeff%d' % s], dtype=np.float64) for s in range(self.S)]
        self.dims = [lm.shape[1] - 1 for lm in self.landmarks]
        self.n_prbs = int(g['acc'].shape[2])
        self.state = np.asarray(g['state'], dtype=np.float32)
        self.final_state = np.asarray(g['final_state'], dtype=np.float32)
        self.security = np.asarray(g['security'][-1], dtype=np.int32)
        self.margins = np.asarray(g['margins'][-1], dtype=np.int32)
        self.action = np.asarray(g['action_out'][-1], dtype=np.int32)
        self.adjusted = int(g['adjusted'][-1])
        self.acc = np.asarray(g['acc'][-1], dtype=np.float64)
        self.a_range = tuple(float(v) for v in g['a_range'])
        assert sum(self.dims) == self.state.shape[1]

    def config(self, capacity=None):
        largest = max(lm.shape[0] for lm in self.landmarks)
        return dict(n_prbs=self.n_prbs, capacity=capacity or max(64, (largest + 63) // 64 * 64), dims=self.dims, alfa=ALFA,
                    accuracy_range=self.a_range, gamma=GAMMA, eta=ETA)

    def agent(self, seed=0):
        """the arrays agent_file.pack takes: control state from the last recorded step"""
        return dict(landmarks=self.landmarks, coeff=self.coeff, action=self.action, security_factors=self.security,
                    margins=self.margins, adjusted=self.adjusted, accuracies=self.acc, seed=seed)


def scores(landmarks, coeff, x_state, n_prbs, gamma=GAMMA):
    """-> (f [n_prbs + 1], tol [n_prbs + 1]) of one learner on one state, as longdouble sums"""
    n = n_prbs
    f, tol = np.zeros(n + 1, dtype=np.longdouble), np.full(n + 1, TOL, dtype=np.longdouble)
    m = landmarks.shape[0]
    if m == 0:
        return f, tol
    co = coeff.astype(np.longdouble)
    xs = np.asarray(x_state, dtype=np.float64)
    d_state = (((landmarks[:, :-1] - xs[None, :]) ** 2).astype(np.longdouble)).sum(axis=1)
    for c in range(n + 1):
        d_last = ((landmarks[:, -1] - c / n) ** 2).astype(np.longdouble)
        k = np.exp(-np.longdouble(gamma) * (d_state + d_last))
        if m == 1:
            k = k.astype(np.float32).astype(np.longdouble)   # (kernel.py:16: one landmark's kernel value is a float32)
        terms = k * co
        f[c] = terms.sum()
        tol[c] = TOL * (1 + np.abs(terms).sum())
    return f, tol


def select_action(fx_or_parts, state, security=None):
    """kbrl_control.py:41-73 -> dict(action, adjusted, margins, found [S] = the candidate each learner stopped at (n_prbs when
    none predicted 1), f [S, n + 1], tol [S, n + 1], ratio [S] = min over the SCANNED candidates of |f| / tol)"""
    fx = fx_or_parts
    n, S = fx.n_prbs, fx.S
    security = fx.security if security is None else security
    action, margins, found = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    F, T, ratio = np.zeros((S, n + 1), dtype=np.longdouble), np.zeros((S, n + 1), dtype=np.longdouble), np.zeros(S)
    at = 0
    for s in range(S):
        x = np.asarray(state[at:at + fx.dims[s]], dtype=np.float32)
        at += fx.dims[s]
        f, tol = scores(fx.landmarks[s], fx.coeff[s], x, n)
        F[s], T[s] = f, tol
        l1, margin = n, 0
        pos = np.nonzero(f > 0)[0] if fx.landmarks[s].shape[0] else np.zeros(0, dtype=np.int64)
        if pos.size:
            l1 = int(pos[0])
            a = min(n, l1 + int(security[s]))
            margin = a - l1
            found[s], action[s] = l1, a
        else:
            found[s], action[s] = n, n
        margins[s] = margin
        scanned = slice(0, (int(pos[0]) if pos.size else n) + 1)
        ratio[s] = float((np.abs(f[scanned]) / tol[scanned]).min()) if fx.landmarks[s].shape[0] else np.inf
    adjusted = 0
    assigned = int(action.sum())
    if assigned > n:
        adjusted = 1
        new = np.array([np.floor(n * p) for p in action / assigned], dtype=np.int64)
        margins = margins - (action - new)
        action = new
    return dict(action=action, adjusted=adjusted, margins=margins, found=found, f=F, tol=T, ratio=ratio)
