"""A plain NumPy restatement of KBRL_Control's closed loop (kbrl_control.py:41-114: select_action, adjust_action,
update_control) over tests/plus_mirror.py's learners, as the device runs it in Projectron++ mode (kb_control_plus.hip, DESIGN.md
§8l).  It imports nothing of the project but that mirror: tests/test_control_plus_mirror.py replays the reference's recording
G19 through it, which pins the recording and the prose of the mode to each other without a GPU.

update_control, per learner in order: f at the executed allocation and its decision (an exact tie against a populated dictionary
draws); the hit; the accuracy table under the margins and `adjusted` of the last select_action; the security factor; then the
augmentation range in the reference's order -- a = action .. n_prbs on +1, 0 .. action on -1 -- every candidate through predict
and the margin rule's update."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from plus_mirror import PlusMirror   # noqa: E402


class ControlMirror:
    def __init__(self, dims, n_prbs, initial_action, security_factor, alfa=0.05, accuracy_range=(0.99, 0.999), gamma=1.0, eta=0.1,
                 plus=True, tie=None):
        self.dims, self.n = list(dims), int(n_prbs)
        self.off = np.concatenate([[0], np.cumsum(self.dims)])
        self.learners = [PlusMirror(gamma=gamma, eta=eta, plus=plus) for _ in self.dims]
        S = len(self.dims)
        self.alfa, self.lo = alfa, accuracy_range[0]
        self.accuracies = np.full((S, self.n), (accuracy_range[0] + accuracy_range[1]) / 2)   # kbrl_control.py:38-39
        self.security = np.asarray(security_factor, dtype=np.int64).copy()
        self.margins = np.zeros(S, dtype=np.int64)
        self.action = np.asarray(initial_action, dtype=np.int64).copy()
        self.adjusted = 0
        self.tie = tie
        self.branches = [[] for _ in self.dims]   # per learner, per sample of the augmentation
        self.f0 = []                              # per step: f at the executed allocation

    def _x(self, state, s, a):
        return np.append(np.asarray(state[self.off[s]:self.off[s + 1]], dtype=np.float64), a / self.n)

    def select_action(self, state):
        """kbrl_control.py:41-73 -> (action, adjusted): per learner the first allocation predicted +1, plus the security factor,
        capped at n_prbs; all of them scaled down together when they exceed the cell"""
        S = len(self.dims)
        action, margins = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
        for s, h in enumerate(self.learners):
            found = -1
            for a in range(self.n + 1):
                y, _ = h.predict(self._x(state, s, a), tie=self.tie)
                if y == 1:
                    found = a
                    break
            if found >= 0:
                action[s] = min(self.n, found + self.security[s])
                margins[s] = action[s] - found
            else:
                action[s] = self.n
        adjusted = 0
        assigned = int(action.sum())
        if assigned > self.n:
            adjusted = 1
            new = np.array([np.floor(self.n * (a / assigned)) for a in action]).astype(np.int16).astype(np.int64)
            margins = (margins - (action - new)).astype(np.int16).astype(np.int64)
            action = new
        self.action, self.margins, self.adjusted = action, margins, adjusted
        return action.copy(), adjusted

    def update_control(self, state, action, labels):
        """kbrl_control.py:80-114 -> hits"""
        S = len(self.dims)
        hits, f0 = np.zeros(S, dtype=np.int64), np.zeros(S)
        for s, h in enumerate(self.learners):
            a_i, y = int(action[s]), int(labels[s])
            y_pred, f0[s] = h.predict(self._x(state, s, a_i), tie=self.tie)
            hit = int(y == y_pred)
            margin = max(0, int(self.margins[s]))
            acc = self.accuracies[s]
            if y_pred == 1:
                if not hit:
                    acc[:margin + 1] = (1 - self.alfa) * acc[:margin + 1]
                else:
                    acc[margin:] = (1 - self.alfa) * acc[margin:] + self.alfa
            if not self.adjusted:
                self.security[s] = int(np.argmax(acc > self.lo))
            hits[s] = hit
            for a in (range(a_i, self.n + 1) if y == 1 else range(0, a_i + 1)):
                x = self._x(state, s, a)
                h.predict(x, tie=self.tie)
                self.branches[s].append(h.update(x, y)[0])
        self.f0.append(f0)
        return hits
