"""The group walk of the closed control loop's Projectron++ update phase (kb_control_plus_batch.hip) restated in
NumPy over tests/control_plus_mirror.py.  It imports nothing of the project but that mirror.

Per learner and step the candidates a0 .. a1 are walked from position p:
  1. fewer than two landmarks, or more than max_landmarks: candidate p goes one by one (predict, update), p advances by one;
  2. otherwise the group is p .. min(p + width - 1, a1): its K_f columns, and each candidate's f from them and the coefficients
     as they are at group start;
  3. nobody of the group inside the margin (y f >= 1 for all): no pass, every candidate is branch 0;
  4. otherwise every column's d* (and with it delta) is formed from the Kinv AT GROUP START, by the per-column call the ungrouped
     mirror uses (PlusMirror._project);
  5. the group is walked in order: f again with the coefficients as they are, the decision, the rule with THAT column's d*; an
     insertion ends the group behind itself.
width = 0 walks every candidate one by one and counts nothing: the ungrouped replay, with the per-sample f recorded.

expected_work computes kb_control_plus_batch_info's work[0..7] from a recording alone (branches per sample, sizes at its start)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from control_plus_mirror import ControlMirror   # noqa: E402


def _tiles(m):
    nb = (m + 63) // 64
    return nb * (nb + 1) // 2


class BatchControlMirror(ControlMirror):
    def __init__(self, *a, width=8, max_landmarks=1024, **kw):
        super().__init__(*a, **kw)
        self.width, self.max_landmarks = int(width), int(max_landmarks)
        self.work = [0] * 8
        self.f = [[] for _ in self.dims]   # per learner, per sample of the augmentation: the f its decision was taken on

    def _one(self, h, s, x, y):
        _, f = h.predict(x, tie=self.tie)
        br = h.update(x, y)[0]
        self.branches[s].append(br)
        self.f[s].append(f)
        return br

    def _walk(self, h, s, state, cands, y):
        W, p = self.width, 0
        while p < len(cands):
            m = h.m
            if W == 0 or m < 2 or m > self.max_landmarks:
                br = self._one(h, s, self._x(state, s, cands[p]), y)
                if W:
                    self.work[6] += 1
                    self.work[7] += br != 0
                p += 1
                continue
            xs = [self._x(state, s, a) for a in cands[p:p + W]]
            g = len(xs)
            self.work[0] += 1
            cols = []
            for x in xs:   # K_f and f at group start (no draw here: the decision is taken in the walk)
                _, f = h.predict(x, tie=None)
                cols.append((f, h.kf))
            if all(y * f >= 1 for f, _ in cols):
                self.work[1] += 1
                for f, _ in cols:
                    self.branches[s].append(0)
                    self.f[s].append(f)
                p += g
                continue
            self.work[2] += 1
            self.work[3] += _tiles(m)
            self.work[4] += g
            proj = []
            for _, kf in cols:   # d* and delta of every column from the Kinv at group start
                h.kf = kf
                proj.append(h._project())
            cut = None
            for w, x in enumerate(xs):
                _, f = h.predict(x, tie=self.tie)   # f with the coefficients as they are
                h._project = lambda w=w: proj[w]
                try:
                    br = h.update(x, y)[0]
                finally:
                    del h._project
                self.branches[s].append(br)
                self.f[s].append(f)
                if h.m > m:
                    cut = w
                    break
            if cut is None:
                p += g
            else:
                self.work[5] += g - 1 - cut
                p += cut + 1

    def update_control(self, state, action, labels):
        """ControlMirror.update_control with the augmentation loop replaced by the walk"""
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
            self._walk(h, s, state, list(range(a_i, self.n + 1) if y == 1 else range(0, a_i + 1)), y)
        self.f0.append(f0)
        return hits


def expected_work(branches, sizes, actions, labels, width, max_landmarks, n_prbs=200, insertions=None):
    """work[0..7] of kb_control_plus_batch_info for a recording: branches[s] the branch of every sample of learner s in order,
    sizes[s] its dictionary size at the start, actions / labels [steps][S] the rows.  A dictionary grows by one with every branch
    2 and never otherwise; a group is skipped iff all its recorded branches are 0 and cut iff it holds a branch 2.  insertions: a
    list that receives (learner, step, size before, position in its group, size of the group) of every insertion -- position
    and size -1 for one that went one by one."""
    work = [0] * 8
    actions, labels = np.asarray(actions), np.asarray(labels)
    for s in range(actions.shape[1]):
        br, at, m = np.asarray(branches[s]), 0, int(sizes[s])
        for t in range(actions.shape[0]):
            a, lab = int(actions[t, s]), int(labels[t, s])
            cnt = n_prbs - a + 1 if lab == 1 else a + 1
            row = br[at:at + cnt]
            assert len(row) == cnt, (s, t, len(row), cnt)
            at += cnt
            p = 0
            while p < cnt:
                if m < 2 or m > max_landmarks:
                    work[6] += 1
                    work[7] += int(row[p] != 0)
                    if row[p] == 2 and insertions is not None:
                        insertions.append((s, t, m, -1, -1))
                    m += int(row[p] == 2)
                    p += 1
                    continue
                grp = row[p:p + width]
                work[0] += 1
                if (grp == 0).all():
                    work[1] += 1
                    p += len(grp)
                    continue
                work[2] += 1
                work[3] += _tiles(m)
                work[4] += len(grp)
                ins = np.nonzero(grp == 2)[0]
                if len(ins):
                    work[5] += len(grp) - 1 - int(ins[0])
                    if insertions is not None:
                        insertions.append((s, t, m, int(ins[0]), len(grp)))
                    m += 1
                    p += int(ins[0]) + 1
                else:
                    p += len(grp)
        assert at == len(br), (s, at, len(br))
    return work
