"""Hand-made learners and control-step rows for tests/test_gpu_control_plus_batch.py (pure NumPy, no GPU): dictionaries of an exact
size, and rows whose insertions fall where the group walk has its seams.  Nothing here is random.

A LINE LEARNER of size m holds the landmarks (7 i, 0, .., 0 | allocation 0 where i is even, 1 where it is odd), i = 0 .. m - 1, with
coefficients +1, -1, +1, ..: its pre-growth stream (line_samples) alternates the label, each sample lies 7 away from its only
neighbour (kernel value below e^-49 = 5e-22), so each one is a mistake with delta = 1 and is inserted -- m samples, m landmarks,
whatever the rounding.  A row at the FRESH state 7 m sees a far field of the sign of the last coefficient and of magnitude 5e-22:
a row labelled against it inserts its first candidate, and every later candidate of the row lies inside the margin of that new
landmark with loss < delta / eta (k(t) = exp(-t^2): 1 - k < 10 (1 - k^2) for every t), so the rule writes nothing more.  A row at
the MIDPOINT 7 (m - 1.5) of the last two landmarks -- one +1 at allocation 0, one -1 at allocation 1, both at distance 3.5 --
sees f(a) = e^-12.25 (k(a / n) - k(1 - a / n)): positive below n / 2, negative above (n_prbs is odd: no candidate has f = 0).
Labelled +1 and started at `action`, its candidates up to n / 2 lie inside the margin with delta = 1 (nothing is written) and the
first one behind is a mistake with delta = 1: an insertion at position (n + 1) / 2 - action of the row, wherever the test wants
it in a group.  No decision is closer to its threshold than the far field is to zero, and that is a sign, not a magnitude."""
import numpy as np

STEP = 7.0


def line_samples(m, d):
    """the pre-growth stream of a line learner of d state variables: X [m, d + 1], y [m]"""
    X = np.zeros((m, d + 1))
    X[:, 0] = STEP * np.arange(m)
    X[:, d] = np.arange(m) % 2
    return X, np.where(np.arange(m) % 2 == 0, 1, -1).astype(np.int8)


def last_sign(m):
    """the coefficient of a line learner's last landmark (an empty one counts as -1)"""
    return 1 if m > 0 and (m - 1) % 2 == 0 else -1


def line_state(i, d):
    s = np.zeros(d, dtype=np.float32)
    s[0] = STEP * i
    return s


def fresh_row(i, d, n_prbs, far_sign, action_if_plus):
    """the row at the fresh state 7 i labelled against a far field of sign far_sign: label -1 spans all candidates 0 .. n_prbs"""
    return (line_state(i, d), action_if_plus, 1) if far_sign < 0 else (line_state(i, d), n_prbs, -1)


def seam_rows(m, d, n_prbs, pos):
    """four rows (state [d], action, label) for a line learner of size m (n_prbs odd):
      1. at the fresh state 7 m, labelled against the far field: its FIRST candidate is inserted -- one by one while m < 2 (and
         the row enters grouping behind it when that made m = 2), as the first column of a group otherwise;
      2. m >= 2: at the midpoint of the last two landmarks, label +1 from allocation (n_prbs + 1) / 2 - pos: an insertion at
         position pos of the row's first group.  m < 2: another fresh row, at 7 (m + 1);
      3. row 1 again: its first candidate is a landmark now (f = 1.0), the others stay inside its margin;
      4. row 2 again."""
    r1 = fresh_row(m, d, n_prbs, last_sign(m), n_prbs - 11)
    if m >= 2:
        r2 = (line_state(m - 1.5, d), (n_prbs + 1) // 2 - pos, 1)
    else:
        r2 = fresh_row(m + 1, d, n_prbs, r1[2], n_prbs - 11)
    return [r1, r2, r1, r2]


def edge_rows(m, d, n_prbs=9):
    """rows of 1, 7, 8, 9 and 10 candidates for both labels on a line learner of size m (n_prbs = 9), each at a fresh state of its
    own and labelled against the far field, so that its first candidate is inserted and the others are walked in groups; the
    labels therefore alternate from row to row.  Behind the one-candidate row of label +1 the same row stands AGAIN: its only
    candidate is now a landmark with coefficient +1 and a far field below 1e-21, f is 1.0 exactly, and the row's one group is
    skipped.  -> list of (state, action, label), and the index of that repeated row"""
    rows, y, i, again = [], -last_sign(m), m, None
    want = [(c, lab) for c in (1, 7, 8, 9, 10) for lab in (1, -1)]
    while want:
        c = next(c for c, lab in want if lab == y)
        want.remove((c, y))
        act = n_prbs + 1 - c if y == 1 else c - 1
        rows.append((line_state(i, d), act, y))
        if c == 1 and y == 1:
            rows.append((line_state(i, d), act, y))
            again = len(rows) - 1
        i += 1
        y = -y
    return rows, again
