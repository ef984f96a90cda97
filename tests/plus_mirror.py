"""A plain float64 NumPy restatement of the Projectron / Projectron++ update rule as the device applies it (kb_kbrl.hip:
predict_column, apply_update, apply_update_plus), with the float32 roundings of the single-landmark regime written out.  It imports
nothing of the project: tests/test_plus_mirror.py replays the reference's recording G18 through it, which pins the recording
and the rule's prose to each other without a GPU.

Branch codes: 0 nothing, 1 projection, 2 insertion, 3 margin update, 4 margin test without update."""
import numpy as np

f32 = np.float32


class PlusMirror:
    def __init__(self, gamma=1.0, eta=0.1, plus=True):
        self.gamma, self.eta, self.plus = gamma, eta, plus
        self.L = None               # landmarks [m, d]
        self.c = np.zeros(0)        # coefficients [m]
        self.P = np.zeros((0, 0))   # Kinv [m, m]
        self.f, self.kf = 0.0, np.zeros(0)

    @property
    def m(self):
        return len(self.c)

    def predict(self, x, tie=None):
        """-> (y_pred, f); tie() supplies the draw of an exact tie with a populated dictionary"""
        x = np.asarray(x, dtype=np.float64)
        if self.m == 0:
            self.f, self.kf = 0.0, np.zeros(0)
            return 0, 0.0
        k = np.exp(-self.gamma * ((self.L - x) ** 2).sum(axis=1))
        if self.m == 1:   # the kernel value, the coefficient and their product are float32
            k = k.astype(f32).astype(np.float64)
            f = float(f32(k[0]) * f32(self.c[0]))
        else:
            f = float(k @ self.c)
        self.f, self.kf = f, k
        y = int(np.sign(f))
        if y == 0:
            y = int(tie()) if tie is not None else 0
        return y, f

    def _project(self):
        """d* = Kinv K_f and delta = max(1 - d* . K_f, 0); float32 operands while one landmark is held"""
        if self.m == 0:
            return np.zeros(0), 1.0
        if self.m == 1:
            ds = np.array([float(f32(1.0) * f32(self.kf[0]))])
            dot = float(f32(ds[0]) * f32(self.kf[0]))
        else:
            ds = self.P @ self.kf
            dot = float(ds @ self.kf)
        return ds, max(1.0 - dot, 0.0)

    def update(self, x, y):
        """the update on the (f, K_f) of the preceding predict(x) -> (branch, delta, slack); delta is NaN for branch 0, slack NaN
        outside the margin case"""
        x = np.asarray(x, dtype=np.float64)
        m, y = self.m, int(y)
        margin = y * self.f
        if margin <= 0:
            ds, delta = self._project()
            if delta <= self.eta:
                nc = self.c + y * ds
                self.c = nc.astype(f32).astype(np.float64) if m == 1 else nc
                return 1, delta, np.nan
            self.L = x[None].copy() if m == 0 else np.vstack([self.L, x])
            self.c = np.append(self.c, float(y))
            if m == 0:
                self.P = np.ones((1, 1))
            else:
                P = np.zeros((m + 1, m + 1))
                P[:m, :m] = self.P
                de = np.append(ds, -1.0)
                self.P = P + np.outer(de, de) / delta
            return 2, delta, np.nan
        if not self.plus or margin >= 1:
            return 0, np.nan, np.nan
        ds, delta = self._project()
        norm = max(1.0 - delta, 0.0)
        loss = float(f32(1.0) - f32(margin)) if m == 1 else 1.0 - margin
        slack = loss - delta / self.eta
        if not slack > 0:
            return 4, delta, slack
        with np.errstate(divide='ignore'):
            alpha = min(min(np.float64(loss) / norm, 1.0), 2.0 * np.float64(slack) / norm)
        nc = self.c + (alpha * y) * ds
        self.c = nc.astype(f32).astype(np.float64) if m == 1 else nc
        return 3, delta, slack


def replay(x, y, ties=(), plus=True, eta=0.1, gamma=1.0, on_sample=None):
    """teacher-forced replay of a sample stream -> (mirror, dict of per-sample arrays f, ypred, branch, delta, slack, m).  ties: the
    recorded draws, consumed in order.  on_sample(i, mirror, branch) is called after every sample."""
    mir = PlusMirror(gamma=gamma, eta=eta, plus=plus)
    draws = iter(ties)
    n = len(x)
    out = dict(f=np.zeros(n), ypred=np.zeros(n, dtype=np.int64), branch=np.zeros(n, dtype=np.int64), delta=np.zeros(n),
               slack=np.zeros(n), m=np.zeros(n, dtype=np.int64))
    for i in range(n):
        out['ypred'][i], out['f'][i] = mir.predict(x[i], tie=lambda: next(draws))
        out['branch'][i], out['delta'][i], out['slack'][i] = mir.update(x[i], y[i])
        out['m'][i] = mir.m
        if on_sample is not None:
            on_sample(i, mir, int(out['branch'][i]))
    return mir, out
