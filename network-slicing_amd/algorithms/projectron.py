"""SVvariable / Projectron / ProjectronPlus with the reference's surface (reference algorithms/projectron.py:3-107).

The dictionary (landmarks, coefficients, K^-1) lives on the GPU inside a kb_* agent; predict(x) and
update(x, y) are kb_predict / kb_update calls.  A Projectron created on its own owns a private
1-learner agent; one handed to kbrl_control.KBRL_Control is re-bound to that agent's learner."""
import numpy as np

from ranslice.kbrl_dev import VecKBRL


class SVvariable:
    """growable landmark/coefficient store (projectron.py:3-21); a view of the device dictionary"""

    def __init__(self):
        self._owner = None

    @property
    def counter(self):
        return self._owner._get()['m'] if self._owner and self._owner._bound() else 0

    @property
    def landmarks(self):
        d = self._owner._get()
        return d['landmarks'][0] if d['m'] == 1 else d['landmarks']  # 1-D while single (projectron.py:16-17)

    @property
    def coeff(self):
        return self._owner._get()['coeff']


class Projectron:
    ALGORITHM = 'projectron'   # the update rule of the private agent (VecKBRL(algorithm=...))

    def __init__(self, kernel, eta=0.1, capacity=4096):
        self.kernel = kernel
        self.sv = kernel.sv
        self.eta = eta
        self.capacity = capacity
        self.f = 0.0
        self._agent = None
        self._e = 0
        self._s = 0
        kernel._owner = self
        self.sv._owner = self

    # ---- binding to a device learner
    def _bound(self):
        return self._agent is not None

    def _bind(self, agent, e, s):
        self._agent, self._e, self._s = agent, e, s

    def _ensure(self, x):
        if self._agent is None:
            self._agent = VecKBRL(1, [len(x) - 1], 200, gamma=self.kernel.gamma, eta=self.eta,
                                  capacity=self.capacity, algorithm=self.ALGORITHM)
            self._agent.reset([[0]], [[0]])
            self._e = self._s = 0

    def _get(self, with_kinv=False):
        return self._agent.learner(self._e, self._s, with_kinv=with_kinv)

    def _kernel_row(self):
        """K_f of the last predict (projectron.py:34)"""
        return self._agent.kernel_row(self._e, self._s)

    @property
    def counter(self):
        return self._get()['m'] if self._bound() else 0

    @property
    def Kinv(self):
        return self._get(with_kinv=True)['kinv']

    # ---- reference surface
    def predict(self, x):
        """projectron.py:32-37"""
        x = np.asarray(x, dtype=np.float64)
        self._ensure(x)
        y, self.f = self._agent.predict(self._e, self._s, x)
        return y

    def update(self, x, y):
        """projectron.py:39-60; uses the f / k cached by the preceding predict(x) (reference Q12)"""
        x = np.asarray(x, dtype=np.float64)
        self._ensure(x)
        self._agent.update(self._e, self._s, x, int(y))

    # ---- build-defined conveniences (the reference has none of them)
    def fit(self, X, y, wide=None):
        """BUILD-DEFINED: predict(x_t) then update(x_t, y_t) over the rows of X in order, in one device call (VecKBRL.fit) -- the
        dictionary, f and every prediction are bit for bit what the loop over predict / update leaves.  -> the predictions
        [len(X)].  The cached (f, k) of predict is invalid afterwards: call predict before the next update.
        wide: None keeps the agent's setting; min_landmarks, or (min_landmarks, window), is handed to VecKBRL.set_fit_wide first
        and stays in force: from that dictionary size on the samples are taught by chip-wide rounds -- same bits, less time once
        the dictionary holds hundreds of landmarks (0 turns it off again).  A ProjectronPlus is taught by those rounds only while its
        attribute wide_plus is true (VecKBRL.set_fit_wide_plus)."""
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(1, -1) if X.ndim == 1 else X
        if X.shape[0] == 0:
            return np.zeros(0, dtype=np.int32)
        self._ensure(X[0])
        if wide is not None:
            self._agent.set_fit_wide(*(wide if isinstance(wide, (tuple, list)) else (wide,)))
        if isinstance(self, ProjectronPlus):
            self._agent.set_fit_wide_plus(bool(self.wide_plus))
        out = self._agent.fit([(self._e, self._s)], [X], [np.asarray(y).reshape(-1)])
        self.f = float(out['f'][0][-1])
        return out['y_pred'][0]

    def decision_function(self, X):
        """BUILD-DEFINED: f(x) for the rows of X (VecKBRL.score), each bit for bit the f that predict(x) leaves in self.f;
        read-only: no cached row, no tie draw, self.f untouched.  -> [len(X)] float64 (zeros while the dictionary is empty)"""
        X = np.asarray(X, dtype=np.float64)
        X = X.reshape(1, -1) if X.ndim == 1 else X
        if X.shape[0] == 0:
            return np.zeros(0)
        self._ensure(X[0])
        return self._agent.score([(self._e, self._s)], [X])[0][0]

    def get_set_size(self):
        """projectron.py:62-64: landmarks.shape[0] (the vector length while a single landmark is held)"""
        d = self._get()
        if d['m'] == 0:
            raise AttributeError("'SVvariable' object has no attribute 'landmarks'")
        return d['landmarks'].shape[1] if d['m'] == 1 else d['m']


class ProjectronPlus(Projectron):
    """Projectron++ (projectron.py:66-107): update(x, y) also acts on a sample classified correctly inside the margin,
    0 < y f < 1 -- a scaled projection that never adds a landmark.  The private one-learner agent runs in Projectron++ mode
    (kb_set_algorithm); predict, update, fit, decision_function and Kinv work as on Projectron.  Accepted by
    kbrl_control.KBRL_Control only when every learner of the list is a ProjectronPlus whose control_plus is true (below); otherwise
    fit logged control steps instead (ranslice.kbrl_dev.augmented_samples + VecKBRL.fit).
    control_plus (a plain attribute, False by default): the learner opts into the closed control loop's margin-rule update phase
    (VecKBRL.set_control_plus); KBRL_Control reads it when it is constructed.
    wide_plus (a plain attribute, False by default): whether fit(..., wide=...) lets the chip-wide rounds teach this learner too;
    fit hands it to VecKBRL.set_fit_wide_plus before every call.  Off, fit keeps the one-workgroup path whatever `wide` says."""
    ALGORITHM = 'projectron_plus'
    control_plus = False

    def __init__(self, kernel, eta=0.1, capacity=4096):
        super().__init__(kernel, eta=eta, capacity=capacity)
        self.wide_plus = False

    def _bind(self, agent, e, s):
        if agent.algorithm != self.ALGORITHM:
            raise ValueError('ProjectronPlus: the agent it is bound to runs %r' % agent.algorithm)
        super()._bind(agent, e, s)
