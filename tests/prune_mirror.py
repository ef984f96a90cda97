"""Float64 mirror of the Projectron update and of the pruning rule of kb_prune, written from the mathematics.

Projectron (Gaussian kernel, k(x, x) = 1).  A dictionary holds landmarks l_j, coefficients c_j and P = inv(Gram).  For a
sample (x, y) with kernel column k_j = exp(-gamma |l_j - x|^2) and f = k . c:  when f y <= 0,  d = P k,
delta = max(1 - k . d, 0);  delta <= eta: c += y d  (the sample is projected onto the span);  otherwise the sample becomes a
landmark with coefficient y and P grows by the bordering formula
    [[P + d d^T / delta, -d / delta], [-d^T / delta, 1 / delta]].
A dictionary of one landmark works in float32, as the device does (the reference's first arrays are float32).

Pruning.  While m > target:  r = argmin_j c_j^2 / P[j][j] (lowest j on a tie);  p = P[:, r], q = P[r][r];
c_i += c_r (-p_i / q) and P[i][j] -= (p_i p_j) / q over the survivors;  the last landmark moves into slot r;  m -= 1.
P[S][S] - P[S][r] P[r][S] / q is the Schur complement that inverts the survivors' Gram matrix, c_r (-p / q) are the
coefficients of the best approximation of c_r k(l_r, .) in their span, and c_r^2 / q is its squared RKHS error.

No sum is formed in a removal, so remove_one() -- separate NumPy ufuncs on IEEE float64, nothing fused -- performs the device's
operations in the device's order: a mirror loaded with a device's own state (Mirror.from_state) defines the device's bits
(tests/test_gpu_prune_chain.py).  remove_one_scalar() is the same removal in Python floats and loops, written from the seven
steps of kb_prune.hip's header; tests/test_prune_mirror.py holds the two to each other bit for bit.
"""
import struct

import numpy as np


def gram(L, gamma, dtype=np.float64):
    L = np.asarray(L, dtype=dtype)
    sq = (L * L).sum(axis=1)
    d2 = sq[:, None] + sq[None, :] - 2 * (L @ L.T)
    return np.exp(-dtype(gamma) * np.maximum(d2, 0))


def gram_exact(L, gamma, dtype=np.longdouble):
    """the Gram matrix from the differences themselves (no cancellation), in `dtype`"""
    L = np.asarray(L, dtype=dtype)
    m = len(L)
    G = np.empty((m, m), dtype=dtype)
    for i in range(m):
        t = L - L[i]
        G[i] = np.exp(-dtype(gamma) * (t * t).sum(axis=1))
    return G


def inv_longdouble(G):
    """Gauss-Jordan inverse of a symmetric positive definite matrix in longdouble (no pivoting needed)"""
    n = len(G)
    A = np.array(G, dtype=np.longdouble)
    X = np.eye(n, dtype=np.longdouble)
    for i in range(n):
        piv = A[i, i]
        A[i] /= piv
        X[i] /= piv
        col = A[:, i].copy()
        col[i] = 0
        A -= col[:, None] * A[i][None, :]
        X -= col[:, None] * X[i][None, :]
    return X


class Mirror:
    """one dictionary; ids[j] = the insertion number of the landmark in slot j"""

    def __init__(self, d, gamma=1.0, eta=0.1, capacity=4096):
        self.d, self.gamma, self.eta, self.cap = d, gamma, eta, capacity
        self.L = np.zeros((0, d))
        self.c = np.zeros(0)
        self.P = np.zeros((0, 0))
        self.ids = []
        self.idx = None      # grid index per slot (from_state): carried through the move of remove_one
        self.born = 0
        self.k = np.zeros(0)
        self.f = 0.0

    @classmethod
    def from_state(cls, L, c, P, idx=None):
        """a mirror loaded with a dictionary as read from a device: landmark rows L [m, d], coefficients c [m], Kinv P [m, m] and,
        optionally, the grid indices idx [m].  Pruning only: remove_one() forms no kernel value, so gamma and eta play no part,
        and fed the device's own state it performs the device's operations in the device's order (ids[j] = the slot the
        landmark held when it was loaded)"""
        L, c, P = (np.array(a, dtype=np.float64) for a in (L, c, P))
        m = len(c)
        if L.shape[0] != m or P.shape != (m, m) or (idx is not None and len(idx) != m):
            raise ValueError('from_state: L [m, d], c [m], P [m, m], idx [m]')
        mr = cls(L.shape[1])
        mr.L, mr.c, mr.P = L, c, P
        mr.ids = list(range(m))
        mr.born = m
        mr.idx = None if idx is None else np.array(idx, dtype=np.int64)
        return mr

    @property
    def m(self):
        return len(self.c)

    def column(self, x):
        t = self.L - np.asarray(x, dtype=np.float64)
        return np.exp(-self.gamma * (t * t).sum(axis=1))

    def predict(self, x):
        """-> f; the column is kept for update (the margin |f| tells how far the sign is from its threshold)"""
        m = self.m
        if m == 0:
            self.k, self.f = np.zeros(0), 0.0
        elif m == 1:
            k32 = np.float32(self.column(x)[0])
            self.k = np.array([float(k32)])
            self.f = float(np.float32(k32 * np.float32(self.c[0])))
        else:
            self.k = self.column(x)
            self.f = float(self.k @ self.c)
        return self.f

    def _insert(self, x, y):
        self.L = np.vstack([self.L, np.asarray(x, dtype=np.float64)[None]])
        self.c = np.append(self.c, float(y))
        self.ids.append(self.born)
        self.born += 1

    def update(self, x, y):
        """after predict(x) -> (branch, delta): 0 no mistake, 1 projected, 2 inserted"""
        if not self.f * y <= 0:
            return 0, 0.0
        m = self.m
        if m == 0:
            self._insert(x, y)
            self.P = np.ones((1, 1))
            return 2, 1.0
        if m == 1:
            k32 = np.float32(self.k[0])
            d = np.array([float(np.float32(1.0) * k32)])
            dot = float(np.float32(np.float32(d[0]) * k32))
        else:
            d = self.P @ self.k
            dot = float(d @ self.k)
        delta = max(1.0 - dot, 0.0)
        if delta <= self.eta or m >= self.cap:
            self.c = self.c + y * d
            if m == 1:
                self.c = np.array([float(np.float32(self.c[0]))])
            return 1, delta
        P = np.empty((m + 1, m + 1))
        P[:m, :m] = self.P + np.outer(d, d) / delta
        P[m, :m] = P[:m, m] = (-1.0 * d) / delta
        P[m, m] = (-1.0 * -1.0) / delta
        self.P = P
        self._insert(x, y)
        return 2, delta

    def remove_one(self):
        """one removal -> dict(slot, id, key, gap = (runner-up - key) / runner-up, q, cr, p, c_before)"""
        m = self.m
        diag = np.diag(self.P)
        key = (self.c * self.c) / diag
        r = int(np.argmin(key))        # (numpy: the first of equal minima)
        rest = np.delete(key, r)
        ru = float(rest.min()) if len(rest) else np.inf
        p = self.P[:, r].copy()
        q = float(p[r])
        cr = float(self.c[r])
        out = dict(slot=r, id=self.ids[r], key=float(key[r]), gap=(ru - float(key[r])) / ru if ru > 0 else 0.0, q=q, cr=cr,
                   p=p, c_before=self.c.copy(), diag_ok=bool(np.isfinite(diag).all() and (diag > 0).all()))
        c = self.c + cr * ((-p) / q)
        c[r] = self.c[r]
        self.P -= np.outer(p, p) / q
        last = m - 1
        if r != last:
            self.P[r, :] = self.P[last, :]
            self.P[:, r] = self.P[:, last]
            self.P[r, r] = self.P[last, last]
            c[r] = c[last]
            self.L[r] = self.L[last]
            self.ids[r] = self.ids[last]
            if self.idx is not None:
                self.idx[r] = self.idx[last]
        if self.idx is not None:
            self.idx = self.idx[:last].copy()
        self.P = self.P[:last, :last].copy()
        self.c = c[:last].copy()
        self.L = self.L[:last].copy()
        self.ids.pop()
        return out

    def prune(self, target):
        log = []
        while self.m > target:
            log.append(self.remove_one())
        return log


def key_bits(x):
    """the bit pattern of a float64 as an unsigned 64-bit integer (the device's __double_as_longlong, read unsigned)"""
    return struct.unpack('<Q', struct.pack('<d', x))[0]


def remove_one_scalar(L, c, P, idx=None):
    """One removal in plain Python floats and loops, written from the seven steps of kb_prune.hip's header and from nothing
    else: lists (of lists) in, -> (r, L, c, P, idx) as new lists, the inputs untouched.  Every product, quotient, sum and
    difference is one IEEE float64 operation of the interpreter, in the order the header writes them; the argmin runs over
    the pair (bit pattern of the key as uint64, slot), as prune_choose_kernel's does."""
    m = len(c)
    # 1. r = argmin_j (c_j c_j) / P[j][j], the lowest j on a tie
    best = None
    for j in range(m):
        pair = (key_bits((c[j] * c[j]) / P[j][j]), j)
        if best is None or pair < best:
            best = pair
    r = best[1]
    # 2. p = P[:, r], q = P[r][r]
    p = [P[i][r] for i in range(m)]
    q = P[r][r]
    cr = c[r]
    # 3. c_i = c_i + c_r * ((-p_i) / q) for every survivor
    c = [c[i] if i == r else c[i] + cr * ((-p[i]) / q) for i in range(m)]
    # 4. P[i][j] = P[i][j] - (p_i * p_j) / q for every survivor pair
    P = [[P[i][j] if (i == r or j == r) else P[i][j] - (p[i] * p[j]) / q for j in range(m)] for i in range(m)]
    L = [list(row) for row in L]
    idx = None if idx is None else list(idx)
    # 5. landmark m - 1 moves into slot r (unless r = m - 1)
    last = m - 1
    if r != last:
        for k in range(m):
            if k != r and k != last:
                P[r][k] = P[last][k]
                P[k][r] = P[last][k]
        P[r][r] = P[last][last]
        L[r] = L[last]
        c[r] = c[last]
        if idx is not None:
            idx[r] = idx[last]
    # 6. slot m - 1 and row / column m - 1 go;  7. m -= 1
    P = [row[:last] for row in P[:last]]
    return r, L[:last], c[:last], P, (None if idx is None else idx[:last])


def build_from_landmarks(L, c, gamma=1.0):
    """a Mirror whose P comes from the Projectron's own bordering recursion over the given landmarks (no projections)"""
    mr = Mirror(L.shape[1], gamma=gamma, eta=-1.0)   # eta < 0: every sample is inserted
    for j in range(len(L)):
        mr.f = 0.0
        if mr.m == 0:
            mr.k = np.zeros(0)
        elif mr.m == 1:
            mr.k = np.array([float(np.float32(mr.column(L[j])[0]))])
        else:
            mr.k = mr.column(L[j])
        mr.update(L[j], 1)
    mr.c = np.asarray(c, dtype=np.float64).copy()
    return mr


def chains(idx):
    """head [256] and links [m] from the grid indices by the invariant: head[a] = the largest slot with index a, every link the
    next smaller slot with the same index (-1: none); off-grid landmarks (index < 0) carry -1"""
    head = -np.ones(256, dtype=np.int64)
    link = -np.ones(len(idx), dtype=np.int64)
    for j, a in enumerate(idx):
        if a >= 0:
            link[j] = head[a]
            head[a] = j
    return head, link
