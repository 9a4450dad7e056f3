"""NumPy restatement of the static filter chain, written from the contract in include/hdpgpc_hip_static.h (not from the kernel):
one chain absorbs n observations with constant A, C, Sigma and Gamma = 0 (GPI.posterior, GPI.py:134-151, on the shared grid with
h = 1), the first-step branch, the status word and the resumable progress counter."""
import numpy as np


def chol_inverse(S):
    """(Z, info): Z = chol(0.5 (S + S^T))^-1, info = 1-based index of the first pivot that is not positive (0: none)."""
    A = 0.5 * (S + S.T)
    T = A.shape[0]
    L = np.zeros_like(A)
    for j in range(T):
        p = A[j, j] - L[j, :j] @ L[j, :j]
        if not p > 0.0:
            return None, j + 1
        L[j, j] = np.sqrt(p)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return np.linalg.solve(L, np.eye(T)), 0


def member(A, C, Sigma, m, P, y, first=False, white=0.0):
    """One member: (m', P', info)."""
    T = A.shape[0]
    xm = A @ m
    if first:
        Pk, fstar, covf = P, np.zeros(T), white * np.eye(T)
    else:
        Pk, fstar, covf = A @ P @ A.T, C @ xm, Sigma
    S = C @ Pk @ C.T + covf
    Z, info = chol_inverse(S)
    if info:
        return None, None, info
    K = (Pk @ C.T) @ (Z.T @ Z)
    IKC = np.eye(T) - K @ C
    return xm + K @ (y - fstar), IKC @ Pk @ IKC.T + (K @ covf) @ K.T, 0


class Chain:
    """The descriptor's fields as arrays; steps(max_steps) is one call."""

    def __init__(self, A, C, Sigma, Fs, Ps, pos, Y, y_idx, first=False, white=0.0):
        self.A, self.C, self.Sigma, self.Y, self.y_idx = A, C, Sigma, Y, np.asarray(y_idx, dtype=np.int64)
        self.Fs, self.Ps = Fs.copy(), Ps.copy()
        self.pos = self.pos0 = int(pos)
        self.n, self.first, self.white, self.info = len(self.y_idx), bool(first), float(white), 0

    def steps(self, max_steps):
        if self.info != 0:
            return self
        i0 = self.pos - self.pos0
        for i in range(i0, min(self.n, i0 + max_steps)):
            r = self.pos0 + i
            with np.errstate(all="ignore"):
                m, P, info = member(self.A, self.C, self.Sigma, self.Fs[r], self.Ps[r], self.Y[self.y_idx[i]],
                                    first=self.first and i == 0, white=self.white)
            if info:
                self.info = info
                self.Fs[r + 1:self.pos0 + self.n + 1] = np.nan
                self.Ps[r + 1:self.pos0 + self.n + 1] = np.nan
                self.pos = self.pos0 + self.n
                break
            self.Fs[r + 1], self.Ps[r + 1] = m, P
            self.pos = r + 1
        return self


def rel_err(got, want):
    """max |got - want| / max |want| (0 / 0 = 0); NaN anywhere in one and not the other = inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return np.inf
    ok = ~np.isnan(want)
    if not ok.any():
        return 0.0
    scale = np.max(np.abs(want[ok]))
    diff = np.max(np.abs(got[ok] - want[ok]))
    return 0.0 if diff == 0.0 else float(diff / scale)
