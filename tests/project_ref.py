"""Restatement of IterativeGaussianProcess.project_y (reference GPI.py:194-238) in the reference's operation order, and a
`longdouble` solve of the same operator: what the projection tests are held against.  Host only.

The Gram matrices are NumPy in scikit-learn's order (bit for bit its ConstantKernel * RBF).  The solve and the two products go
through torch on the CPU in float64, as in the reference: at length-scale 3 with 45 points on a span of 30 the system has a
condition number near 1e9, and another LAPACK's solve (numpy.linalg.solve) of the same matrix sits 3e-10 from the reference's
numbers, which says nothing about the operation order."""
import numpy as np
import torch


def rbf(xa, xb, c, ell):
    """ConstantKernel(c) * RBF(ell) called with two arguments (no white noise): scikit-learn divides both grids by the
    length-scale first, then takes the squared distance."""
    a = np.asarray(xa, dtype=np.float64).reshape(-1, 1) / ell
    b = np.asarray(xb, dtype=np.float64).reshape(1, -1) / ell
    return c * np.exp(-0.5 * (a - b) ** 2)


def project_y_ref(x_train, y, C, Sigma, x_basis, c, ell, jitter=1e-4):
    """(y_p, Sigma) as GPI.py:194-238 computes them: the equal-grid short-circuit, else
    y_p = solve(K_nn^T, (C K_mn)^T)^T y with K_nn = K(x, x) + jitter I and K_mn = K(xb, x)."""
    xb = np.asarray(x_basis, dtype=np.float64).reshape(-1)
    x = np.asarray(x_train, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64)
    if xb.shape == x.shape and np.array_equal(xb, x):
        return y, Sigma
    K_mn = rbf(xb, x, c, ell)
    K_nn = rbf(x, x, c, ell) + jitter * np.eye(x.shape[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    K_mn, K_nn = t(K_mn), t(K_nn)
    C = torch.eye(xb.shape[0], dtype=torch.float64) if C is None else t(C)
    K_nn_inv = torch.linalg.solve(K_nn.T, torch.matmul(C, K_mn).T).T
    return torch.linalg.multi_dot([K_nn_inv, t(y.reshape(x.shape[0], -1))]).numpy(), Sigma


def project_y_longdouble(x_train, y, x_basis, c, ell, jitter=1e-4):
    """K(xb, x) (K(x, x) + jitter I)^-1 y with the Gram matrices, a Cholesky factorisation and both triangular solves carried in
    numpy's longdouble from the float64 inputs on (the exponentials included)."""
    ld = np.longdouble
    x = np.asarray(x_train, dtype=np.float64).reshape(-1).astype(ld) / ld(ell)
    xb = np.asarray(x_basis, dtype=np.float64).reshape(-1).astype(ld) / ld(ell)
    Y = np.asarray(y, dtype=np.float64).reshape(x.shape[0], -1).astype(ld)
    n = x.shape[0]
    K = ld(c) * np.exp(ld(-0.5) * (x[:, None] - x[None, :]) ** 2) + ld(jitter) * np.eye(n, dtype=ld)
    Ks = ld(c) * np.exp(ld(-0.5) * (xb[:, None] - x[None, :]) ** 2)
    L = np.zeros((n, n), dtype=ld)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Z = np.zeros_like(Y)
    for i in range(n):
        Z[i] = (Y[i] - L[i, :i] @ Z[:i]) / L[i, i]
    A = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        A[i] = (Z[i] - L[i + 1:, i] @ A[i + 1:]) / L[i, i]
    return (Ks @ A).astype(np.float64)


def rel_err(got, want):
    """max |got - want| relative to max |want| (the row's scale)."""
    want = np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - want)) / max(float(np.max(np.abs(want))), 1e-300))
