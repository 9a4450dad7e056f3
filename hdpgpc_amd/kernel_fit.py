"""Kernel hyper-parameter fit of a new cluster: Adam on the exact marginal log-likelihood of ONE segment,
restating what IterativeGaussianProcess.fit_torch asks gpytorch for on the shared grid (GPI.py:610-770):

* model: constant mean m, ScaleKernel(RBFKernel) -> K = s exp(-0.5 d^2 / l^2) + noise I, Gaussian likelihood;
* parameterisation (gpytorch defaults): s = softplus(raw_s), l = softplus(raw_l), noise = lo + (hi - lo) sigmoid(raw_n) with
  (lo, hi) = the white-kernel bounds (GPI.py:629,655-656); every raw parameter and m start at 0;
* loss = - log p(y | theta) / T (ExactMarginalLogLikelihood divides by the number of points), Adam(lr = 0.1), at most 4000
  iterations, early stop once 1000 iterations have run and the last ten loss increments sum to 0 within 1e-4 (GPI.py:689-693);
* afterwards the length-scale is OVERWRITTEN with 1.2 (GPI.py:711); output-scale and noise are kept.

The value and the gradient of the log-likelihood come from the a10 kernels (Gram, Cholesky score, Cholesky inverse,
hgp_lml_grad_f64); only four scalars per iteration reach the host.  gpytorch is absent in the build container, so this
step has no golden vector ("parity unpinned"): tests check it against a NumPy restatement of the same
optimiser on the oracle's log-likelihood, and that the bounds hold and the loss settles.

fit_kernels_batch runs the same optimisation for B segments at once with every iteration on the device
(hgp_kernel_fit_steps_f64, include/hdpgpc_hip_fit.h): nothing returns to the host but one status vector per chunk of iterations.
"""
import math

import numpy as np
import torch

from . import ops

f64 = torch.float64


def _softplus(x):
    return math.log1p(math.exp(-abs(x))) + max(x, 0.0)


def _sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x)) if x >= 0 else math.exp(x) / (1.0 + math.exp(x))


def lml_value_grad(x, r, c, ell, noise, ones_row):
    """log N(r | 0, c RBF(ell) + noise I) and its gradient w.r.t. (log c, log ell, log noise), plus sum(K^-1 r).
    x [T], r [1,T], ones_row [1,T] device tensors.  Returns (value, grad[3], sum_alpha) as host floats, or None if K is not PD."""
    T = x.numel()
    K = ops.gram_rbf(x, None, c, ell, noise)
    items = ops.build_items([0], [0.0], [1])
    quad, logdet, info = ops.score_groups(r, None, K, *items, jitter_rel=0.0, want_logdet=True)
    Z, _ = ops.chol_inverse(K)
    Kinv = ops.gemm_batched(Z[0], Z[0], transA=True)
    alpha = ops.gemm_batched(Kinv, r.reshape(-1, 1))
    grad = ops.lml_grad(x, alpha.reshape(-1), Kinv, c, ell, noise)
    sa = ops.gemm_batched(ones_row, alpha)
    host = torch.cat([quad.reshape(1), logdet.reshape(1), grad.reshape(3), sa.reshape(1), info.to(f64).reshape(1)]).cpu().numpy()
    if host[6] != 0:
        return None
    val = -0.5 * host[0] - 0.5 * host[1] - 0.5 * T * math.log(2.0 * math.pi)
    return val, host[2:5], host[5]


def fit_kernel_adam(x, y, noise_bounds, device="cuda", max_iter=4000, lr=0.1, min_iter=1000, return_trace=False):
    """Returns (outputscale, lengthscale, noise, mean) at the end of the optimisation (the caller applies GPI.py:711)."""
    xh = np.asarray(x, dtype=np.float64).reshape(-1)
    yh = np.asarray(y, dtype=np.float64).reshape(-1)
    T = xh.size
    xd = torch.as_tensor(xh, dtype=f64, device=device)
    ones_row = torch.ones((1, T), dtype=f64, device=device)
    lo, hi = float(noise_bounds[0]), float(noise_bounds[1])
    p = np.zeros(4)                        # raw noise, mean, raw outputscale, raw lengthscale (gpytorch's parameter order)
    m1, m2 = np.zeros(4), np.zeros(4)
    b1, b2, eps = 0.9, 0.999, 1e-8          # torch.optim.Adam defaults
    losses = []
    for it in range(1, max_iter + 1):
        s_n = _sigmoid(p[0])
        noise = lo + (hi - lo) * s_n
        c, ell = _softplus(p[2]), _softplus(p[3])
        r = torch.as_tensor((yh - p[1])[None, :], dtype=f64, device=device)
        out = lml_value_grad(xd, r, c, ell, noise, ones_row)
        if out is None:
            raise torch.linalg.LinAlgError("kernel fit: K(theta) is not positive-definite")
        val, glog, sum_alpha = out
        losses.append(-val / T)
        g = np.array([glog[2] / noise * (hi - lo) * s_n * (1.0 - s_n),        # d noise / d raw
                      sum_alpha,                                                 # d L / d mean = 1^T K^-1 (y - m)
                      glog[0] / c * _sigmoid(p[2]),                             # d softplus = sigmoid
                      glog[1] / ell * _sigmoid(p[3])]) * (-1.0 / T)
        m1 = b1 * m1 + (1 - b1) * g
        m2 = b2 * m2 + (1 - b2) * g * g
        p = p - lr * (m1 / (1 - b1 ** it)) / (np.sqrt(m2 / (1 - b2 ** it)) + eps)
        if len(losses) > min_iter and abs(float(np.sum(np.subtract(losses[-10:], losses[-11:-1])))) <= 1e-4:
            break
    theta = (_softplus(p[2]), _softplus(p[3]), lo + (hi - lo) * _sigmoid(p[0]), p[1])
    return (theta, np.asarray(losses)) if return_trace else theta


def theta_of_state(state, noise_bounds):
    """theta [B,4] = (outputscale, lengthscale, noise, mean), as fit_kernel_adam defines them, of the raw parameters in the
    state rows [B, FIT_STATE_DOUBLES] of ops.kernel_fit_steps (host arrays)."""
    nb = np.asarray(noise_bounds, dtype=np.float64).reshape(-1, 2)
    return np.array([(_softplus(p[2]), _softplus(p[3]), lo + (hi - lo) * _sigmoid(p[0]), p[1])
                     for p, (lo, hi) in zip(np.asarray(state, dtype=np.float64).tolist(), nb.tolist())]).reshape(-1, 4)


def fit_kernels_batch(x, Y, noise_bounds, device="cuda", max_iter=4000, lr=0.1, min_iter=1000, chunk=250, return_trace=False,
                      check=True, return_state=False):
    """fit_kernel_adam for B segments Y [B,T] (numpy or a device tensor) in one batch on the device (ops.kernel_fit_steps): the
    iterations run in calls of `chunk`, nothing returns to the host inside a call, and the status of the fits is read once per
    call to stop when none is running.  x [T] or [B,T]; noise_bounds one pair or [B,2].
    Returns theta [B,4] = (outputscale, lengthscale, noise, mean) and n_iter [B] (numpy); with return_trace also a list of each
    fit's losses, trimmed to its n_iter; with return_state also (state, status) as the device left them.
    A fit that failed (K not positive-definite, or a non-finite value) keeps the parameters of its last good iteration and does
    not disturb the others; check=True raises torch.linalg.LinAlgError naming the failed fits."""
    Yd = ops.to_dev(Y, f64, device)
    if Yd.dim() != 2:
        raise ValueError("fit_kernels_batch: Y must be [B, T]")
    B, T = Yd.shape
    nb = np.ascontiguousarray(np.broadcast_to(np.asarray(noise_bounds, dtype=np.float64).reshape(-1, 2), (B, 2)))
    if B == 0:
        out = (np.zeros((0, 4)), np.zeros(0, dtype=np.int64))
        out += ([],) if return_trace else ()
        return out + ((None, None),) if return_state else out
    xd = ops.to_dev(x, f64, device)
    xd = xd.reshape(B, T) if xd.numel() == B * T and xd.dim() == 2 else xd.reshape(-1)
    bd = ops.to_dev(nb, f64, device)
    state = torch.zeros((B, ops._ffi.FIT_STATE_DOUBLES), dtype=f64, device=Yd.device)
    status = torch.zeros(B, dtype=torch.int32, device=Yd.device)
    losses = torch.zeros((B, max_iter), dtype=f64, device=Yd.device) if return_trace else None
    done, chunk = 0, max(int(chunk), 1)
    while done < max_iter:
        n = min(chunk, max_iter - done)
        ops.kernel_fit_steps(xd, Yd, bd, state, status, n, lr=lr, min_iter=min_iter, max_iter=max_iter, loss_out=losses)
        done += n
        if not bool((status == 0).any()):        # the one read per call
            break
    st_h, status_h = state.cpu().numpy(), status.cpu().numpy()
    if check and (status_h < 0).any():
        bad = np.nonzero(status_h < 0)[0].tolist()
        raise torch.linalg.LinAlgError(f"kernel fit: fits {bad} failed (status {status_h[bad].tolist()}: -1 = K(theta) is not "
                                       "positive-definite, -2 = a non-finite value)")
    n_iter = st_h[:, 12].astype(np.int64)
    out = (theta_of_state(st_h, nb), n_iter)
    if return_trace:
        lh = losses.cpu().numpy()
        out += ([lh[b, :n_iter[b]].copy() for b in range(B)],)
    return out + ((state, status),) if return_state else out
