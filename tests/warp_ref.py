"""Two plain statements of the batched warp fit (hgp_warp_batch_f64; Warping_system.compute_warp_batch) on the CPU in fp64,
and the inputs of the sweep that tests/test_warp_ref_host.py and tests/test_gpu_warp_kernel.py share.

    u_T   = linear interpolation of the n_ctrl control values onto the T grid points (align_corners)
    inc   = softplus(u_T) + 1e-6;  g_raw = cumsum(inc);  g = x_0 + (x_end - x_0) (g_raw - g_raw[0]) / (g_raw[-1] - g_raw[0] + 1e-12)
    Y_w   = linear interpolation of the target y at clamp(g);  x_warp = g - x
    loss  = 0.5 |Y_w - Y_model|^2 / (noise + 1e-12) + lam_s |D2 x_warp|^2 + lam_a |x_warp|^2, weighted mean over the batch
    u    <- torch.optim.Adam (defaults) on the [B, n_ctrl] controls, `iters` steps, then one more forward pass

  warp_autograd: torch operators, torch autograd, torch.optim.Adam - the reference.
  warp_restated: NumPy, the reverse pass derived by hand (below), the two scans as sequential sums - what the kernel does, so
                 it checks the derivation and measures how far two honest fp64 evaluations drift apart over the iterations.

Both return (u [B,n], x_warp [B,T], y_warp [B,T,D], trace [B,iters,4] per sample and unweighted: loss, data, smooth, amp,
knot_margin).  knot_margin is the smallest |g[b,t] - x[j]| over every forward pass from `margin_from` on, every b, every
interior t and every j, over the grid's span: the interpolant has a kink at every knot, so a sample sitting on one makes the
gradient depend on rounding and not on the code under test.

A test helper (like kl_ref.py and mds_ref.py), not part of the product.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def _margin(g, x):
    """min |g[b,t] - x[j]| over interior t, over the span (inf where there is no interior point)."""
    if g.shape[1] < 3:
        return np.inf
    return float(np.min(np.abs(g[:, 1:-1, None] - x[None, None, :])) / (x[-1] - x[0]))


# ---------------------------------------------------------------------------------------------------- torch autograd
def _forward_torch(u, x, Yt, Ym, noise, lam_s, lam_a):
    B, T, D = Yt.shape
    uT = F.interpolate(u[:, None, :], size=T, mode="linear", align_corners=True)[:, 0, :]
    inc = F.softplus(uT) + 1e-6
    graw = torch.cumsum(inc, dim=1)
    x0, xN = x[0], x[-1]
    g = x0 + (xN - x0) * (graw - graw[:, :1]) / (graw[:, -1:] - graw[:, :1] + 1e-12)
    xq = torch.clamp(g, x0, xN)
    ih = torch.clamp(torch.searchsorted(x, xq.detach().contiguous(), right=False), 1, T - 1)
    il = ih - 1
    den = x[ih] - x[il] + 1e-12
    tt = ((xq - x[il]) / den)[:, :, None]
    ylo = torch.gather(Yt, 1, il[:, :, None].expand(B, T, D))
    yhi = torch.gather(Yt, 1, ih[:, :, None].expand(B, T, D))
    yw = (1.0 - tt) * ylo + tt * yhi
    xw = g - x[None, :]
    data = 0.5 * ((yw - Ym) ** 2).sum(dim=(1, 2)) / (noise + 1e-12)
    d2 = xw[:, 2:] - 2.0 * xw[:, 1:-1] + xw[:, :-2]
    smooth = lam_s * (d2 ** 2).sum(dim=1)
    amp = lam_a * (xw ** 2).sum(dim=1)
    return g, xw, yw, torch.stack([data + smooth + amp, data, smooth, amp], dim=1)


def warp_autograd(x, Yt, Ym, n_ctrl, iters, noise, lam_s, lam_a, lr, weights=None, u0=None, margin_from=0):
    x = torch.as_tensor(np.asarray(x, dtype=np.float64).reshape(-1))
    Yt = torch.as_tensor(np.asarray(Yt, dtype=np.float64))
    Ym = torch.as_tensor(np.asarray(Ym, dtype=np.float64))
    B, T, D = Yt.shape
    w = torch.ones(B, dtype=torch.float64) if weights is None else torch.clamp(
        torch.as_tensor(np.asarray(weights, dtype=np.float64).reshape(B)), min=0.0)
    u = torch.zeros((B, n_ctrl), dtype=torch.float64)
    if u0 is not None:
        u += torch.as_tensor(np.asarray(u0, dtype=np.float64).reshape(1, n_ctrl))
    u.requires_grad_(True)
    opt = torch.optim.Adam([u], lr=lr)
    trace = np.zeros((B, iters, 4))
    margin = np.inf
    xn = x.numpy()
    for it in range(iters):
        opt.zero_grad()
        g, _, _, terms = _forward_torch(u, x, Yt, Ym, noise, lam_s, lam_a)
        loss = (w * terms[:, 0]).sum() / (w.sum() + 1e-12)
        loss.backward()
        opt.step()
        trace[:, it, :] = terms.detach().numpy()
        if it >= margin_from:
            margin = min(margin, _margin(g.detach().numpy(), xn))
    with torch.no_grad():
        g, xw, yw, _ = _forward_torch(u, x, Yt, Ym, noise, lam_s, lam_a)
    if iters >= margin_from:
        margin = min(margin, _margin(g.numpy(), xn))
    return u.detach().numpy().copy(), xw.numpy().copy(), yw.numpy().copy(), trace, margin


# ------------------------------------------------------------------------------------ NumPy, reverse pass by hand
def _interp_weights(n, T):
    """Control i0[t], i1[t] and the weight l1[t] of i1 in u_T[t] = (1 - l1) u[i0] + l1 u[i1]  (source index t (n-1)/(T-1))."""
    src = (float(n - 1) / float(T - 1)) * np.arange(T, dtype=np.float64)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    return i0, i1, np.clip(src - i0, 0.0, 1.0)


def forward_grid(u, x, dtype=np.float64):
    """(g [B,T], d softplus / d u_T [B,T], q = (g - x_0) / span [B,T], S [B]) of the controls u [B,n], evaluated in `dtype`."""
    u = np.asarray(u, dtype=dtype)
    x = np.asarray(x, dtype=dtype)
    T = x.size
    i0, i1, l1 = _interp_weights(u.shape[1], T)
    l1 = l1.astype(dtype)
    uT = u[:, i0] * (1 - l1) + u[:, i1] * l1
    big = uT > 20
    z = np.exp(np.where(big, 0, uT))
    inc = np.where(big, uT, np.log1p(z)) + dtype(1e-6)
    sig = np.where(big, 1, z / (z + 1))
    graw = np.cumsum(inc, axis=1, dtype=dtype)                       # one running sum in index order
    S = graw[:, -1] - graw[:, 0] + dtype(1e-12)
    q = (graw - graw[:, :1]) / S[:, None]
    return x[0] + (x[-1] - x[0]) * q, sig, q, S


def intervals(g, x):
    """idx_hi [B,T]: the upper knot of the interval each clamped g falls in (lower bound, clamped to [1, T-1])."""
    xq = np.clip(g, x[0], x[-1])
    return np.clip(np.searchsorted(x, xq.ravel(), side="left").reshape(xq.shape), 1, x.size - 1), xq


def warp_restated(x, Yt, Ym, n_ctrl, iters, noise, lam_s, lam_a, lr, weights=None, u0=None, margin_from=0):
    """With L_b the loss of sample b, r = Y_w - Y_m, e = D2 x_warp (e[t] = w[t] - 2 w[t+1] + w[t+2], t <= T-3):
        dL/dg[t]  = [x_0 <= g[t] <= x_end] sum_d r[t,d] / (noise + 1e-12) (y_hi - y_lo) / den
                    + 2 lam_a w[t] + 2 lam_s (e[t] - 2 e[t-1] + e[t-2])                         (e outside 0..T-3 is 0)
        dq = span dL/dg;  q[t] = (c[t] - c[0]) / S,  S = c[T-1] - c[0] + 1e-12,  c = g_raw:
        dL/dc[t]  = dq[t] / S (t >= 1);  dL/dS = -sum_t dq[t] q[t] / S;  dL/dc[T-1] += dL/dS;
        dL/dc[0]  = -sum_{t>=1} dq[t] / S - dL/dS
        dL/dinc[t] = sum_{s>=t} dL/dc[s];  dL/du_T = dL/dinc * sigmoid(u_T);  dL/du[i] = sum_t (weight of u[i] in u_T[t]) dL/du_T[t]
    and the gradient of the batch mean is w_b / (sum w + 1e-12) dL_b/du_b."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    Yt = np.asarray(Yt, dtype=np.float64)
    Ym = np.asarray(Ym, dtype=np.float64)
    B, T, D = Yt.shape
    Ym = np.broadcast_to(Ym, (B, T, D))
    n = int(n_ctrl)
    w = np.ones(B) if weights is None else np.maximum(np.asarray(weights, dtype=np.float64).reshape(B), 0.0)
    wb = w / (np.sum(w) + 1e-12)
    u = np.zeros((B, n)) + (0.0 if u0 is None else np.asarray(u0, dtype=np.float64).reshape(1, n))
    m1, m2 = np.zeros((B, n)), np.zeros((B, n))
    i0, i1, l1 = _interp_weights(n, T)
    span = x[-1] - x[0]
    inv_noise = 1.0 / (noise + 1e-12)
    rows = np.arange(B)[:, None]
    trace = np.zeros((B, iters, 4))
    margin = np.inf
    for it in range(iters + 1):
        g, sig, q, S = forward_grid(u, x)
        if it >= margin_from:
            margin = min(margin, _margin(g, x))
        xw = g - x[None, :]
        ih, xq = intervals(g, x)
        il = ih - 1
        den = x[ih] - x[il] + 1e-12
        tt = (xq - x[il]) / den
        ylo, yhi = Yt[rows, il], Yt[rows, ih]                          # [B,T,D]
        yw = (1.0 - tt)[:, :, None] * ylo + tt[:, :, None] * yhi
        if it == iters:
            break
        r = yw - Ym
        e = np.zeros((B, T + 2))                                       # e[:, 2 + t] = second difference t; zero outside
        e[:, 2:T] = xw[:, :-2] - 2.0 * xw[:, 1:-1] + xw[:, 2:]
        data = 0.5 * np.sum(r * r, axis=(1, 2)) * inv_noise
        smooth, amp = lam_s * np.sum(e * e, axis=1), lam_a * np.sum(xw * xw, axis=1)
        trace[:, it, :] = np.stack([data + smooth + amp, data, smooth, amp], axis=1)
        inside = (g >= x[0]) & (g <= x[-1])
        dg = np.where(inside, np.sum(r * inv_noise * (yhi - ylo) / den[:, :, None], axis=2), 0.0)
        dg = dg + 2.0 * lam_a * xw + 2.0 * lam_s * (e[:, 2:] - 2.0 * e[:, 1:-1] + e[:, :-2])
        dq = span * dg
        dR = dq / S[:, None]                                           # through the numerator c[t] - c[0]
        dS = -np.sum(dq * q, axis=1) / S
        dc = dR.copy()
        dc[:, -1] += dS
        dc[:, 0] = -np.sum(dR[:, 1:], axis=1) - dS
        dinc = np.cumsum(dc[:, ::-1], axis=1)[:, ::-1]                 # suffix sums, from the end
        duT = dinc * sig
        du = np.zeros((B, n))
        for t in range(T):
            du[:, i0[t]] += (1.0 - l1[t]) * duT[:, t]
            if i1[t] != i0[t]:
                du[:, i1[t]] += l1[t] * duT[:, t]
        gk = du * wb[:, None]
        step = float(it + 1)
        m1 = m1 + (gk - m1) * (1.0 - 0.9)
        m2 = m2 * 0.999 + (1.0 - 0.999) * gk * gk
        bc1, bc2 = 1.0 - 0.9 ** step, 1.0 - 0.999 ** step
        u = u - (lr / bc1) * (m1 / (np.sqrt(m2) / np.sqrt(bc2) + 1e-8))
    return u, xw, yw, trace, margin


# ---------------------------------------------------------------------------------------------------- the sweep
NOISE, LAM_S, LAM_A, LR = 1.7, 200.0, 1e-3, 5e-2

#        T    B  D  n  iters  grid       u0      Ym per sample  weights
SWEEP = {
    "a": (256, 3, 1, 8, 25, "uniform", None, False, None),          # four strides, cold start
    "b": (256, 3, 4, 32, 25, "random", "warm", True, "one_neg"),    # every limit; ym_stride != 0; a zero-weight sample
    "c": (129, 2, 3, 4, 25, "random", "warm", False, None),         # one element in the third stride; n - 1 does not divide T - 1
    "d": (64, 2, 2, 2, 25, "random", "warm", True, None),           # smallest n_ctrl; exactly one stride
    "e": (65, 2, 1, 5, 25, "random", "warm", False, None),          # one element past a stride
    "f": (7, 2, 1, 4, 25, "random", "warm", False, None),           # T < 2 n_ctrl
    "g": (3, 2, 1, 2, 10, "uniform", "warm", False, None),          # a single second difference
    "h": (20, 70, 1, 8, 12, "random", "warm", False, "uniform_one_neg"),   # B > 64
    "i": (90, 3, 1, 8, 250, "random", "warm", False, None),         # the longest run the callers use
    "j": (40, 2, 1, 6, 15, "uniform", 25.0, False, None),           # softplus beyond its threshold
}
# g == x up to rounding in the first forward pass (equal increments on a uniform grid): the knot condition is stated on the
# chosen intervals there (tests/test_warp_ref_host.py) and on the margin from the second pass on
FLAT_START = ("a", "j")
SEED = 2024


def make_data(rng, x, B, D, per_sample_ym):
    """The two-bump curve of the golden generator (+ 5 d per output dimension) as the model mean; observations are that curve
    under a random smooth shift plus N(0,1) noise.  A per-sample mean is the curve under a second, smaller shift."""
    t = (x - x[0]) / (x[-1] - x[0])
    base = np.stack([80 * np.exp(-0.5 * ((t - 0.45) / 0.05) ** 2) - 30 * np.exp(-0.5 * ((t - 0.6) / 0.08) ** 2) + 5 * d
                     for d in range(D)], axis=1)
    Yt = np.zeros((B, x.size, D))
    Ym = np.zeros((B, x.size, D)) if per_sample_ym else base
    for b in range(B):
        tw = np.clip(t + rng.uniform(-0.06, 0.06) * np.sin(np.pi * t), 0, 1)
        tm = np.clip(t + rng.uniform(-0.02, 0.02) * np.sin(np.pi * t), 0, 1)
        for d in range(D):
            Yt[b, :, d] = np.interp(tw, t, base[:, d]) + rng.normal(0, 1.0, x.size)
            if per_sample_ym:
                Ym[b, :, d] = np.interp(tm, t, base[:, d])
    return Yt, Ym


@functools.lru_cache(maxsize=None)
def sweep_case(name):
    """Inputs of one sweep case as keyword arguments of warp_autograd / warp_restated / ops.warp_batch (NumPy arrays)."""
    T, B, D, n, iters, grid, u0, per_sample, wkind = SWEEP[name]
    rng = np.random.default_rng([SEED, ord(name)])
    x = np.arange(float(T)) if grid == "uniform" else np.cumsum(rng.uniform(0.3, 1.7, T))
    Yt, Ym = make_data(rng, x, B, D, per_sample)
    u0v = None if u0 is None else (rng.normal(0.0, 0.4, n) if u0 == "warm" else np.full(n, float(u0)))
    w = None
    if wkind == "one_neg":
        w = np.array([0.7, -0.3, 1.0])
    elif wkind == "uniform_one_neg":
        w = rng.uniform(0.2, 1.0, B)
        w[B // 2] = -0.5
    return dict(x=x, Yt=Yt, Ym=Ym, n_ctrl=n, iters=iters, noise=NOISE, lam_s=LAM_S, lam_a=LAM_A, lr=LR, weights=w, u0=u0v)


@functools.lru_cache(maxsize=None)
def sweep_reference(name):
    """warp_autograd of one sweep case, computed once per session; callers must not modify the arrays."""
    margin_from = 1 if name in FLAT_START else 0
    return warp_autograd(**sweep_case(name), margin_from=margin_from)


def deviations(got, ref, case):
    """Largest deviation per quantity, normalised as the device test asserts it: u by max(1, max|u_ref|), x_warp by the span,
    y_warp by max|Yt|, every trace element by the reference's total loss of its sample and iteration."""
    u, xw, yw, tr = got[:4]
    ur, xwr, ywr, trr = ref[:4]
    x = case["x"]
    out = {"u": float(np.max(np.abs(u - ur)) / max(1.0, np.max(np.abs(ur)))),
           "x_warp": float(np.max(np.abs(xw - xwr)) / (x[-1] - x[0])),
           "y_warp": float(np.max(np.abs(yw - ywr)) / np.max(np.abs(case["Yt"])))}
    out["trace"] = float(np.max(np.abs(tr - trr) / trr[:, :, :1])) if tr.size else 0.0
    return out
