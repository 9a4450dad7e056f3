"""hgp_warp_batch_f64 called directly (ops.warp_batch) at the shapes its only other test, the golden run through
Warping_system.compute_warp_batch (n_ctrl = 8, shared Ym, uniform grids, T <= 128, D <= 2, batch-mean trace), never reaches:
T up to 256 (every pass of the t += 64 loops), D up to 4, n_ctrl from 2 to 32 with n_ctrl - 1 not dividing T - 1, per-sample Ym,
non-uniform grids, negative and zero weights, B > 64, the softplus branch beyond 20, iters = 0, no trace, T = 2 and the status codes.

Reference: tests/warp_ref.py::warp_autograd (torch operators + autograd + torch.optim.Adam on the CPU in fp64), held to the
reference project's recorded outputs and to a hand-derived NumPy restatement in tests/test_warp_ref_host.py.  The per-sample
trace is compared element by element relative to the sample's total loss of that iteration: the first Adam step only sees the
gradient's sign, so a wrong magnitude shows from the second iteration on, in the trace.

Largest deviation per quantity over the ten sweep cases (u over max(1, max|u_ref|), x_warp over the span, y_warp over
max|Yt|, trace over the total loss):
                         u         x_warp    y_warp    trace
    CPU floor (restated) 9.0e-15   6.1e-16   9.4e-15   6.4e-14
    MI355X               6.3e-15   6.8e-16   1.3e-14   8.2e-14
TOL = 1e-12: ten times the largest device figure (8.2e-13) rounded up to a power of ten, which is also the smallest value
the test is allowed; the most it could have been is 1e-9.
"""
import ctypes

import numpy as np
import pytest
import torch

import warp_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

TOL = 1e-12
EPS = float(np.finfo(np.float64).eps)


def dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def run(case, **over):
    kw = {**case, **over}
    out = ops.warp_batch(dev(kw["x"]), dev(kw["Yt"]), dev(kw["Ym"]), kw["n_ctrl"], kw["iters"], kw["noise"], kw["lam_s"], kw["lam_a"],
                         kw["lr"], weights=dev(kw["weights"]), u0=dev(kw["u0"]), want_trace=kw.get("want_trace", True))
    return tuple(None if o is None else o.cpu().numpy() for o in out)


@pytest.mark.parametrize("name", sorted(warp_ref.SWEEP))
def test_sweep_against_autograd(name):
    case = warp_ref.sweep_case(name)
    ref = warp_ref.sweep_reference(name)
    u, xw, yw, tr = run(case)
    d = warp_ref.deviations((u, xw, yw, tr), ref, case)
    first = np.argwhere(np.abs(tr - ref[3]) > TOL * ref[3][:, :, :1])
    print(f"device deviation, case {name}: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items())
          + (f"  first trace element beyond TOL (b, it, term): {first[np.argmin(first[:, 1])]}" if first.size else ""))
    x = case["x"]
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(xw)) and np.all(np.isfinite(yw)) and np.all(np.isfinite(tr))
    assert np.all(np.abs(u - ref[0]) <= TOL * max(1.0, np.max(np.abs(ref[0])))), d
    assert np.all(np.abs(xw - ref[1]) <= TOL * (x[-1] - x[0])), d
    assert np.all(np.abs(yw - ref[2]) <= TOL * np.max(np.abs(case["Yt"]))), d
    assert np.all(np.abs(tr - ref[3]) <= TOL * ref[3][:, :, :1]), d
    g = xw + x[None, :]                                   # monotone warps that keep both end points
    assert np.all(np.diff(g, axis=1) > 0) and np.allclose(g[:, 0], x[0]) and np.allclose(g[:, -1], x[-1])
    w = case["weights"]
    if w is not None:                                     # a sample without weight keeps its start bit for bit
        u0 = np.zeros(case["n_ctrl"]) if case["u0"] is None else case["u0"]
        assert np.any(w <= 0) and np.array_equal(u[w <= 0], np.broadcast_to(u0, u[w <= 0].shape))


def test_zero_iterations_is_the_forward_pass_of_u0():
    case = warp_ref.sweep_case("c")
    ref = warp_ref.warp_autograd(**{**case, "iters": 0})
    u, xw, yw, tr = run(case, iters=0)
    assert tr.shape == (2, 0, 4)
    assert np.array_equal(u, np.broadcast_to(case["u0"], u.shape))
    x = case["x"]
    assert np.all(np.abs(xw - ref[1]) <= TOL * (x[-1] - x[0]))
    assert np.all(np.abs(yw - ref[2]) <= TOL * np.max(np.abs(case["Yt"])))


@pytest.mark.parametrize("name", ["b", "e"])
def test_without_trace_same_bits(name):
    case = warp_ref.sweep_case(name)
    with_tr, without = run(case), run(case, want_trace=False)
    assert without[3] is None
    for a, b in zip(with_tr[:3], without[:3]):
        assert np.array_equal(a, b)


def test_two_grid_points():
    """T = 2: nothing to fit.  The first point is exact; the last one is the end point up to the two 1e-12 terms of the
    operation itself (S = inc[1] + 1e-12 in the normalisation, den = span + 1e-12 in the interpolation), which both references
    show as well: x_warp[1] = -span 1e-12 / S.  u is not compared: the gradient is that of the 1e-12 terms alone, and Adam
    divides it by its own magnitude."""
    rng = np.random.default_rng(5)
    x = np.array([3.7, 5.1])
    Yt, Ym = rng.normal(size=(3, 2, 2)) * 10, rng.normal(size=(2, 2))
    u, xw, yw, tr = run(dict(x=x, Yt=Yt, Ym=Ym, n_ctrl=2, iters=10, noise=warp_ref.NOISE, lam_s=warp_ref.LAM_S, lam_a=warp_ref.LAM_A,
                             lr=warp_ref.LR, weights=None, u0=rng.normal(0.0, 0.4, 2)))
    assert np.all(np.isfinite(u)) and np.all(np.isfinite(xw)) and np.all(np.isfinite(yw)) and np.all(np.isfinite(tr))
    span = x[1] - x[0]
    assert np.all(xw[:, 0] == 0.0) and np.array_equal(yw[:, 0, :], Yt[:, 0, :])
    S = np.logaddexp(0.0, u[:, 1]) + 1e-6 + 1e-12          # u_T[1] is the last control
    assert np.all(np.abs(xw[:, 1] + span * 1e-12 / S) <= 4 * EPS * x[1])
    one_minus_tt = 1e-12 / S + 1e-12 / span + 16 * EPS
    assert np.all(np.abs(yw[:, 1, :] - Yt[:, 1, :]) <= one_minus_tt[:, None] * np.abs(Yt[:, 0, :] - Yt[:, 1, :]) + 4 * EPS * np.abs(Yt[:, 1, :]))


def test_block_index_does_not_leak():
    case = dict(warp_ref.sweep_case("d"))
    B = 5
    rng = np.random.default_rng(9)
    Yt = np.concatenate([case["Yt"], case["Yt"] + rng.normal(size=case["Yt"].shape), case["Yt"][:1]])
    Ym = np.concatenate([case["Ym"], case["Ym"], case["Ym"][:1]])
    assert Yt.shape[0] == B and np.array_equal(Yt[0], Yt[B - 1]) and np.array_equal(Ym[0], Ym[B - 1])
    w = np.array([0.6, 1.0, 0.3, 0.8, 0.6])
    for weights in (None, w):
        u, xw, yw, tr = run(case, Yt=Yt, Ym=Ym, weights=weights)
        for a in (u, xw, yw, tr):
            assert np.array_equal(a[0], a[B - 1])
        assert not np.array_equal(u[0], u[1])


def test_status_codes():
    lib = _ffi.lib
    T, B, D, n = 257, 2, 5, 33                            # every buffer large enough for every call below
    x = torch.arange(T, dtype=torch.float64, device="cuda")
    Yt = torch.zeros((B, T, D), dtype=torch.float64, device="cuda")
    Ym = torch.zeros((T, D), dtype=torch.float64, device="cuda")
    outs = [torch.full(s, float("nan"), dtype=torch.float64, device="cuda") for s in ((B, n), (B, T), (B, T, D), (B, 4, 4))]
    p = lambda t: ctypes.c_void_p(t.data_ptr())           # noqa: E731
    z = ctypes.c_void_p(0)

    def call(T=16, B=2, D=1, n=4, iters=4, noise=1.0):
        rc = lib.hgp_warp_batch_f64(p(x), p(Yt), p(Ym), 0, T, B, D, n, iters, noise, 200.0, 1e-3, 5e-2, z, z, *(p(o) for o in outs), z)
        torch.cuda.synchronize()
        return rc

    assert call(T=1) == -1 and call(n=1) == -1 and call(D=0) == -1 and call(iters=-1) == -1 and call(noise=float("nan")) == -1
    assert call(T=257) == -2 and call(D=5) == -2 and call(n=33) == -2
    assert call(B=0) == 0
    assert all(bool(torch.isnan(o).all()) for o in outs)   # none of the calls above wrote anything
    assert call() == 0 and bool(torch.isfinite(outs[0].reshape(-1)[:8]).all())   # u [2,4] at the head of its buffer
