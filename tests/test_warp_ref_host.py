"""The CPU references of the warp fit (tests/warp_ref.py) before the device is held to them: warp_autograd reproduces the
reference project's recorded outputs (tests/golden/warp_batch.npz), the hand-derived restatement agrees with autograd on every
case of the device sweep (the printed deviations are the CPU floor quoted in tests/test_gpu_warp_kernel.py), and no sweep case
puts a sample on a knot of the interpolant, where the gradient would depend on rounding."""
import numpy as np
import pytest

from conftest import golden

import warp_ref
from hdpgpc_amd.amtgp_warping_system import Warping_system


def test_autograd_reproduces_recorded_outputs():
    g = golden("warp_batch.npz")
    for i in range(int(g["n_cases"])):
        iters, recursive, reps, n_ctrl, lr, ls, la, nw, lo, hi = g[f"c{i}_meta"]
        th = g[f"c{i}_theta"]
        theta = None if np.isnan(th[0]) else (float(th[0]) if th.size == 1 else tuple(float(v) for v in th))
        x = g[f"c{i}_x"]
        ws = Warping_system(x[:, None], noise_warp=float(nw), bound_noise_warp=(float(lo), float(hi)), recursive=bool(recursive),
                            lambda_smooth=float(ls), lambda_amp=float(la), device="cpu")
        lam_s, lam_a = ws._theta_to_lambdas(theta)
        noise = float(np.clip(g[f"c{i}_noise"].mean(), lo, hi))
        w = g[f"c{i}_w"] if f"c{i}_w" in g.files else None
        wn = np.ones(g[f"c{i}_Yt"].shape[0]) if w is None else np.maximum(w, 0.0)
        u0 = None
        for rep in range(int(reps)):
            u, xw, yw, tr, _ = warp_ref.warp_autograd(x, g[f"c{i}_Yt"], g[f"c{i}_Ym"], int(n_ctrl), int(iters), noise, lam_s, lam_a,
                                                      float(lr), weights=w, u0=u0)
            ref_xw, ref_yw, ref_loss = g[f"c{i}_r{rep}_xw"], g[f"c{i}_r{rep}_yw"], g[f"c{i}_r{rep}_loss"]
            loss = np.einsum("b,bi->i", wn, tr[:, :, 0]) / (wn.sum() + 1e-12)
            print(f"golden case {i} rep {rep}: loss {np.max(np.abs(loss / ref_loss - 1)):.2e}  "
                  f"x_warp {np.max(np.abs(xw - ref_xw)) / np.max(np.abs(ref_xw)):.2e}  "
                  f"y_warp {np.max(np.abs(yw - ref_yw)) / np.max(np.abs(ref_yw)):.2e}")
            assert np.allclose(loss, ref_loss, rtol=1e-9, atol=0.0), (i, rep)
            assert np.max(np.abs(xw - ref_xw)) <= 1e-9 * np.max(np.abs(ref_xw)), (i, rep)
            assert np.max(np.abs(yw - ref_yw)) <= 1e-9 * np.max(np.abs(ref_yw)), (i, rep)
            if recursive:
                u0 = u.mean(axis=0)                      # the warm start across calls: mean control vector of the last one


@pytest.mark.parametrize("name", sorted(warp_ref.SWEEP))
def test_restated_agrees_with_autograd(name):
    case = warp_ref.sweep_case(name)
    ref = warp_ref.sweep_reference(name)
    got = warp_ref.warp_restated(**case)
    dev = warp_ref.deviations(got, ref, case)
    print(f"CPU floor, case {name}: " + "  ".join(f"{k} {v:.2e}" for k, v in dev.items()))
    for k, v in dev.items():
        assert v <= 1e-12, (name, k, v)
    w = case["weights"]
    if w is not None:                                    # a sample without weight is never moved
        u0 = np.zeros(case["n_ctrl"]) if case["u0"] is None else case["u0"]
        for u in (got[0], ref[0]):
            assert np.array_equal(u[w <= 0], np.broadcast_to(u0, u[w <= 0].shape))


@pytest.mark.parametrize("name", sorted(warp_ref.SWEEP))
def test_no_sample_sits_on_a_knot(name):
    case = warp_ref.sweep_case(name)
    margin = warp_ref.sweep_reference(name)[4]
    print(f"knot margin, case {name}: {margin:.2e}" + (" (from the second forward pass on)" if name in warp_ref.FLAT_START else ""))
    assert margin >= 1e-9, (name, margin)
    if name in warp_ref.FLAT_START:
        # g == x up to rounding in the first pass: the intervals chosen there must not depend on the rounding of the scan
        B, n = case["Yt"].shape[0], case["n_ctrl"]
        u0 = np.zeros((B, n)) + (0.0 if case["u0"] is None else case["u0"][None, :])
        ih64 = warp_ref.intervals(warp_ref.forward_grid(u0, case["x"])[0], case["x"])[0]
        xl = case["x"].astype(np.longdouble)
        ihld = warp_ref.intervals(warp_ref.forward_grid(u0, xl, dtype=np.longdouble)[0], xl)[0]
        assert np.array_equal(ih64, ihld), (name, np.nonzero(ih64 != ihld))
