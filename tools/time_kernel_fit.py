"""Time the batched kernel hyper-parameter fit (hgp_kernel_fit_steps_f64) on the device against the host-driven fit it restates
(kernel_fit.fit_kernel_adam): device events around a synchronise, after a warm-up, one process.  Per T (90: beats of record 100;
171: the same beats resampled to the ocean notebook's length) and B in {1, 8, 64, 256}: one call of 1 000 Adam iterations
(min_iter = 10**9: no fit stops), repeated `reps` times ALTERNATING with 1 000 iterations of fit_kernel_adam on beat 0 of the
same batch.  Records the time per call and per Adam step, the spread of both paths, the two acceptance ratios of the feature
(B = 64 against 64 single host-driven fits; B = 1 against one) and the agreement of the two paths' final theta.
Writes profiles/kernel_fit_batch.json.

    python tools/time_kernel_fit.py [--out profiles/kernel_fit_batch.json] [--reps 3] [--iters 1000]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hdpgpc_amd import _ffi, ops  # noqa: E402
from hdpgpc_amd.kernel_fit import fit_kernel_adam, theta_of_state  # noqa: E402

BOUNDS = (1e-3, 20.0)
NEVER = 10 ** 9
SIZES_B = (1, 8, 64, 256)


def beats(T, n):
    y90 = np.load(os.path.join(ROOT, "tests", "golden", "mitbih100_lead0.npz"))["y"][:n].astype(np.float64)
    if T == 90:
        return y90
    tt = np.linspace(0, 89, T)
    return np.stack([np.interp(tt, np.arange(90.0), r) for r in y90])


def one_T(T, reps, iters):
    Yall = beats(T, max(SIZES_B))
    x = np.arange(float(T))
    xd = torch.as_tensor(x, device="cuda")
    runs = {}
    for B in SIZES_B:
        Yd = torch.as_tensor(Yall[:B], device="cuda").contiguous()
        bd = torch.as_tensor(np.tile(BOUNDS, (B, 1)), device="cuda").contiguous()
        state = torch.zeros((B, _ffi.FIT_STATE_DOUBLES), dtype=torch.float64, device="cuda")
        status = torch.zeros(B, dtype=torch.int32, device="cuda")

        def call(n, state=state, status=status, Yd=Yd, bd=bd):
            state.zero_()
            status.zero_()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.kernel_fit_steps(xd, Yd, bd, state, status, n, lr=0.1, min_iter=NEVER, max_iter=NEVER)
            b.record()
            b.synchronize()
            return a.elapsed_time(b)

        runs[B] = {"call": call, "state": state, "status": status, "ms": []}
        call(20)                                                                # warm-up: code objects, workspace, LDS attributes
    fit_kernel_adam(x, Yall[0], BOUNDS, max_iter=20, min_iter=NEVER)           # warm-up of the host-driven path
    torch.cuda.synchronize()
    parent_ms, parent_theta = [], None
    for _ in range(reps):                                                       # alternate the two paths
        for B in SIZES_B:
            runs[B]["ms"].append(runs[B]["call"](iters))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        parent_theta = fit_kernel_adam(x, Yall[0], BOUNDS, max_iter=iters, min_iter=NEVER)
        torch.cuda.synchronize()
        parent_ms.append((time.perf_counter() - t0) * 1e3)                      # host-driven: wall clock around a synchronise
    rec = {"T": T, "iters": iters, "parent_fit_kernel_adam_ms": float(np.median(parent_ms)), "parent_all_ms": parent_ms,
           "parent_us_per_step": float(np.median(parent_ms)) * 1e3 / iters, "batch": []}
    for B in SIZES_B:
        ms = float(np.median(runs[B]["ms"]))
        th = theta_of_state(runs[B]["state"].cpu().numpy(), np.tile(BOUNDS, (B, 1)))
        assert runs[B]["status"].cpu().numpy().tolist() == [0] * B
        rec["batch"].append({"B": B, "call_ms": ms, "call_all_ms": runs[B]["ms"], "us_per_step": ms * 1e3 / iters,
                             "us_per_step_per_fit": ms * 1e3 / iters / B,
                             "ratio_to_B_parent_fits": ms / (B * rec["parent_fit_kernel_adam_ms"]),
                             "theta_fit0_max_rel_diff_vs_parent": float(np.max(np.abs(th[0] - np.asarray(parent_theta)) /
                                                                               np.abs(np.asarray(parent_theta))))})
    by_B = {r["B"]: r for r in rec["batch"]}
    rec["accept_B64_under_64_parent_fits"] = bool(by_B[64]["call_ms"] < 64 * rec["parent_fit_kernel_adam_ms"])
    rec["accept_B1_not_slower_than_parent"] = bool(by_B[1]["call_ms"] <= rec["parent_fit_kernel_adam_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_fit_batch.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "bounds": BOUNDS,
           "sizes": [one_T(90, a.reps, a.iters), one_T(171, a.reps, a.iters)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
