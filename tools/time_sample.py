"""Time the draws from many states (hgp_sample_states_f64) on the device against the composition the library offered before:
ops.potrf_batched + ops.gemm_batched(z, L, transB=True) + the mean add.  Event timing after a warm-up; every timed window holds
`inner` calls; the two paths alternate window by window in one process; median over `reps` windows, the spread is the
interquartile range over the median (minimum and maximum are recorded too).  Distinct covariance per state, shared normals.
Writes profiles/sample_timing.json.

    python tools/time_sample.py [--out profiles/sample_timing.json] [--reps 15] [--inner 10]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hdpgpc_amd import _ffi, ops  # noqa: E402

PEAK_F64_MFMA = 78.6e12
PEAK_HBM = 8.0e12
SHAPES = [(64, 90, 256), (8, 256, 1024), (512, 90, 16)]


def states(S, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = torch.randn((S, T, 6), dtype=torch.float64, device="cuda", generator=g)
    d = 0.1 + 0.3 * torch.rand((S, T), dtype=torch.float64, device="cuda", generator=g)
    cov = (0.05 * ops.gemm_batched(B, B, transB=True) + torch.diag_embed(d)).contiguous()
    mean = torch.randn((S, T), dtype=torch.float64, device="cuda", generator=g)
    return mean, cov


def window_ms(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def stats(t):
    t = np.asarray(t)
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"median_ms": float(med), "iqr_over_median": float((q3 - q1) / med), "min_ms": float(t.min()), "max_ms": float(t.max()),
            "all_ms": [float(v) for v in t]}


def algorithmic(S, T, n):
    """What the algorithm needs: the factor reads cov and writes L once per state (T^3 / 3 flop), every draw costs T^2 flop
    (half a square product) and 8 T bytes out; the shared normals and L are read once (they stay in L2 across the panels)."""
    flop = S * (T ** 3 / 3.0 + float(n) * T * T)
    byts = 8.0 * (S * (3 * T * T + T) + n * T + S * n * T)
    return flop, byts


def one(S, T, n, reps, inner):
    mean, cov = states(S, T, 1)
    z = torch.randn((n, T), dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    out = torch.empty((S, n, T), dtype=torch.float64, device="cuda")
    info = torch.zeros(S, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.sample_ws_doubles(S, T), dtype=torch.float64, device="cuda")
    P = ops._ptr

    def fused():
        _ffi.check(_ffi.lib.hgp_sample_states_f64(P(mean), P(cov), None, T, S, P(z), n, 1, 0.0, P(out), P(info), P(ws), ws.numel() * 8, ops._stream()),
                   "sample_states")

    def composed():
        L, _ = ops.potrf_batched(cov, 0.0, 0.0)
        return ops.gemm_batched(z, L, transB=True) + mean[:, None, :]

    for _ in range(3):
        fused()
        ref = composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(reps):                                      # alternating windows
        tf.append(window_ms(fused, inner))
        tc.append(window_ms(composed, inner))
    flop, byts = algorithmic(S, T, n)
    rec = {"S": S, "T": T, "n": n, "fused": stats(tf), "composition": stats(tc), "algorithmic_flop": flop, "algorithmic_bytes": byts}
    floor_ms = max(flop / PEAK_F64_MFMA, byts / PEAK_HBM) * 1e3
    rec["roofline_bound"] = "fp64 MFMA" if flop / PEAK_F64_MFMA > byts / PEAK_HBM else "HBM"
    rec["roofline_floor_ms"] = floor_ms
    rec["roofline_fraction"] = floor_ms / rec["fused"]["median_ms"]
    rec["fused_over_composition"] = rec["fused"]["median_ms"] / rec["composition"]["median_ms"]
    rec["not_slower_within_spread"] = bool(rec["fused"]["median_ms"] <= rec["composition"]["median_ms"] * (1.0 + rec["composition"]["iqr_over_median"]))
    rec["check_max_abs_diff_vs_composition"] = float((out - ref).abs().max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_timing.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "peak_f64_mfma": PEAK_F64_MFMA, "peak_hbm": PEAK_HBM,
           "method": f"HIP events, {a.inner} calls per window, {a.reps} alternating windows per path, median; spread = IQR / median",
           "sizes": [one(S, T, n, a.reps, a.inner) for S, T, n in SHAPES]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
