"""Timings of the ragged projection (ops.project_ragged):   python tools/time_project.py [windows]

ONE project_ragged call for the whole batch against the only way without it: IterativeGaussianProcess.projection_matrix (five
launches, a [T, T*] matrix in HBM and a host look at info per segment) plus one product per segment.  The per-segment way is
timed on a SAMPLE of 64 segments (the first 64 of the batch) and SCALED by N / 64: it is a host loop, linear in N.
  1. N = 2 048, T = 128, lengths uniform in 60 .. 128 (fixed seed), two leads;
  2. the same with every length = 128;
  3. N = 256, T = 256, lengths uniform in 129 .. 256 (the cooperative range).
Kernel c = 300, length-scale 3.0 (the drivers'), unit grids with jitter.  Device events around windows of calls (10 calls of
project_ragged, one pass over the sample for the loop) after a warm-up, the two ways taking their windows in turns, `windows`
(default 7) each; one JSON line per measurement with every window, and the ratio of the medians."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hdpgpc_amd import ops
from hdpgpc_amd.GPI import IterativeGaussianProcess, RBFWhiteKernel

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS, SAMPLE = 10, 64
C_OUT, ELL, D = 300.0, 3.0, 2
d = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731


def window(fn, reps):
    """ms per call of fn() over one window of `reps` calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def report(what, ms, **more):
    print(json.dumps({"what": what, "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                      "ms_max": round(max(ms), 4), "windows": [round(v, 4) for v in ms], **more}), flush=True)
    return statistics.median(ms)


def workload(N, T, lo, hi, ld, seed=20260703):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, N).astype(np.int32)
    X, Y = np.full((N, ld), np.nan), np.full((N, ld, D), np.nan)
    for n, L in enumerate(lens):
        x = np.arange(L, dtype=np.float64) * ((T - 1.0) / max(L - 1.0, 1.0) if L > T else 1.0) + rng.uniform(-0.3, 0.3, L)
        u = x / T
        X[n, :L] = x
        Y[n, :L, 0] = 150.0 * np.exp(-0.5 * ((u - 0.4) / 0.06) ** 2) + 20.0 * np.sin(2 * np.pi * u) + rng.standard_normal(L)
        Y[n, :L, 1] = -60.0 * np.exp(-0.5 * ((u - 0.55) / 0.04) ** 2) + 10.0 * np.cos(3 * np.pi * u) + rng.standard_normal(L)
    return lens, X, Y


def measure(tag, N, T, lo, hi, ld):
    lens, X, Y = workload(N, T, lo, hi, ld)
    xb = d(np.arange(T, dtype=np.float64))
    Xd, Yd, lens_d = d(X), d(Y), torch.as_tensor(lens, device="cuda")
    gp = IterativeGaussianProcess(RBFWhiteKernel(C_OUT, ELL, 1.0), xb.reshape(-1, 1))
    seg = [(d(X[n, :L]).reshape(-1, 1), d(Y[n, :L])) for n, L in enumerate(lens[:SAMPLE])]

    def one_call():
        return ops.project_ragged(Xd, Yd, lens_d, xb, C_OUT, ELL)[0]

    def per_segment():
        return [ops.gemm_batched(gp.projection_matrix(xb, x), y) for x, y in seg]

    yp = one_call()
    worst = max(float((yp[n] - p).abs().max() / p.abs().max()) for n, p in enumerate(per_segment()))
    for _ in range(2):
        one_call(), per_segment()
    a, b = [], []
    for _ in range(WINDOWS):
        a.append(window(one_call, REPS))
        b.append(window(per_segment, 1) * (N / SAMPLE))
    m1 = report(f"{tag}: one project_ragged call, N={N} T={T} ld={ld} D={D}", a)
    m2 = report(f"{tag}: projection_matrix + product per segment, {SAMPLE} segments timed, SCALED by {N}/{SAMPLE}", b,
                max_rel_diff_to_the_one_call=worst)
    print(f"{tag}: per-segment way / one call = {m2 / m1:.1f}   ({m1 * 1e3 / N:.2f} us per segment in the one call)", flush=True)


measure("lengths 60..128", 2048, 128, 60, 128, 128)
measure("all lengths 128", 2048, 128, 128, 128, 128)
measure("lengths 129..256", 256, 256, 129, 256, 256)
