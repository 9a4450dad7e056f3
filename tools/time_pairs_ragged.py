"""Timings of the ragged pair call (PairsPlan.loglik(lengths=...)):   python tools/time_pairs_ragged.py [repeats]

1. cost of raggedness: 2 048 x 8 pairs at T = 128 and at T = 90, the rectangular call against a ragged call whose lengths are all T;
2. what it buys: 2 048 segments, K = 8, T = 128, lengths uniform in 60 .. 128 (fixed seed): ONE ragged call against one
   rectangular call per distinct length on the same plan (sub-batches gathered beforehand: only launches and kernels are timed),
   with a check that the two give the same bits.
Device events around windows of 20 calls after a warm-up of every shape; the two calls of a comparison take their windows in turns,
`repeats` (default 5) each; one JSON line per measurement with every window, min, median and max."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import synthetic_workload as synth
from hdpgpc_amd import ops

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 20
N, K = 2048, 8
d = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731


def window(fn):
    """ms per call of fn() over one window of REPS calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


def alternating(fa, fb):
    """REPEATS windows of each of two calls, taken in turns after a warm-up of both."""
    for _ in range(3):
        fa(), fb()
    a, b_ = [], []
    for _ in range(REPEATS):
        a.append(window(fa))
        b_.append(window(fb))
    return a, b_


def report(what, ms, **more):
    print(json.dumps({"what": what, "ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4),
                      "ms_max": round(max(ms), 4), "runs": [round(v, 4) for v in ms], **more}), flush=True)
    return statistics.median(ms)


def plan_for(T, b):
    return ops.PairsPlan(T, T, b["theta"]).update(d(b["xb"]), d(b["mean"]), d(b["Sigma"]))


for T in (128, 90):
    b = synth.synthetic_batch(N, K, T, seed=20260703)
    plan, x, y = plan_for(T, b), d(b["x"]), d(b["y"])
    full = torch.full((N,), T, dtype=torch.int32, device="cuda")
    q0 = plan.loglik(x, y, want_logdet=False)[0]
    q1 = plan.loglik(x, y, want_logdet=False, lengths=full)[0]
    same = bool(torch.equal(q0, q1))
    rect, rag = alternating(lambda: plan.loglik(x, y, want_logdet=False), lambda: plan.loglik(x, y, want_logdet=False, lengths=full))
    m0 = report(f"rectangular T={T} {N}x{K}", rect)
    m1 = report(f"ragged, all lengths = {T}, T={T} {N}x{K}", rag, same_bits_as_rectangular=same)
    print(f"T={T}: ragged / rectangular = {m1 / m0:.4f}", flush=True)

T = 128
b = synth.synthetic_batch(N, K, T, seed=20260703)
rng = np.random.default_rng(20260703)
lens = rng.integers(60, T + 1, N).astype(np.int32)
X, Y = b["x"].copy(), b["y"].copy()
for n, L in enumerate(lens):
    X[n, L:], Y[n, L:] = np.nan, np.nan
plan, Xd, Yd, lens_d = plan_for(T, b), d(X), d(Y), torch.as_tensor(lens, device="cuda")
groups = []
for L in np.unique(lens):
    rows = np.nonzero(lens == L)[0]
    groups.append((rows, d(np.ascontiguousarray(X[rows, :L])), d(np.ascontiguousarray(Y[rows, :L]))))


def per_length():
    return [plan.loglik(xg, yg, want_logdet=False)[0] for _, xg, yg in groups]


q = plan.loglik(Xd, Yd, want_logdet=False, lengths=lens_d)[0]
same = all(bool(torch.equal(q[torch.as_tensor(rows, device="cuda")], qg)) for (rows, _, _), qg in zip(groups, per_length()))
one, many = alternating(lambda: plan.loglik(Xd, Yd, want_logdet=False, lengths=lens_d), per_length)
m1 = report(f"one ragged call, lengths 60..128, T=128 {N}x{K}", one)
m2 = report(f"{len(groups)} rectangular calls, one per distinct length, same pairs", many, same_bits_as_ragged=same,
            launches_per_call_set=len(groups))
print(f"per-length calls / one ragged call = {m2 / m1:.2f}", flush=True)
