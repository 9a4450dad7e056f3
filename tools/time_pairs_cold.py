"""The pair path when NOTHING carries over between calls:  python tools/time_pairs_cold.py T N K [reps]
Every call scores another batch of grids (two batches alternate, so each call finds the segment-operator store of
PairsPlan.loglik filled for the other one and rebuilds every record), against the same loop with one batch (every record kept).
Events around PairsPlan.loglik only; prints ms per call for both loops.  Runs unchanged on a tree without the store, where the
two loops do the same work."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import synthetic_workload as synth
from hdpgpc_amd import ops

T, N, K = (int(v) for v in sys.argv[1:4])
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
d = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731
b = synth.synthetic_batch(N, K, T, seed=20260703)
b2 = synth.synthetic_batch(N, K, T, seed=20260704)
plan = ops.PairsPlan(T, T, b["theta"])
plan.update(d(b["xb"]), d(b["mean"]), d(b["Sigma"]))
xs, y = [d(b["x"]), d(b2["x"])], d(b["y"])


def loop(grids):
    for i in range(4):
        quad, _, info = plan.loglik(grids[i % len(grids)], y, want_logdet=False)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        quad, _, info = plan.loglik(grids[i % len(grids)], y, want_logdet=False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps, float(quad.sum()), int(info.abs().max())


warm = loop(xs[:1])
cold = loop(xs)
print(f"T={T} N={N} K={K} store={'yes' if getattr(plan, '_segops', None) is not None else 'no'}: same grids every call "
      f"{warm[0]:.4f} ms/call, other grids every call {cold[0]:.4f} ms/call, checksums {warm[1]:.10e} {cold[1]:.10e}, "
      f"info {max(warm[2], cold[2])}")
