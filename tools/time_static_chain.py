"""Timings of the static filter chain:   python tools/time_static_chain.py [windows]

chain_batch.run over static chains - ONE hgp_static_chain_steps_f64 launch for all of them (one workgroup per chain walks its
members) - against the route the same jobs took before the fused chain existed, GPI_model._full_pass_eager (a dozen launches
and host work per member, one chain after the other):
  1. B = 8 static chains of 250 members each, T = 90;
  2. B = 1 chain of 2 000 members, T = 90.
Both routes include what follows the chain in full_pass_weighted (the scores of every segment under the finished model).  The
kernel alone is timed too (the launch without the Python around it).  Device events around windows of one pass each after a
warm-up, the two routes taking their windows in turns, `windows` (default 5) each; one JSON line per measurement with every
window, and the ratio of the medians.  The eager route at 2 000 members is timed on the first 250 members and SCALED by 8: it is
a host loop, linear in the members."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from hdpgpc_amd import chain_batch, ops
from hdpgpc_amd.GPI import RBFWhiteKernel
from hdpgpc_amd.GPI_model import GPI_model
from hdpgpc_amd.member_step import upload_descs

WINDOWS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
T = 90
d = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def report(what, ms, **more):
    print(json.dumps({"what": what, "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                      "ms_max": round(max(ms), 3), "windows": [round(v, 3) for v in ms], **more}), flush=True)
    return statistics.median(ms)


def beats(N, seed):
    rng = np.random.default_rng(seed)
    u = np.arange(T) / T
    base = 150.0 * np.exp(-0.5 * ((u - 0.4) / 0.06) ** 2) + 20.0 * np.sin(2 * np.pi * u)
    return np.stack([base * (1.0 + 0.05 * rng.standard_normal()) + 3.0 * rng.standard_normal(T) for _ in range(N)])[:, :, None]


def model():
    m = GPI_model(RBFWhiteKernel(300.0, 3.0, 1e-4), np.arange(float(T))[:, None], annealing=True, bayesian=True, free_deg_MNIV=5)
    cond = m.GPR_static(10.0)
    m.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    m.fixed_theta = (341.0, 1.2, 4.66)
    return m


def measure(tag, B, n, n_eager):
    xs = d(np.repeat(np.arange(float(T))[None, :, None], n, axis=0))
    ys = [d(beats(n, 100 + b)) for b in range(B)]
    ones, part = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    part[:n_eager] = 1.0

    def fused():
        return chain_batch.run([chain_batch.Job(model(), xs, y, ones) for y in ys])

    def eager():
        return [m._full_pass_eager(xs, y, part, list(range(n_eager))) for m, y in ((model(), y) for y in ys)]

    def kernel_only():
        eye = torch.eye(T, dtype=torch.float64, device="cuda")
        Sig = 10.0 * eye                                   # (held here: a descriptor carries addresses, not tensors)
        k = RBFWhiteKernel(341.0, 1.2, 4.66)
        keep, descs = [], []
        for y in ys:
            Fs, Ps = torch.zeros((n + 1, T), dtype=torch.float64, device="cuda"), torch.zeros((n + 1, T, T), dtype=torch.float64, device="cuda")
            Ps[0] = k(d(np.arange(float(T))[:, None]), d(np.arange(float(T))[:, None]))
            pos, info = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
            idx = torch.arange(n, dtype=torch.int64, device="cuda")
            Y = y[..., 0].contiguous()
            keep.append((Fs, Ps, pos, info, idx, Y))
            descs.append(ops.static_chain_desc(eye, eye, Sig, Fs, Ps, pos, Y, idx, info, n, 0, first=True, white=4.66))
        dd = upload_descs(descs, "cuda")
        torch.cuda.synchronize()
        t = window(lambda: ops.static_chain_steps(dd, B, T, n))
        assert all(int(k_[3][0]) == 0 and int(k_[2][0]) == n for k_ in keep)
        return t

    for _ in range(2):
        fused(), eager()
    a, b, c = [], [], []
    for _ in range(WINDOWS):
        a.append(window(fused))
        b.append(window(eager) * (n / n_eager))
        c.append(kernel_only())
    m1 = report(f"{tag}: chain_batch.run, fused static chain, B={B} n={n} T={T}", a)
    m2 = report(f"{tag}: _full_pass_eager per chain, {n_eager} members timed" + (f", SCALED by {n}/{n_eager}" if n != n_eager else ""), b)
    m3 = report(f"{tag}: the launch alone", c, us_per_member=round(statistics.median(c) * 1e3 / n, 2))
    print(f"{tag}: eager / fused = {m2 / m1:.1f}   (kernel {m3 * 1e3 / n:.1f} us per member step; B chains side by side)", flush=True)


measure("B=8 x 250", 8, 250, 250)
measure("B=1 x 2000", 1, 2000, 250)
