"""Time a chain with an estimation limit: GPI_model.full_pass_weighted on one 200-member chain of record 100 (T = 90, and
resampled to T = 144) with E = 30 - the eager path (all a limited model had before the frozen step existed) against the graphed
path - and the frozen member step against the full graphed one (E = 2: every graphed step frozen; no limit: none).  Then the
online step on tests/golden/include_sample_r102_n40_el4.npz: the pool against the one-by-one path (OnlinePool.supports forced
false).  Alternating runs; per figure the median and the spread (max - min) of the runs.

    python tools/time_estlimit.py [runs [chains|online]]
"""
import io
import os
import sys
import time
from contextlib import redirect_stdout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from hdpgpc_amd.GPI import RBFWhiteKernel  # noqa: E402
from hdpgpc_amd.GPI_model import GPI_model  # noqa: E402

RUNS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WHAT = sys.argv[2:] or ["chains", "online"]
N = 200
d = np.load(os.path.join(ROOT, "tests", "golden", "mitbih100_lead0.npz"))["y"][:N]


def chain(T, E, use_graphs):
    t = np.linspace(0, d.shape[1] - 1, T)
    y = d if T == d.shape[1] else np.stack([np.interp(t, np.arange(d.shape[1]), r) for r in d])
    m = GPI_model(RBFWhiteKernel(300.0, 3.0, 9e-5), np.arange(float(T))[:, None], annealing=True, bayesian=True,
                  estimation_limit=E, free_deg_MNIV=5)
    cond = m.GPR_dynamic(12.0, 9.0)
    m.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    m.fixed_theta, m.noise_bounds = (341.0, 1.2, 4.66), (9e-5, 18.0)
    xs = m.cond_to_torch(np.repeat(np.arange(float(T))[None, :, None], N, axis=0))
    ys = m.cond_to_torch(y[:, :, None])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m.full_pass_weighted(xs, ys, torch.ones(N), use_graphs=use_graphs)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert len(m.A) == min(N + 1, m.estimation_limit) and (getattr(m, "graph_replays", 0) > 0) == use_graphs
    return dt / N * 1e6                                    # us per member (forward steps, RTS pass and both score calls)


def online(pool_on):
    import estlimit_trace as et
    from hdpgpc_amd.online_chain import OnlinePool
    g = np.load(os.path.join(ROOT, "tests", "golden", "include_sample_r102_n40_el4.npz"))
    real = OnlinePool.__dict__["supports"]
    if not pool_on:
        OnlinePool.supports = staticmethod(lambda g_: False)
    try:
        sw, xb, data = et.online_mirror(g)
        secs = []
        with redirect_stdout(io.StringIO()):
            for i in range(data.shape[0]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sw.include_sample(xb, data[i], with_warp=False)
                torch.cuda.synchronize()
                secs.append(time.perf_counter() - t0)
    finally:
        OnlinePool.supports = real
    assert [len(m.indexes) for m in sw.gpmodels[0]] == g[f"b{data.shape[0] - 1}_counts"].tolist()
    return float(np.mean(secs[8:])) * 1e3                  # ms per beat, beats 8..39 (clusters past the limit exist from beat 7)


def report(name, cases, unit):
    for fn in cases.values():                              # warm-up: allocator, plan caches, first-use kernel loads
        fn()
    res = {k: [] for k in cases}
    for _ in range(RUNS):
        for k, fn in cases.items():                        # alternating
            res[k].append(fn())
    for k, v in res.items():
        print(f"{name} {k}: median {np.median(v):.1f} {unit}, spread {max(v) - min(v):.1f} ({', '.join(f'{x:.1f}' for x in v)})", flush=True)
    return {k: float(np.median(v)) for k, v in res.items()}


for T in (90, 144) if "chains" in WHAT else ():
    r = report(f"T={T} 200 members, us per member:", {
        "E=30 eager": lambda: chain(T, 30, False), "E=30 graphed": lambda: chain(T, 30, True),
        "E=2 graphed (all steps frozen)": lambda: chain(T, 2, True), "no limit graphed (all steps full)": lambda: chain(T, None, True)}, "us")
    print(f"T={T}: eager / graphed at E = 30: {r['E=30 eager'] / r['E=30 graphed']:.1f}x; frozen step saves "
          f"{r['no limit graphed (all steps full)'] - r['E=2 graphed (all steps frozen)']:.1f} us per member of the full graphed step", flush=True)
if "online" in WHAT:
    report("online, include_sample_r102_n40_el4, ms per beat:", {"pool": lambda: online(True), "one by one": lambda: online(False)}, "ms")
