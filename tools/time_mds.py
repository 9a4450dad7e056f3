"""Time the batched SMACOF embedding (hgp_smacof_steps_f64) on the device: event timing after a warm-up, median of 3, one
process.  Per size n, with B = 4 starts, p = 2 and eps = 0 so that all 300 iterations run: (a) the C-ABI call for 300 passes
(two launches each) and the time per pass; (b) the whole mds.smacof from a host matrix; (c) where scikit-learn is importable,
sklearn.manifold.smacof on this host's CPUs from the same four starts, one after the other as MDS(n_init=4) runs them - at the
sizes up to --sklearn-max-n in full, above that for --sklearn-iters iterations, EXTRAPOLATED linearly and marked so.  The
distance matrix is the Euclidean one of points drifting in three groups (the shape of a cluster history), so every start keeps
moving for the whole run.  Writes profiles/mds_timing.json; `--parity FILE` copies the largest deviations the GPU tests of
tests/test_gpu_mds.py recorded (the parity_observed.json that tests/conftest.py writes at the end of a session) into it.

    python tools/time_mds.py [--out profiles/mds_timing.json] [--reps 3] [--sizes 600 1200 2272]
"""
import argparse
import json
import os
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hdpgpc_amd import _ffi, mds, ops  # noqa: E402

B, P, ITERS = 4, 2, 300
LAUNCHES_PER_ITERATION = 2


def event_ms(fn, reps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), [float(v) for v in t]


def matrix(n, seed=3, dim=6, groups=3):
    rng = np.random.default_rng(seed)
    cur = 5.0 * rng.standard_normal((groups, dim))
    pts = np.empty((n, dim))
    for i in range(n):
        cur[i % groups] += 0.5 * rng.standard_normal(dim)
        pts[i] = cur[i % groups]
    g = pts @ pts.T
    sq = np.diag(g)[:, None] + np.diag(g)[None, :] - 2.0 * g
    D = np.sqrt(np.maximum(0.5 * (sq + sq.T), 0.0))
    np.fill_diagonal(D, 0.0)
    return D


def one(n, reps, sk_max_n, sk_iters):
    D = matrix(n)
    X0 = mds.initial_configurations(n, P, B, 0)
    Dd = torch.as_tensor(D, device="cuda")
    X = torch.empty((B, n, P), dtype=torch.float64, device="cuda")
    X0d = torch.as_tensor(X0, device="cuda")
    state = torch.zeros((B, _ffi.MDS_STATE_DOUBLES), dtype=torch.float64, device="cuda")
    status, n_it = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    stress = torch.zeros(B, dtype=torch.float64, device="cuda")
    ws = torch.empty(ops.smacof_ws_doubles(B, n, P), dtype=torch.float64, device="cuda")
    Pt = ops._ptr

    def entry():
        X.copy_(X0d)
        state.zero_()
        status.zero_()
        _ffi.check(_ffi.lib.hgp_smacof_steps_f64(Pt(Dd), n, n, P, B, Pt(X), 0.0, ITERS, ITERS + 1, Pt(state), Pt(status), Pt(stress),
                                                 Pt(n_it), Pt(ws), ws.numel() * 8, ops._stream()), "smacof_steps")

    rec = {"n": n, "B": B, "p": P, "passes": ITERS, "launches_per_iteration": LAUNCHES_PER_ITERATION, "delta_MB": n * n * 8 / 1e6}
    rec["entry_ms"], rec["entry_all_ms"] = event_ms(entry, reps)
    rec["ms_per_pass"] = rec["entry_ms"] / ITERS
    # every pass reads delta once for the four starts
    rec["delta_GBps_if_read_once_per_pass"] = n * n * 8 / (rec["ms_per_pass"] * 1e-3) / 1e9
    rec["passes_done"] = [int(v) for v in state[:, 0].cpu().numpy()]
    rec["status_after"] = [int(v) for v in status.cpu().numpy()]
    t0 = time.perf_counter()
    _, s_best, it_best, info = mds.smacof(D, n_components=P, init=X0, max_iter=ITERS, eps=0.0)
    rec["mds_smacof_wall_ms"] = (time.perf_counter() - t0) * 1e3
    rec["mds_smacof_n_iter"] = [int(v) for v in info["n_iter"]]
    rec["mds_smacof_stress"] = [float(v) for v in info["stress"]]
    try:
        from sklearn.manifold import smacof as sk_smacof
    except ImportError:
        rec["sklearn"] = None
        return rec
    iters = ITERS if n <= sk_max_n else sk_iters
    t0 = time.perf_counter()
    sk = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for b in range(B):
            sk.append(sk_smacof(D, init=X0[b].copy(), n_init=1, max_iter=iters, eps=0.0, normalized_stress=False, return_n_iter=True))
    sk_ms = (time.perf_counter() - t0) * 1e3
    done = sum(r[2] for r in sk)
    rec["sklearn_iterations_run"] = done
    rec["sklearn_cpus"] = os.cpu_count()
    if iters == ITERS:
        rec["sklearn_ms"] = sk_ms
        rec["sklearn_stress"] = [float(r[1]) for r in sk]
    else:
        rec["sklearn_ms_EXTRAPOLATED"] = sk_ms * B * ITERS / done
        rec["sklearn_note"] = f"{sk_ms:.1f} ms for {done} iterations, times {B * ITERS}/{done}"
    rec["sklearn_ms_per_iteration"] = sk_ms / done
    rec["speedup_vs_sklearn_same_host"] = (sk_ms / done) / rec["ms_per_pass"] * B
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mds_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[600, 1200, 2272])
    ap.add_argument("--sklearn-max-n", type=int, default=600, help="largest n at which scikit-learn runs all 4 x 300 iterations")
    ap.add_argument("--sklearn-iters", type=int, default=10, help="iterations per start above that size (extrapolated)")
    ap.add_argument("--parity", default=None, help="parity_observed.json of a GPU test run: its test_gpu_mds entries are recorded")
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "launches_per_iteration": LAUNCHES_PER_ITERATION,
           "sizes": [one(n, a.reps, a.sklearn_max_n, a.sklearn_iters) for n in a.sizes]}
    if a.parity and os.path.exists(a.parity):
        with open(a.parity) as f:
            obs = {k: v for k, v in json.load(f).items() if "test_gpu_mds" in k}
        res["parity_vs_restatement"] = {"gate": 1e-9, "largest_deviation": max(obs.values()) if obs else None, "per_test": obs}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
