"""Time the predictive bands of many states on a query grid (hgp_pred_bands_f64) on the device: event timing after a warm-up,
median of 3, one process.  Per size S x T x Q: (a) the C-ABI call (its three launches) and the whole ops.pred_bands; (b) the
same call with Q = 1 (the per-state preparation: K~ and its inverse factor, one query panel); (c) the code path the library
offered before: a loop of GPI_model.observe_last over the same states - at most 16 of them are run, larger S is
EXTRAPOLATED linearly and marked so.  Writes profiles/bands_timing.json.

    python tools/time_bands.py [--out profiles/bands_timing.json] [--reps 3]
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
from hdpgpc_amd.GPI import RBFWhiteKernel  # noqa: E402
from hdpgpc_amd.GPI_model import GPI_model  # noqa: E402

PEAK_F64_MFMA = 78.6e12
THETA = (1.0, 1.2, 0.05)
LOOP_MAX = 16


def event_ms(fn, reps, warmup=2):
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


def states(S, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    B = torch.randn((S, T, 6), dtype=torch.float64, device="cuda", generator=g)
    d = 0.1 + 0.3 * torch.rand((S, T), dtype=torch.float64, device="cuda", generator=g)
    Sig = (0.05 * ops.gemm_batched(B, B, transB=True) + torch.diag_embed(d)).contiguous()
    mean = torch.randn((S, T), dtype=torch.float64, device="cuda", generator=g)
    return mean, Sig


def executed_flop(S, T, Q):
    """MFMA flops k_bands executes: per (state, 16-wide query tile) 4 nb^2 + 2 nb products of 16 x 16 x 16 (two full and four
    block-triangular T x T operands), nb = ceil(T / 16); the query tiles come in panels of 4 (T <= 128) or 2."""
    nb = -(-T // 16)
    ct = 4 if nb <= 8 else 2
    tiles = -(-Q // (16 * ct)) * ct
    return float(S) * tiles * (4 * nb * nb + 2 * nb) * 2 * 16 ** 3


def one(S, T, Q, reps):
    mean, Sig = states(S, T, 1)
    xb = torch.arange(T, dtype=torch.float64, device="cuda")
    xq = torch.arange(Q, dtype=torch.float64, device="cuda") * ((T - 1) / Q)
    theta = torch.tensor([THETA] * S, dtype=torch.float64, device="cuda")
    mq, vq = torch.empty((S, Q), dtype=torch.float64, device="cuda"), torch.empty((S, Q), dtype=torch.float64, device="cuda")
    info = torch.zeros(S, dtype=torch.int32, device="cuda")
    ws = torch.empty(ops.pred_bands_ws_doubles(S, T), dtype=torch.float64, device="cuda")
    P = ops._ptr

    def entry(q):
        _ffi.check(_ffi.lib.hgp_pred_bands_f64(P(xb), T, P(theta), P(mean), P(Sig), None, S, P(xq), q, P(mq), P(vq), P(info), P(ws), ws.numel() * 8,
                                               ops._stream()), "pred_bands")

    n_loop = min(S, LOOP_MAX)
    eye = np.eye(T)[None]
    models = []
    for s in range(n_loop):
        m = GPI_model(RBFWhiteKernel(*THETA, device="cuda"), np.arange(float(T)))
        f = mean[s].cpu().numpy()[None]
        m.load_state(f, Sig[s].cpu().numpy()[None], eye, [0], f_star_sm=f)
        models.append(m)
    xq_col = xq.reshape(-1, 1)

    def loop():
        for m in models:
            m.observe_last(xq_col)

    rec = {"S": S, "T": T, "Q": Q, "executed_mfma_flop": executed_flop(S, T, Q)}
    rec["entry_ms"], rec["entry_all_ms"] = event_ms(lambda: entry(Q), reps)
    rec["entry_q1_ms"], _ = event_ms(lambda: entry(1), reps)
    rec["ops_pred_bands_ms"], _ = event_ms(lambda: ops.pred_bands(xb, theta, mean, Sig, xq), reps)
    loop_ms, _ = event_ms(loop, reps, warmup=1)
    rec["observe_last_loop_states_run"] = n_loop
    if n_loop == S:
        rec["observe_last_loop_ms"] = loop_ms
    else:
        rec["observe_last_loop_ms_EXTRAPOLATED"] = loop_ms * S / n_loop
        rec["observe_last_loop_note"] = f"{loop_ms:.3f} ms for {n_loop} states, times {S}/{n_loop}"
    rec["speedup_vs_loop"] = loop_ms * S / n_loop / rec["entry_ms"]
    rec["frac_peak_on_executed_flop"] = rec["executed_mfma_flop"] / (rec["entry_ms"] * 1e-3) / PEAK_F64_MFMA
    m0, v0 = models[0].observe_last(xq_col)
    entry(Q)
    rec["check_max_rel_var_vs_loop_state0"] = float(((vq[0] - torch.diagonal(v0)).abs() / torch.diagonal(v0).abs()).max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bands_timing.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "peak_f64_mfma": PEAK_F64_MFMA,
           "sizes": [one(16, 90, 891, a.reps), one(2000, 90, 891, a.reps), one(16, 256, 2551, a.reps)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
