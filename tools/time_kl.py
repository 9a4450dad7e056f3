"""Time the symmetric-KL distance matrix (hgp_kl_sym_f64) on the device: event timing over repeated launches after a warm-up,
one process.  Per size: (a) the kernel alone and the whole ops.kl_sym (inversion included); (b) the composition the library
offered before for the same Frobenius terms, ops.gemm_batched with batch 1, M = N = n, K = T^2 (two products); (c) the
reference's formula on the host (tests/kl_ref.py, sampled pairs, EXTRAPOLATED to all pairs).  Writes profiles/kl_timing.json.

    python tools/time_kl.py [--out profiles/kl_timing.json] [--reps 5]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hdpgpc_amd import _ffi, ops  # noqa: E402
import kl_ref  # noqa: E402

PEAK_F64_MFMA = 78.6e12


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


def states(n, T, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    W = torch.randn((n, T, T), dtype=torch.float64, device="cuda", generator=g)
    cov = ops.gemm_batched(W, W, transB=True) / T + torch.eye(T, dtype=torch.float64, device="cuda")
    cov = 0.5 * (cov + cov.transpose(1, 2)).contiguous()
    mean = torch.randn((n, T), dtype=torch.float64, device="cuda", generator=g)
    return mean, cov


def one(n, T, reps):
    mean, cov = states(n, T, 1)
    prec = ops._kl_precisions(cov, "state")
    out = torch.empty((n, n), dtype=torch.float64, device="cuda")
    P = ops._ptr

    def kernel():
        _ffi.check(_ffi.lib.hgp_kl_sym_f64(P(mean), P(cov), P(prec), n, None, None, None, 0, T, P(out), ops._stream()), "kl")

    def kernel_rect():
        _ffi.check(_ffi.lib.hgp_kl_sym_f64(P(mean), P(cov), P(prec), n, P(mean), P(cov), P(prec), n, T, P(out), ops._stream()), "kl")

    cf, pf = cov.reshape(n, T * T), prec.reshape(n, T * T)
    g1, g2 = torch.empty((n, n), dtype=torch.float64, device="cuda"), torch.empty((n, n), dtype=torch.float64, device="cuda")

    def before():
        ops.gemm_batched(cf, pf, transB=True, out=g1)
        ops.gemm_batched(pf, cf, transB=True, out=g2)

    rec = {"n": n, "T": T, "flop_4n2T2": 4.0 * n * n * T * T}
    rec["kernel_self_ms"], rec["kernel_self_all_ms"] = event_ms(kernel, reps)
    rec["kernel_rect_ms"], _ = event_ms(kernel_rect, reps)
    rec["ops_kl_sym_ms"], _ = event_ms(lambda: ops.kl_sym(mean, cov), reps)
    rec["before_gemm_batched_frobenius_only_ms"], _ = event_ms(before, max(2, reps // 2), warmup=1)
    rec["frac_peak_rect_on_4n2T2"] = rec["flop_4n2T2"] / (rec["kernel_rect_ms"] * 1e-3) / PEAK_F64_MFMA
    rec["frac_peak_self_on_4n2T2"] = rec["flop_4n2T2"] / (rec["kernel_self_ms"] * 1e-3) / PEAK_F64_MFMA
    m, c = mean[:32].cpu().numpy(), cov[:32].cpu().numpy()
    t0 = time.perf_counter()
    for i in range(16):
        kl_ref.kl_pair(m[i], c[i], m[i + 16], c[i + 16], "inv")
    per_pair = (time.perf_counter() - t0) / 16
    rec["host_reference_formula_s_EXTRAPOLATED"] = per_pair * n * (n - 1) / 2
    rec["host_reference_formula_note"] = f"{per_pair * 1e3:.3f} ms per pair over 16 pairs, {torch.get_num_threads()} host threads, times n(n-1)/2"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_timing.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse HEAD)")
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None
        except OSError:
            commit = None
    res = {"commit": commit, "device": torch.cuda.get_device_name(0), "peak_f64_mfma": PEAK_F64_MFMA,
           "sizes": [one(2272, 90, a.reps), one(2048, 256, a.reps)]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
