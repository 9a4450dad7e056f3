"""Latency of ops.chol_inverse_rhs (the two inversions of the LDS member step) at small batches:
    python tools/time_inv_rhs.py [T] [plain|ws]
Prints us per call for b = 2, 4, 8, 20, 40, 80 and a checksum of the outputs.  With `plain` it times ops.chol_inverse(A, 0.0, 1e-8)
on the same matrices instead (T up to 256; checksum of Z and info); with `ws` the same call with a workspace, which for T > 128 and
b * NB > 512 factors once (k_coop_potrf) and takes L^-1 from L (k_trtri).  HGP_LIB selects another build."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from hdpgpc_amd import ops  # noqa: E402

T = int(sys.argv[1]) if len(sys.argv) > 1 else 90
mode = sys.argv[2] if len(sys.argv) > 2 else ""
plain = mode in ("plain", "ws")
rng = np.random.default_rng(7)
dev = "cuda"
for b in (2, 4, 8, 20, 40, 80):
    G = rng.standard_normal((b, T, T))
    A = torch.as_tensor(G @ G.transpose(0, 2, 1) / T + 0.5 * np.eye(T), device=dev)
    B = torch.as_tensor(rng.standard_normal((b, T, T)), device=dev)
    Z, Y = torch.zeros_like(A), torch.zeros_like(A)
    info = torch.zeros(b, dtype=torch.int32, device=dev)
    on = torch.tensor([1, 1, 0, 0] * (b // 4) + [1] * (b % 4), dtype=torch.int32, device=dev)
    W = torch.empty_like(A) if mode == "ws" else None
    if plain:
        call = lambda: ops.chol_inverse(A, 0.0, 1e-8, out=Z, info=info, work=W)  # noqa: E731
    else:
        call = lambda: ops.chol_inverse_rhs(A, Z, B, Y, info, rhs_on=on, add_diag=1e-8)  # noqa: E731
    for _ in range(5):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 200
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    keep = on.bool().cpu().numpy()
    solved = b"" if plain else Y.cpu().numpy()[keep].tobytes()
    h = hashlib.sha1(Z.cpu().numpy().tobytes() + solved + info.cpu().numpy().tobytes()).hexdigest()[:12]
    err = float(torch.linalg.norm(Z @ A @ Z.transpose(1, 2) - torch.eye(T, device=dev, dtype=torch.float64)) / np.sqrt(b * T))
    print(f"T={T} b={b:3d}{' ' + mode if plain else ''}: {1e3 * e0.elapsed_time(e1) / reps:7.2f} us per call (back to back)   sha1 {h}   |Z A Z^T - I| {err:.2e}  info {int(info.abs().max())}")
