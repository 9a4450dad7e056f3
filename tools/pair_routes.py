"""Every launch route of a pair-scoring call, once, at N = 8 segments and K = 2 clusters:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/pair_routes.py
    python tools/pair_routes.py --compare DIR_A DIR_B

Routes: T = 32 (mask-driven kernel alone); T = 90 with the prologue built in the kernel and streamed from the store, T = 200
(cooperative kernel), each rectangular and ragged; acc_tol = 0 (every cluster by the solve-based kernel); T = 90 with
HGP_PAIRS_GENERIC=1, in a child process of its own.  HGP_LIB selects the build, as everywhere.  The second form reads the
kernel traces of two such runs (one csv per process, taken in the order the processes started) and compares the sequences of
(kernel, grid, workgroup, LDS bytes) line for line; exit status 0 only when they are equal."""
import csv
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K = 8, 2


def routes(generic_only=False):
    import numpy as np
    import torch

    import synthetic_workload as synth
    from hdpgpc_amd import ops

    d = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda")  # noqa: E731
    for T, stores in ((90, (0,)),) if generic_only else ((32, (0,)), (90, (0, 1 << 30)), (200, (0,))):
        b = synth.synthetic_batch(N, K, T, seed=20260703)
        plan = ops.PairsPlan(T, T, b["theta"]).update(d(b["xb"]), d(b["mean"]), d(b["Sigma"]))
        x, y = d(b["x"]), d(b["y"])
        lens = np.array([T, 1, T - 1, T // 2, T, 17, T, T - 3], dtype=np.int32)
        for cap in stores:
            plan.SEGOPS_MAX_BYTES = cap
            for lengths in (None, lens):
                quad, _, info = plan.loglik(x, y, lengths=lengths)
                torch.cuda.synchronize()
                print(f"T={T} store={'yes' if cap else 'no'} ragged={lengths is not None} generic={generic_only}: "
                      f"checksum {float(quad.sum()):.12e} info {int(info.abs().max())}", flush=True)
        if T == 90 and not generic_only:
            plan.set_accuracy(0.0)
            plan.update(d(b["xb"]), d(b["mean"]), d(b["Sigma"]))
            quad, _, info = plan.loglik(x, y)
            torch.cuda.synchronize()
            print(f"T={T} acc_tol=0: checksum {float(quad.sum()):.12e} info {int(info.abs().max())}", flush=True)
        plan.close()


def launches(directory):
    """[(kernel, grid, workgroup, LDS bytes)] of every process's trace under directory, processes in the order they started"""
    per = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
        if rows:
            per.append((int(rows[0]["Start_Timestamp"]), rows))
    out = []
    for _, rows in sorted(per, key=lambda p: p[0]):
        for r in rows:
            out.append((r["Kernel_Name"], "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"),
                        "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"), r.get("LDS_Block_Size", r.get("Group_Segment_Size"))))
    return out


def compare(dir_a, dir_b):
    a, b = launches(dir_a), launches(dir_b)
    bad = [i for i in range(max(len(a), len(b))) if i >= len(a) or i >= len(b) or a[i] != b[i]]
    print(f"launches: {len(a)} in {dir_a}, {len(b)} in {dir_b}; lines that differ: {len(bad)}")
    for i in bad[:20]:
        print(f"  {i}: {a[i] if i < len(a) else None} | {b[i] if i < len(b) else None}")
    for i, l in enumerate(a):
        print(f"{i:4d} {' '.join(l[1:])} {l[0]}")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if sys.argv[1:2] == ["--generic"]:
        routes(generic_only=True)
    else:
        routes()
        subprocess.run([sys.executable, os.path.abspath(__file__), "--generic"], check=True, env=dict(os.environ, HGP_PAIRS_GENERIC="1"))
