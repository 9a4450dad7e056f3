"""python tools/time_plan_update.py [from the repository root; HGP_LIB selects another build]: us per PairsPlan.update(): none flagged (ell 1.2) and all flagged (ell 3.0), K = 8, T = 128 and T = 90."""
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
import plan_ops_case as pc
from hdpgpc_amd import ops
dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda:0")
for T in (128, 90):
    for ell in (1.2, 3.0):
        K = 8
        theta = np.array([[1.0, ell, 0.125]] * K)
        Sg = dev(pc.make_sigma(T, K, 5, iso=None)); xb = dev(np.arange(T, dtype=np.float64)); mean = dev(np.zeros((K, T)) + 0.25)
        plan = ops.PairsPlan(T, T, theta, device="cuda:0")
        for _ in range(20): plan.update(xb, mean, Sg)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200): plan.update(xb, mean, Sg)
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 200 * 1e3)
        print(f"T={T} ell={ell} flagged={int(plan.solve_based().sum())}/{K}  update {best:.1f} us (back-to-back, best of 5)", flush=True)
