"""Record the plan-update operators (M', a', scal, acc_list, packed solve-based operands) and the pair scores of the seeded
cases of tests/plan_ops_case.py as tests/golden/plan_ops_t<T>.npz.

Run once on the GPU with the build whose results are the yardstick (the commit BEFORE a change to the plan update):

    python tests/golden/make_golden_plan_ops.py [outdir]

tests/test_gpu_plan_ops.py then asks the current build for the same bits."""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # repository root

import plan_ops_case as pc  # noqa: E402
from hdpgpc_amd import ops  # noqa: E402


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def main(outdir):
    os.makedirs(outdir, exist_ok=True)
    dev = lambda a: torch.as_tensor(a, dtype=torch.float64, device="cuda:0")  # noqa: E731
    for T in pc.WAVE_T + (pc.COOP_T,):
        case = pc.make_case(T)
        plan = ops.PairsPlan(T, T, case["theta"], device="cuda:0")
        plan.update(dev(case["xb"]), dev(case["mean"]), dev(case["Sigma"]))
        rec = pc.record(plan, case)
        K = case["K"]
        want = np.zeros(K)
        want[K - 1] = 1.0
        assert np.array_equal(rec["scal"][:, 7], want), ("routing of the seeded clusters", T, rec["scal"])
        assert rec["scal"][0, 3] == 1.0 and not rec["scal"][1:, 3].any(), ("iso flags", T)
        assert int(plan.info.abs().max()) == 0
        quad, logdet, info = plan.loglik(dev(case["x"]), dev(case["y"]))
        torch.cuda.synchronize()
        out = {k: rec[k] for k in ("Mp", "ap", "scal", "acc_list")}
        for name in pc.PACKED:           # sha-256 of the flagged cluster's packed operands; the arrays themselves at one size
            out["sha_" + name] = digest(rec[name])
            if T == 50:
                out[name] = rec[name]
        out.update(quad=quad.cpu().numpy(), logdet=logdet.cpu().numpy(), info=info.cpu().numpy())
        assert np.isfinite(out["quad"]).all() and np.isfinite(out["Mp"]).all()
        path = os.path.join(outdir, f"plan_ops_t{T}.npz")
        np.savez_compressed(path, **out)
        print(T, os.path.getsize(path), "bytes; info max", int(np.abs(out["info"]).max()), "bound",
              2.220446049250313e-16 * (rec["scal"][:, 0] * rec["scal"][:, 6]) ** 2)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)
