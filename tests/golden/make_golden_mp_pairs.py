"""40-digit truth of the pair scores and plan operators of tests/mp_pairs_case.py -> tests/golden/mp_pairs_t<T>.npz.

    python tests/golden/make_golden_mp_pairs.py [--out DIR] [T ...]      # CPU only, needs mpmath; about ten minutes for all sizes
    python tests/golden/make_golden_mp_pairs.py --bisect                 # prints the length-scales of clusters (b) and (c)

Each file holds the SHA-256 of the regenerated inputs, truth quad / logdet [N, K] with and without first_noise (rounded to
float64), ||K~^-1||_inf, kappa_inf(K~), bound and jitter per cluster, a' of every cluster and the upper triangle of M' of the
clusters the explicit-operator kernels score, (a) and (b): no kernel reads the M' of a routed cluster."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # repository root

import mp_pairs_case as mc  # noqa: E402


def bound64(case, k):
    """eps (c ||K~^-1||_inf)^2 in float64, for the bisection only."""
    from oracle import hdpgpc_oracle as orc

    c, ell, _ = case["theta"][k]
    T = case["T"]
    Kt = orc.gram_rbf(case["xb"], case["xb"], c, ell) + 1e-4 * np.mean(np.abs(np.diag(case["Sigma"][k]))) * np.eye(T)
    return np.finfo(np.float64).eps * (c * np.abs(np.linalg.inv(Kt)).sum(1).max()) ** 2


def bisect():
    for name, k, target in (("ELL_BELOW", 1, 0.35e-9), ("ELL_ABOVE", 2, 2.8e-9)):
        found = {}
        for T in mc.SIZES:
            lo, hi = 1.0, 3.0
            for _ in range(40):
                mid = 0.5 * (lo + hi)
                kw = {"ell_below": mid, "ell_above": mid}
                if bound64(mc.make_case(T, **kw), k) < target:
                    lo = mid
                else:
                    hi = mid
            found[T] = round(lo, 4)
        print(name, "=", found)


def generate(T, dps=None):
    """The arrays of one fixture file."""
    import mp_ref as mr

    dps = mr.DPS if dps is None else dps
    case = mc.make_case(T)
    Kc, N = case["K"], mc.N_FULL + mc.N_SHORT
    ops = [mr.cluster_ops(case["xb"], case["mean"][k], case["Sigma"][k], case["theta"][k], want_M=k in mc.EXPLICIT, dps=dps)
           for k in range(Kc)]
    out = {"sha_inputs": mc.digest(case)}
    for name in ("norm", "kappa", "bound", "jitter"):
        out[name] = np.array([float(o[name]) for o in ops])
    assert mc.WIN_BELOW[0] <= out["bound"][1] <= mc.WIN_BELOW[1], ("cluster (b) outside its window", T, out["bound"])
    assert mc.WIN_ABOVE[0] <= out["bound"][2] <= mc.WIN_ABOVE[1], ("cluster (c) outside its window", T, out["bound"])
    assert [o["iso"] for o in ops] == [False, False, False, True]
    out["ap"] = np.stack([mr.to_f64(o["ap"]).reshape(-1) for o in ops])
    iu = np.triu_indices(T)
    out["Mp_triu"] = np.stack([mr.to_f64(ops[k]["Mp"])[iu] for k in mc.EXPLICIT])
    quad, logdet, quad_f, logdet_f = (np.zeros((N, Kc)) for _ in range(4))
    for s, (xs, ys) in enumerate(case["sets"]):
        for i, n in enumerate(range(N)[mc.set_rows(s)]):
            for k in range(Kc):
                res = mr.pair(xs[i], ys[i], case["xb"], ops[k], (0.0, case["first"][n, k]), dps=dps)
                (quad[n, k], logdet[n, k]), (quad_f[n, k], logdet_f[n, k]) = [(float(q), float(ld)) for q, ld in res]
    out.update(quad=quad, logdet=logdet, quad_first=quad_f, logdet_first=logdet_f)
    return out


def main(argv):
    if "--bisect" in argv:
        return bisect()
    outdir = HERE
    if "--out" in argv:
        outdir = argv[argv.index("--out") + 1]
        argv = [a for a in argv if a not in ("--out", outdir)]
    os.makedirs(outdir, exist_ok=True)
    for T in [int(a) for a in argv] or mc.SIZES:
        path = os.path.join(outdir, f"mp_pairs_t{T}.npz")
        out = generate(T)
        np.savez_compressed(path, **out)
        print(T, os.path.getsize(path), "bytes; bound", out["bound"], "kappa", out["kappa"], flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
