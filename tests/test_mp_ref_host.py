"""Host tier of the 40-digit pair fixtures (tests/golden/mp_pairs_t*.npz, tests/mp_ref.py): the fixtures are what the generator
gives, the 40 digits are enough, clusters (b) and (c) sit where they were meant to, and every gate that
tests/test_gpu_pairs_truth.py holds the kernels to is met by a plain NumPy float64 restatement of the two evaluations - the
explicit operator as Z = L^-1, Z^T Z, M', E^T M' E, the solve-based one as the oracle - so no gate is tight by construction.

    python tests/test_mp_ref_host.py        # the NumPy ratios of every size, as kept in profiles/mp_truth_cpu.txt"""
import os
import sys

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE), os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mp_pairs_case as mc  # noqa: E402
from oracle import hdpgpc_oracle as orc  # noqa: E402


def _gold(T):
    return np.load(os.path.join(HERE, "golden", f"mp_pairs_t{T}.npz"))


def explicit_numpy(case, first):
    """The explicit-operator evaluation in float64 -> quad, logdet [N, K] and the per-cluster jitter, ||K~^-1||_inf, a', M'."""
    T, K = case["T"], case["K"]
    N = mc.N_FULL + mc.N_SHORT
    quad, logdet = np.zeros((N, K)), np.zeros((N, K))
    ops = []
    for k in range(K):
        c, ell, noise = case["theta"][k]
        Sigma = case["Sigma"][k]
        dS = np.diag(Sigma)
        mS = float(np.mean(dS))
        iso = bool(np.all(np.abs(dS - mS) <= 1e-8 + 1e-5 * abs(mS)))
        jit = 1e-4 * float(np.mean(np.abs(dS)))
        L = cholesky(orc.gram_rbf(case["xb"], case["xb"], c, ell) + jit * np.eye(T), lower=True)
        Z = solve_triangular(L, np.eye(T), lower=True)
        Kinv = Z.T @ Z
        Q = Kinv @ (0.5 * (Sigma + Sigma.T)) @ Kinv
        Mp = c * c * (0.5 * (Q + Q.T) - 0.5 * (Kinv + Kinv.T))
        ap = c * (Kinv @ case["mean"][k])
        ops.append(dict(jitter=jit, norm=np.abs(Kinv).sum(1).max(), ap=ap, Mp=Mp))
        for s, (xs, ys) in enumerate(case["sets"]):
            for i, n in enumerate(range(N)[mc.set_rows(s)]):
                m = xs.shape[1]
                E = orc.gram_rbf(case["xb"], xs[i], c, ell) / c
                if iso:
                    cov = mS * np.eye(m)
                else:
                    cov = orc.gram_rbf(xs[i], None, c, ell, noise) + E.T @ Mp @ E
                    cov = 0.5 * (cov + cov.T) + 1e-6 * np.eye(m)
                if first:
                    cov = cov + case["first"][n, k] * np.eye(m)
                quad[n, k], logdet[n, k] = orc.quad_logdet(ys[i] - E.T @ ap, cov)
    return quad, logdet, ops


def numpy_ratios(T):
    """name -> observed / allowed of every gate of the GPU tier, for the NumPy restatement at size T."""
    case, gold = mc.make_case(T), _gold(T)
    out = {}
    for first in (False, True):
        sfx = "_first" if first else ""
        q, ld, ops = explicit_numpy(case, first)
        refs = mc.oracle_errors(case, gold, first)
        for name, got, ref in (("quad", q, refs[0]), ("logdet", ld, refs[1])):
            err = mc.rel_each(got, gold[name + sfx])
            routed = np.where(np.arange(mc.K)[None, :] < 2, err, ref)          # default routing: (a), (b) explicit, (c), (d) oracle
            out[f"promise/{name}{sfx}"] = mc.gate_promise(routed)
            for k in mc.EXPLICIT:
                out[f"bound/{name}{sfx}/{'ab'[k]}"] = mc.gate_bound(err[:, k], ref[:, k], gold["bound"][k])
            for k in range(mc.K):
                out[f"solve/{name}{sfx}/{'abcd'[k]}"] = mc.gate_solve(ref[:, k], ref[:, k])
            # cluster (c) on the explicit path: above the floor term of the bound gate, below 10 x bound
            out[f"unrouted_c/{name}{sfx}/floor_over_err"] = 4.0 * max(float(ref[:, 2].max()), mc.EPS) / float(err[:, 2].max())
            out[f"unrouted_c/{name}{sfx}/err_over_10bound"] = float(err[:, 2].max()) / (10.0 * gold["bound"][2])
            out[f"observed/{name}{sfx}/err_over_bound_abc"] = [float(err[:, k].max() / gold["bound"][k]) for k in range(3)]
            out[f"observed/{name}{sfx}/err_ref_abcd"] = [float(ref[:, k].max()) for k in range(4)]
    for k in range(mc.K):
        tol = mc.gate_inverse(T, gold["kappa"][k])
        out[f"jitter/{'abcd'[k]}"] = abs(ops[k]["jitter"] - gold["jitter"][k]) / gold["jitter"][k] / (T * mc.EPS)
        out[f"norm/{'abcd'[k]}"] = abs(ops[k]["norm"] - gold["norm"][k]) / gold["norm"][k] / tol
        out[f"ap/{'abcd'[k]}"] = float(np.max(np.abs(ops[k]["ap"] - gold["ap"][k])) / np.max(np.abs(gold["ap"][k]))) / tol
    for i, k in enumerate(mc.EXPLICIT):
        Mt = mc.triu_to_full(T, gold["Mp_triu"][i])
        out[f"Mp/{'ab'[k]}"] = float(np.max(np.abs(ops[k]["Mp"] - Mt)) / np.max(np.abs(Mt))) / mc.gate_inverse(T, gold["kappa"][k])
    return out


def test_regenerating_t20_reproduces_the_fixture():
    pytest.importorskip("mpmath")
    import make_golden_mp_pairs as gen

    new, gold = gen.generate(20), _gold(20)
    assert sorted(new) == sorted(gold.files)
    for name in gold.files:
        assert new[name].dtype == gold[name].dtype and new[name].tobytes() == gold[name].tobytes(), name


def test_dps80_agrees_with_dps40():
    mp = pytest.importorskip("mpmath")
    import mp_ref as mr

    case = mc.make_case(20)
    worst = 0.0
    for k in range(mc.K):
        o40, o80 = (mr.cluster_ops(case["xb"], case["mean"][k], case["Sigma"][k], case["theta"][k], dps=d) for d in (40, 80))
        with mp.workdps(80):
            pairs = [(o40["norm"], o80["norm"]), (o40["bound"], o80["bound"])]
            for M40, M80 in ((o40["ap"], o80["ap"]), (o40["Mp"], o80["Mp"])):
                scale = max(abs(v) for v in M80)
                worst = max(worst, float(max(abs(a - b) for a, b in zip(M40, M80)) / scale))   # max-norm, as the operator gates
            for s, (xs, ys) in enumerate(case["sets"]):
                n = range(4)[mc.set_rows(s)][1]
                r40, r80 = (mr.pair(xs[1], ys[1], case["xb"], o, (0.0, case["first"][n, k] + 0.125), dps=d)
                            for o, d in ((o40, 40), (o80, 80)))
                pairs += [(a, b) for p40, p80 in zip(r40, r80) for a, b in zip(p40, p80)]
            worst = max([worst] + [mr.rel(a, b) for a, b in pairs])
    print(f"dps 40 against dps 80: {worst:.2e}")
    assert worst <= 1e-30


@pytest.mark.parametrize("T", mc.SIZES)
def test_truth_bounds_lie_in_their_windows(T):
    gold = _gold(T)
    assert np.array_equal(gold["sha_inputs"], mc.digest(mc.make_case(T)))
    assert mc.WIN_BELOW[0] <= gold["bound"][1] <= mc.WIN_BELOW[1]
    assert mc.WIN_ABOVE[0] <= gold["bound"][2] <= mc.WIN_ABOVE[1]
    assert gold["bound"][0] < 0.1 * mc.WIN_BELOW[0] and gold["bound"][3] > 10.0 * mc.WIN_ABOVE[1]
    assert gold["Mp_triu"].shape == (len(mc.EXPLICIT), T * (T + 1) // 2) and gold["ap"].shape == (mc.K, T)


def test_numpy_restatement_meets_every_gate():
    ratios = numpy_ratios(20)
    gates = {k: v for k, v in ratios.items() if not k.startswith("observed/")}
    for name, v in gates.items():
        print(f"{name:40s} {v:.3g}")
    assert all(v <= 1.0 for v in gates.values()), {k: v for k, v in gates.items() if not v <= 1.0}


if __name__ == "__main__":
    print("# NumPy float64 restatement against 40-digit truth: observed / allowed per gate of tests/test_gpu_pairs_truth.py")
    print("# (explicit path: Z = L^-1, Z^T Z, M', E^T M' E; solve-based path: the oracle itself, so its ratio is 1/8 by definition)")
    for T in mc.SIZES:
        for name, v in numpy_ratios(T).items():
            print(f"T={T:<4d} {name:44s} " + (" ".join(f"{x:.3g}" for x in v) if isinstance(v, list) else f"{v:.3g}"))
