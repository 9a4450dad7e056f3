"""The pair path (PairsPlan.update -> k_pairs / k_pairs_cooph / k_pairs_acc) against 40-digit truth, on both sides of the accuracy
threshold that routes a cluster from the explicit operator M' to the solve-based kernel.

Truth: tests/golden/mp_pairs_t<T>.npz (tests/golden/make_golden_mp_pairs.py, tests/mp_ref.py), for the seeded clusters and
segments of tests/mp_pairs_case.py: (a) ell = 1.2, (b) bound just below 1e-9, (c) just above, (d) iso Sigma at ell = 3.  "err" is
the relative error against truth; err_ref is the float64 oracle's error against truth for the same pairs, computed here, the
floor a float64 evaluation of the reference's operation order reaches.  The gates (mp_pairs_case.gate_*):
  promise   default routing: every quad and logdet within RT_PAIR = 1e-8
  bound     explicit clusters (a), (b): err <= truth bound + 4 max(err_ref of the cluster's pairs, eps)
  solve     solve-based clusters: err <= 8 max(err_ref of the cluster's pairs, 64 eps)
  operators jitter within T eps; ||K~^-1||_inf, a', M' within 8 T eps kappa_inf(K~) in max norm
tests/test_mp_ref_host.py holds a NumPy restatement to the same gates; observed ratios: profiles/mp_truth_observed.txt."""
import functools
import os

import numpy as np
import pytest

import mp_pairs_case as mc
import plan_ops_case as pc
from conftest import rel_err

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QUANT = ("quad", "logdet")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


@functools.lru_cache(maxsize=None)
def _ctx(T):
    """Case, fixture and err_ref = {first: (quad err, logdet err)} of size T, computed once and shared."""
    case = mc.make_case(T)
    gold = dict(np.load(os.path.join(GOLD, f"mp_pairs_t{T}.npz")))
    assert np.array_equal(gold["sha_inputs"], mc.digest(case))
    ref = {first: mc.oracle_errors(case, gold, first) for first in (False, True)}
    for v in gold.values():
        v.setflags(write=False)
    return case, gold, ref


def _plan(T, acc_tol=None):
    from hdpgpc_amd import ops

    case = _ctx(T)[0]
    plan = ops.PairsPlan(T, T, case["theta"], device="cuda:0")
    if acc_tol is not None:
        plan.set_accuracy(acc_tol)
    plan.update(_dev(case["xb"]), _dev(case["mean"]), _dev(case["Sigma"]))
    assert int(plan.info.abs().max()) == 0
    return plan


def _score(plan, case, first):
    """quad, logdet [N, K] of both segment sets (two calls: Ts = T and Ts = ceil(0.7 T))."""
    N = mc.N_FULL + mc.N_SHORT
    quad, logdet = np.zeros((N, mc.K)), np.zeros((N, mc.K))
    for s, (xs, ys) in enumerate(case["sets"]):
        r = mc.set_rows(s)
        q, ld, info = plan.loglik(_dev(xs), _dev(ys), first_noise=_dev(case["first"][r]) if first else None)
        assert int(info.abs().max()) == 0
        quad[r], logdet[r] = q.cpu().numpy(), ld.cpu().numpy()
    return quad, logdet


@functools.lru_cache(maxsize=None)
def _default_run(T):
    """Default routing: {first: (quad, logdet)}, scal, and the plan's a' and M' areas."""
    case = _ctx(T)[0]
    plan = _plan(T)
    rec = pc.record(plan, case)
    scores = {first: _score(plan, case, first) for first in (False, True)}
    return scores, rec


def _errs(T, scores):
    """{(quantity, first): (err [N, K], err_ref [N, K])}"""
    _, gold, ref = _ctx(T)
    out = {}
    for first in (False, True):
        for i, name in enumerate(QUANT):
            truth = gold[name + ("_first" if first else "")]
            rel_err(scores[first][i], truth)           # conftest keeps the worst value per test
            out[name, first] = (mc.rel_each(scores[first][i], truth), ref[first][i])
    return out


def _report(T, what, ratios):
    print(f"T={T} {what}: " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


@pytest.mark.parametrize("T", mc.SIZES)
def test_promise(T):
    ratios = {f"{n}{'_first' if f else ''}": mc.gate_promise(err) for (n, f), (err, _) in _errs(T, _default_run(T)[0]).items()}
    _report(T, "promise err/1e-8", ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("T", mc.SIZES)
def test_bound_is_a_bound(T):
    gold = _ctx(T)[1]
    ratios, plain = {}, {}
    for (n, f), (err, ref) in _errs(T, _default_run(T)[0]).items():
        for k in mc.EXPLICIT:
            key = f"{n}{'_first' if f else ''}/{'ab'[k]}"
            ratios[key] = mc.gate_bound(err[:, k], ref[:, k], gold["bound"][k])
            plain[key] = float(err[:, k].max() / gold["bound"][k])
    _report(T, "bound gate", ratios)
    _report(T, "err/bound", plain)
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("T", mc.SIZES)
def test_solve_based_path(T):
    case = _ctx(T)[0]
    ratios = {}
    for (n, f), (err, ref) in _errs(T, _default_run(T)[0]).items():     # (c), (d) as the default routing sends them
        for k in (2, 3):
            ratios[f"{n}{'_first' if f else ''}/default/{'abcd'[k]}"] = mc.gate_solve(err[:, k], ref[:, k])
    plan = _plan(T, acc_tol=0.0)
    assert plan.solve_based().all()
    forced = {first: _score(plan, case, first) for first in (False, True)}
    for (n, f), (err, ref) in _errs(T, forced).items():
        for k in range(mc.K):
            ratios[f"{n}{'_first' if f else ''}/forced/{'abcd'[k]}"] = mc.gate_solve(err[:, k], ref[:, k])
    _report(T, "solve gate", ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("T", mc.SIZES)
def test_routing(T):
    case, gold, _ = _ctx(T)
    scal = _default_run(T)[1]["scal"]
    assert list(scal[:, 7] != 0.0) == [False, False, True, True]
    assert list(scal[:, 3]) == [0.0, 0.0, 0.0, 1.0]
    jit = np.abs(scal[:, 5] - gold["jitter"]) / gold["jitter"] / (T * mc.EPS)
    nrm = np.abs(scal[:, 6] - gold["norm"]) / gold["norm"] / mc.gate_inverse(T, gold["kappa"])
    _report(T, "jitter / (T eps)", dict(zip("abcd", jit)))
    _report(T, "norm / (8 T eps kappa)", dict(zip("abcd", nrm)))
    assert (jit <= 1.0).all() and (nrm <= 1.0).all()
    # the explicit operator everywhere: cluster (c) is now worse than the floor its solve-based evaluation is held to, and the
    # bound still bounds
    plan = _plan(T, acc_tol=-1.0)
    assert not plan.solve_based().any()
    unrouted = {first: _score(plan, case, first) for first in (False, True)}
    over_floor, under = {}, {}
    for (n, f), (err, ref) in _errs(T, unrouted).items():
        key = f"{n}{'_first' if f else ''}"
        over_floor[key] = float(err[:, 2].max()) / (4.0 * max(float(ref[:, 2].max()), mc.EPS))
        under[key] = float(err[:, 2].max()) / (10.0 * gold["bound"][2])
    _report(T, "(c) explicit: err / floor", over_floor)
    _report(T, "(c) explicit: err / (10 bound)", under)
    assert all(v > 1.0 for v in over_floor.values()), over_floor
    assert all(v <= 1.0 for v in under.values()), under


def _mp_logical(T, Mp):
    """[K, TP, TP] as stored -> logical column order (plan_mp_col of hgp_plan.hip undone; T > 128 is row-major)."""
    if T > 128:
        return Mp
    TP = pc.tp_for(T)
    nh = (TP // 16) // 2
    col = []
    for j in range(TP):
        hh, tl, cc = j // (16 * nh), (j // 16) % nh, j % 16
        col.append(16 * nh * hh + (32 * (tl // 2) + 2 * cc + (tl & 1) if tl < 2 * (nh // 2) else 16 * (nh - 1) + cc))
    assert sorted(col) == list(range(TP))
    return Mp[:, :, col]


@pytest.mark.parametrize("T", mc.SIZES)
def test_operators(T):
    _, gold, _ = _ctx(T)
    rec = _default_run(T)[1]
    ratios = {}
    for k in range(mc.K):
        ap = rec["ap"][k]
        assert not ap[T:].any()
        ratios[f"ap/{'abcd'[k]}"] = (float(np.max(np.abs(ap[:T] - gold["ap"][k])) / np.max(np.abs(gold["ap"][k])))
                                     / mc.gate_inverse(T, gold["kappa"][k]))
    Mp = _mp_logical(T, rec["Mp"])
    for i, k in enumerate(mc.EXPLICIT):
        M = Mp[k]
        assert np.array_equal(M, M.T), ("M' is not exactly symmetric", T, k)
        assert not M[T:, :].any() and not M[:, T:].any(), ("M' padding is not zero", T, k)
        Mt = mc.triu_to_full(T, gold["Mp_triu"][i])
        ratios[f"Mp/{'ab'[k]}"] = float(np.max(np.abs(M[:T, :T] - Mt)) / np.max(np.abs(Mt))) / mc.gate_inverse(T, gold["kappa"][k])
    _report(T, "operators / (8 T eps kappa)", ratios)
    assert all(v <= 1.0 for v in ratios.values()), ratios
