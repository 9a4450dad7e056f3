"""The plan update keeps, per cluster, the operators that depend on the basis grid and on the jitter 1e-4 mean|diag Sigma_k|
alone (K~, Z = chol(K~)^-1, K~^-1) for as long as both keep their bits, and the device decides that from the data.

Every comparison is bitwise (integer views, so NaN patterns compare too), and the reference is always a freshly created plan
that has seen only the final inputs: M', a', the scalars block with ||K~^-1||_inf and the routing flag, acc_list, the packed
operands of the flagged cluster, the plan's info, and the loglik outputs.  The `same` words of the plan (PlanReuse in
hgp_internal.hpp: what k_prep_build decided in the last call) are read as well, so that a test which is meant to run the
reuse path - or the recomputing one - fails if the other one ran: a -0.0 for a 0.0 changes no operator, only the decision.

Sizes: T = 32 (NB = 2), T = 90 (NB = 6, padded basis), T = 128 with K = 2; K = 3 with two length-scale groups at 32 and 90.
The last cluster of every case has length-scale 3 and is flagged for the solve-based kernel."""
import numpy as np
import pytest

import plan_ops_case as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [(32, 3), (90, 3), (128, 2)]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda:0")


def _case(T, K):
    """plan_ops_case's inputs; K = 2 keeps the ordinary cluster and the flagged one (both non-isotropic)."""
    c = pc.make_case(T)
    if K < c["K"]:
        keep = slice(c["K"] - K, c["K"])
        for name in ("theta", "mean", "Sigma", "Sigma_other"):
            c[name] = np.ascontiguousarray(c[name][keep])
        c["K"] = K
    rs = np.random.RandomState(77 + T)
    c["mean2"] = rs.randint(-256, 256, size=c["mean"].shape) / 256.0
    # the same diagonal, other off-diagonal entries: the jitter keeps its bits, P, Q, M' do not
    off = c["Sigma_other"].copy()
    for k in range(K):
        np.fill_diagonal(off[k], np.diag(c["Sigma"][k]))
    c["Sigma_offdiag"] = off
    return c


def _plan(case, acc_tol=1e-9):
    from hdpgpc_amd import ops

    return ops.PairsPlan(case["T"], case["T"], case["theta"], device="cuda:0", acc_tol=acc_tol)


def _same_words(plan, case):
    """[K] int32: k_prep_build's decision of the last update (1: cluster k kept its operators)."""
    K = case["K"]
    areas = pc.plan_areas(case["T"], K, plan._buf.numel())
    mat = areas["Mp"][1]
    q_off = areas["Mp"][0] - ((mat + 255) & ~255)
    off = q_off + K * 8 + K * 4   # behind key_jit [K] int64 and valid [K] int32
    torch.cuda.synchronize()
    return plan._buf[off:off + 4 * K].view(torch.int32).cpu().numpy().copy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _state(plan, case, score=True):
    rec = pc.record(plan, case)
    rec["plan_info"] = plan.info.cpu().numpy().copy()
    if score:
        quad, logdet, info = plan.loglik(_dev(case["x"]), _dev(case["y"]))
        torch.cuda.synchronize()
        rec["quad"], rec["logdet"], rec["info"] = quad.cpu().numpy(), logdet.cpu().numpy(), info.cpu().numpy()
    return rec


def _fresh(case, xb, mean, Sigma, acc_tol=1e-9, score=True):
    plan = _plan(case, acc_tol)
    plan.update(_dev(xb), _dev(mean), _dev(Sigma))
    rec = _state(plan, case, score)
    assert not _same_words(plan, case).any()   # the first update after plan_create computes everything
    plan.close()
    return rec


def _assert_equal(got, ref, what):
    assert got.keys() == ref.keys()
    for name in ref:
        assert got[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(_bits(got[name]), _bits(ref[name])), (what, name)


def _update_check(plan, case, xb, mean, Sigma, expect_same, what, acc_tol=1e-9, score=True):
    """update() with tensors of its own, then: the decision was the expected one and everything equals a fresh plan's."""
    plan.update(xb if torch.is_tensor(xb) else _dev(xb), _dev(mean), _dev(Sigma))
    same = _same_words(plan, case)
    assert np.array_equal(same != 0, np.broadcast_to(np.asarray(expect_same, dtype=bool), same.shape)), (what, same)
    xb_h = xb.cpu().numpy() if torch.is_tensor(xb) else xb
    _assert_equal(_state(plan, case, score), _fresh(case, xb_h, mean, Sigma, acc_tol, score), what)


@pytest.mark.parametrize("T,K", SIZES)
def test_same_basis_new_state(T, K):
    """The first update after plan_create computes; then the same grid three times with a new mean, new off-diagonal Sigma (the
    jitter keeps its bits: every cluster is kept) and a Sigma with another diagonal (another jitter: K~ itself changes, so
    nothing of it is kept), and the first state again."""
    c = _case(T, K)
    plan = _plan(c)
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], False, "first")
    _update_check(plan, c, c["xb"], c["mean2"], c["Sigma"], True, "new mean")
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma_offdiag"], True, "new off-diagonal Sigma")
    _update_check(plan, c, c["xb"], c["mean2"], c["Sigma_other"], False, "new diagonal of Sigma")
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], False, "first state again")
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], True, "and once more")


def test_one_cluster_changes_the_others_are_kept():
    """The online use: one cluster's Sigma moves, the others keep theirs - only that cluster is recomputed."""
    c = _case(90, 3)
    plan = _plan(c)
    plan.update(_dev(c["xb"]), _dev(c["mean"]), _dev(c["Sigma"]))
    Sig = c["Sigma"].copy()
    Sig[1] = c["Sigma_other"][1]
    _update_check(plan, c, c["xb"], c["mean2"], Sig, [True, False, True], "cluster 1 moved")
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], [True, False, True], "cluster 1 back")


@pytest.mark.parametrize("T,K", SIZES)
def test_basis_replaced_and_restored(T, K):
    c = _case(T, K)
    plan = _plan(c)
    plan.update(_dev(c["xb"]), _dev(c["mean"]), _dev(c["Sigma"]))
    xb2 = c["xb"] * 1.0625 + 0.25
    _update_check(plan, c, xb2, c["mean"], c["Sigma"], False, "other grid")
    _update_check(plan, c, xb2, c["mean2"], c["Sigma"], True, "other grid again")
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], False, "first grid back")


@pytest.mark.parametrize("T,K", SIZES)
def test_basis_modified_in_place(T, K):
    """The caller's tensor keeps its address: one entry moves by one ulp, then a 0.0 becomes -0.0.  Both are other grids."""
    c = _case(T, K)
    plan = _plan(c)
    xb = _dev(c["xb"])
    plan.update(xb, _dev(c["mean"]), _dev(c["Sigma"]))
    ptr = xb.data_ptr()
    xb[T // 2] = float(np.nextafter(c["xb"][T // 2], np.inf))
    _update_check(plan, c, xb, c["mean"], c["Sigma"], False, "one ulp")
    _update_check(plan, c, xb, c["mean"], c["Sigma"], True, "one ulp, again")
    assert float(xb[0]) == 0.0
    xb[0] = -0.0
    _update_check(plan, c, xb, c["mean"], c["Sigma"], False, "minus zero")
    assert xb.data_ptr() == ptr and bool(torch.signbit(xb[0]))


def test_new_plan_in_a_freed_plans_memory():
    """A plan created where an identical one was freed finds that plan's grid copy and operators in its buffer, and must not
    believe them: plan_create marks every cluster as not computed."""
    c = _case(32, 3)
    ref = _fresh(c, c["xb"], c["mean"], c["Sigma"])
    for _ in range(2):   # the second plan gets the first one's block from the caching allocator
        plan = _plan(c)
        _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], False, "first update")
        _assert_equal(_state(plan, c), ref, "reference")
        plan.close()
        del plan


def test_two_plans_alternate():
    c = _case(90, 3)
    xb2 = c["xb"] * 0.9375
    p1, p2 = _plan(c), _plan(c)
    for rnd, mean in enumerate((c["mean"], c["mean2"], c["mean"])):
        _update_check(p1, c, c["xb"], mean, c["Sigma"], rnd > 0, ("plan 1", rnd))
        _update_check(p2, c, xb2, mean, c["Sigma_other"], rnd > 0, ("plan 2", rnd))


@pytest.mark.parametrize("T,K", SIZES)
def test_flagged_cluster_on_the_reuse_path(T, K):
    """The length-scale 3 cluster is routed to the solve-based kernel: its flag, its packed operands (from the factor that
    k_acc_factor wrote over the kept K~ one call earlier) and its solve-based scores are those of a fresh plan; a cluster that
    becomes flagged while it is kept (set_accuracy) gets its factor from the kept K~."""
    c = _case(T, K)
    plan = _plan(c)
    plan.update(_dev(c["xb"]), _dev(c["mean"]), _dev(c["Sigma"]))
    assert plan.solve_based()[K - 1] and not plan.solve_based()[K - 2]
    _update_check(plan, c, c["xb"], c["mean2"], c["Sigma_offdiag"], True, "flagged, kept")
    assert plan.solve_based()[K - 1]
    plan.set_accuracy(-1.0)
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma"], True, "none flagged", acc_tol=-1.0)
    plan.set_accuracy(0.0)
    _update_check(plan, c, c["xb"], c["mean2"], c["Sigma"], True, "all flagged", acc_tol=0.0)
    assert plan.solve_based().all()
    plan.set_accuracy(1e-9)
    _update_check(plan, c, c["xb"], c["mean"], c["Sigma_offdiag"], True, "default routing")


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_basis(bad):
    """A grid with a non-finite entry equals itself bit for bit, so the second call keeps what the first one computed: info and
    every output of the update are a fresh plan's, whatever they are.  (The scoring kernels are not run on such a plan here:
    they read nothing of the plan but the outputs compared.)"""
    c = _case(90, 3)
    xb = c["xb"].copy()
    xb[17] = bad
    plan = _plan(c)
    _update_check(plan, c, xb, c["mean"], c["Sigma"], False, "first", score=False)
    _update_check(plan, c, xb, c["mean2"], c["Sigma"], True, "second", score=False)


def test_cooperative_size_repeated_update():
    """T = 192 keeps its chain, which has no reuse: a repeated update gives a fresh plan's operators."""
    from hdpgpc_amd import ops

    c = pc.make_case(192)
    plan = ops.PairsPlan(192, 192, c["theta"], device="cuda:0")
    for mean in (c["mean"], -c["mean"]):
        plan.update(_dev(c["xb"]), _dev(mean), _dev(c["Sigma"]))
        got = _state(plan, c)
        ref_plan = ops.PairsPlan(192, 192, c["theta"], device="cuda:0")
        ref_plan.update(_dev(c["xb"]), _dev(mean), _dev(c["Sigma"]))
        _assert_equal(got, _state(ref_plan, c), "T = 192")
        ref_plan.close()
