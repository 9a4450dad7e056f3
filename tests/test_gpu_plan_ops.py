"""The plan update keeps its bits: M', a', scal, acc_list, the packed solve-based operands and the pair scores of the seeded
cases of plan_ops_case.py equal, bit for bit, what the library computed before the update's GEMM chain and k_prep_final were
folded into one launch (fixtures tests/golden/plan_ops_t*.npz, recorded by tests/golden/make_golden_plan_ops.py with that
earlier build).  The operation order per accumulator is unchanged and 0.5 x is exact, so no tolerance applies."""
import hashlib
import os

import numpy as np
import pytest

import plan_ops_case as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _dev(a):
    return torch.as_tensor(a, dtype=torch.float64, device="cuda:0")


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def _setup(T):
    from hdpgpc_amd import ops

    case = pc.make_case(T)
    gold = np.load(os.path.join(GOLD, f"plan_ops_t{T}.npz"))
    plan = ops.PairsPlan(T, T, case["theta"], device="cuda:0")
    return case, gold, plan


def _update(plan, case, sigma="Sigma"):
    plan.update(_dev(case["xb"]), _dev(case["mean"]), _dev(case[sigma]))
    return pc.record(plan, case)


def _check_operators(rec, gold, T):
    for name in ("Mp", "ap", "scal", "acc_list"):
        assert np.array_equal(rec[name], gold[name]), (T, name, _maxdiff(rec[name], gold[name]))
    for name in pc.PACKED:
        assert np.array_equal(_sha(rec[name]), gold["sha_" + name]), (T, name)
        if name in gold.files:
            assert np.array_equal(rec[name], gold[name]), (T, name, _maxdiff(rec[name], gold[name]))


def _maxdiff(a, b):
    if a.shape != b.shape:
        return (a.shape, b.shape)
    return float(np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64))))


def _check_scores(plan, case, gold, T):
    quad, logdet, info = plan.loglik(_dev(case["x"]), _dev(case["y"]))
    torch.cuda.synchronize()
    assert np.array_equal(quad.cpu().numpy(), gold["quad"]), (T, _maxdiff(quad.cpu().numpy(), gold["quad"]))
    assert np.array_equal(logdet.cpu().numpy(), gold["logdet"]), (T, _maxdiff(logdet.cpu().numpy(), gold["logdet"]))
    assert np.array_equal(info.cpu().numpy(), gold["info"]), T


def _counters(plan, case):
    """fb[0], fb[1 + PAIRS_FB_CAP] and the completion counter of the update (first word of the P area)."""
    areas = pc.plan_areas(case["T"], case["K"], plan._buf.numel())
    fb = pc.read_area(plan, areas, "fb", torch.int32)
    mat = areas["Mp"][1]
    p_off = areas["Mp"][0] - 2 * ((mat + 255) & ~255)
    done = plan._buf[p_off:p_off + 4].view(torch.int32).cpu().numpy()
    return int(fb[0]), int(fb[1 + pc.PAIRS_FB_CAP]), int(done[0])


@pytest.mark.parametrize("T", pc.WAVE_T)
def test_operators_and_scores_equal_fixture(T):
    case, gold, plan = _setup(T)
    _check_operators(_update(plan, case), gold, T)
    assert _counters(plan, case) == (0, 0, 0)
    _check_scores(plan, case, gold, T)


@pytest.mark.parametrize("T", pc.WAVE_T)
def test_second_update_is_rearmed(T):
    """Another Sigma on the same plan, then the first one again: a completion counter or a fall-back counter that was not
    re-armed would leave stale routing flags or stale operators."""
    case, gold, plan = _setup(T)
    first = _update(plan, case)
    other = _update(plan, case, "Sigma_other")
    assert not np.array_equal(other["Mp"], first["Mp"])
    assert other["scal"][0, 3] == 0.0          # no cluster is isotropic in the other state
    assert _counters(plan, case) == (0, 0, 0)
    _check_operators(_update(plan, case), gold, T)
    assert _counters(plan, case) == (0, 0, 0)
    _check_scores(plan, case, gold, T)


@pytest.mark.parametrize("T", pc.WAVE_T)
def test_set_accuracy_routes_all_then_none(T):
    case, gold, plan = _setup(T)
    K = case["K"]
    plan.set_accuracy(0.0)
    rec = _update(plan, case)
    assert np.array_equal(rec["scal"][:, 7], np.ones(K))
    assert np.array_equal(rec["acc_list"], np.array([K] + list(range(K))))
    assert np.array_equal(rec["Mp"], gold["Mp"]) and np.array_equal(rec["ap"], gold["ap"])
    plan.set_accuracy(-1.0)
    rec = _update(plan, case)
    assert np.array_equal(rec["scal"][:, 7], np.zeros(K))
    assert rec["acc_list"][0] == 0
    assert np.array_equal(rec["Mp"], gold["Mp"]) and np.array_equal(rec["ap"], gold["ap"])
    plan.set_accuracy(1e-9)                    # back to the default: the fixture's routing
    _check_operators(_update(plan, case), gold, T)


def test_cooperative_size_untouched():
    T = pc.COOP_T
    case, gold, plan = _setup(T)
    _check_operators(_update(plan, case), gold, T)
    _check_scores(plan, case, gold, T)
