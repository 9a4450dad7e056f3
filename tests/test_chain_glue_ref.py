"""CPU tier: pins tests/chain_glue_ref.py - the NumPy restatement the device tests of the member step's gather / finish kernels
compare with (tests/test_gpu_chain_glue.py) - to what the reference itself computed: the inputs and outputs of
matrix_normal_inv_wishart.posterior and the rows bayesian_new_params appended during a full_pass_weighted on the t30
configuration (tests/golden/chain_step_t30.npz, written by tests/golden/make_golden_chain.py).  No kernel runs here."""
import numpy as np
import pytest

import chain_glue_ref as cg
from conftest import golden

STEPS = (2, 3)          # N = 2: right covariances still the identity; N = 3: dense
# The header's scl = n0' / (n0' - 2) and ann = 1 / Nf'^2 are formed first and multiplied in; the reference forms
# (scale n0') / (n0' - 2) and Gamma[0] / N^2: two roundings each way on the leading term, one on the small one - a few ulp of the
# largest entry at most (seen: 1.9e-16).  The means follow the reference's own expression and come out equal.
ROW_TOL = 1e-15


def step_case(g, N, L=4, pos=1, seed=0):
    """(state before the step, inputs of the finish) from the recorded step N; what the reference does not hand to the MNIW
    updates (the covariances of the state, the rows of the stacks that the step does not read) is random."""
    p = f"s{N}_"
    T = g[p + "Gamma0"].shape[0]
    rng = np.random.default_rng(seed + N)
    st = {k: rng.normal(size=(L, T) if k in ("F", "Fsm") else (L, T, T)) for k in cg.STACKS}
    st["G"][0], st["S"][0] = g[p + "Gamma0"], g[p + "Sigma0"]
    d = [{k: g[f"{p}d{i}_{k}"] for k in ("old_m_mean", "old_m_r_cov", "old_scale", "old_n0", "y1", "y2", "S__", "part_mean",
                                         "jitter", "new_m_mean", "new_m_r_cov", "new_n0", "new_scale")} for i in range(2)]
    assert float(d[0]["old_n0"]) == float(d[1]["old_n0"])
    assert np.array_equal(d[1]["y2"], d[0]["y1"])             # the observation update's y2 is the new filtered mean
    st["W"] = np.stack([np.stack([d[0][k], d[1][k]]) for k in ("old_m_mean", "old_m_r_cov", "old_scale")])
    st.update(n0=float(d[0]["old_n0"]), Nf=float(g[p + "N"]) - 1.0, pos=pos, bad_count=np.zeros(2, dtype=np.int32))
    inputs = {"f_post": d[0]["y1"].reshape(-1), "f_sm_prev": d[0]["y2"].reshape(-1), "y": d[1]["y1"].reshape(-1),
              "c_post": rng.normal(size=(T, T)), "P_sm_prev": rng.normal(size=(T, T)),
              "part": np.stack([d[0]["part_mean"], d[1]["part_mean"]]), "Snew": np.stack([d[0]["S__"], d[1]["S__"]])}
    return st, inputs, d


def within(a, b, tol):
    return float(np.max(np.abs(a - b))) <= tol * float(np.max(np.abs(b)))


@pytest.mark.parametrize("N", STEPS)
def test_finish_ref_reproduces_the_reference_step(N):
    g = golden("chain_step_t30.npz")
    st, inputs, d = step_case(g, N)
    new = cg.finish_ref(st, inputs, [0, 0, 0, 0], [0, 0], cg.ANNEAL)
    pos = st["pos"]
    for i in range(2):
        assert np.array_equal(new["W"][2, i], d[i]["new_scale"])          # bit for bit
        assert np.array_equal(new["W"][1, i], d[i]["S__"]) and np.array_equal(d[i]["S__"], d[i]["new_m_r_cov"])
        assert within(new["W"][0, i], d[i]["new_m_mean"], ROW_TOL)
        print(f"N={N} d{i}: means off by {np.max(np.abs(new['W'][0, i] - d[i]['new_m_mean'])) / np.max(np.abs(d[i]['new_m_mean'])):.2e}")
    assert new["n0"] == float(d[0]["new_n0"]) == float(d[1]["new_n0"])
    assert new["Nf"] == float(g[f"s{N}_N"]) and new["pos"] == pos + 1 and new["bad_count"].tolist() == [0, 0]
    for key, name in (("A", "A_last"), ("G", "Gamma_last"), ("C", "C_last"), ("S", "Sigma_last")):
        ref = g[f"s{N}_{name}"]
        print(f"N={N} {name}: off by {np.max(np.abs(new[key][pos + 1] - ref)) / np.max(np.abs(ref)):.2e}")
        assert within(new[key][pos + 1], ref, ROW_TOL)
    # the state rows: appended, and the previous smoothed one rewritten; everything else as it was
    assert np.array_equal(new["P"][pos + 1], inputs["c_post"]) and np.array_equal(new["Psm"][pos + 1], inputs["c_post"])
    assert np.array_equal(new["F"][pos + 1], inputs["f_post"]) and np.array_equal(new["Fsm"][pos + 1], inputs["f_post"])
    assert np.array_equal(new["Psm"][pos], inputs["P_sm_prev"]) and np.array_equal(new["Fsm"][pos], inputs["f_sm_prev"])
    for k in cg.STACKS:
        rows = [r for r in range(st[k].shape[0]) if r != pos + 1 and not (r == pos and k in ("Psm", "Fsm"))]
        assert np.array_equal(new[k][rows], st[k][rows])


@pytest.mark.parametrize("N", STEPS)
def test_gather_ref_jitter_is_the_reference_s(N):
    """jitter = 1e-2 max(mean |diag scale|, eps) as GPI_model.py:1314 computed it on the same scale: the float64 mean of T
    non-negative terms is within T eps of the longdouble one."""
    g = golden("chain_step_t30.npz")
    st, _, d = step_case(g, N)
    T = st["W"].shape[-1]
    out, y_out, Rp, jit = cg.gather_ref(st, st["pos"], st["W"], None, -1)
    assert y_out is None and out.shape == (6 * T * T + 2 * T,)
    for i in range(2):
        ref = float(d[i]["jitter"])
        assert ref > 0 and abs(float(jit[i]) - ref) <= T * cg.EPS * ref
        off = ~np.eye(T, dtype=bool)
        assert np.array_equal(Rp[i][off].astype(np.float64), st["W"][1, i][off])
        assert np.allclose((np.diag(Rp[i]) - np.diag(st["W"][1, i]).astype(np.longdouble)).astype(np.float64), ref, rtol=1e-12, atol=0)
    o = 0
    for k in cg.STACKS:
        n = st[k][st["pos"]].size
        assert np.array_equal(out[o:o + n], st[k][st["pos"]].reshape(-1))
        o += n


@pytest.mark.parametrize("word,idx", [(0, 2), (0, 3), (1, 0), (1, 1)], ids=["info1[2]", "info1[3]", "info2[0]", "info2[1]"])
def test_finish_ref_keeps_the_distributions_of_a_failed_step(word, idx):
    g = golden("chain_step_t30.npz")
    st, inputs, d = step_case(g, 3)
    info1, info2 = [0, 0, 0, 0], [0, 0]
    (info1, info2)[word][idx] = 7
    new = cg.finish_ref(st, inputs, info1, info2, cg.ANNEAL)
    pos, n0, Nf1 = st["pos"], st["n0"], st["Nf"] + 1.0
    assert np.array_equal(new["W"], st["W"]) and new["n0"] == n0
    assert new["Nf"] == Nf1 and new["pos"] == pos + 1 and new["bad_count"].tolist() == [1, 0]
    assert np.array_equal(new["A"][pos + 1], st["W"][0, 0]) and np.array_equal(new["C"][pos + 1], st["W"][0, 1])
    ann = 1.0 / (Nf1 * Nf1)
    assert np.array_equal(new["G"][pos + 1], st["W"][2, 0] * (n0 / (n0 - 2.0)) + st["G"][0] * ann)
    assert np.array_equal(new["S"][pos + 1], st["W"][2, 1] * (n0 / (n0 - 2.0)) + st["S"][0] * ann)
    assert np.array_equal(new["P"][pos + 1], inputs["c_post"]) and np.array_equal(new["Fsm"][pos], inputs["f_sm_prev"])


def test_finish_ref_flags_and_latch():
    """Bit 1 (candidate step) writes rows only; bit 2 leaves the previous smoothed state; info1[0..1] latch bad_count[1] once and
    do not make the step bad."""
    g = golden("chain_step_t30.npz")
    st, inputs, _ = step_case(g, 2)
    full = cg.finish_ref(st, inputs, [0, 0, 0, 0], [0, 0], cg.ANNEAL)
    dry = cg.finish_ref(st, inputs, [0, 0, 0, 0], [0, 0], cg.ANNEAL | cg.DRY)
    assert np.array_equal(dry["W"], st["W"]) and (dry["n0"], dry["Nf"], dry["pos"]) == (st["n0"], st["Nf"], st["pos"])
    for k in cg.STACKS:
        assert np.array_equal(dry[k], full[k])
    keep = cg.finish_ref(st, inputs, [0, 0, 0, 0], [0, 0], cg.KEEP_PREV)
    pos = st["pos"]
    assert np.array_equal(keep["Psm"][pos], st["Psm"][pos]) and np.array_equal(keep["Fsm"][pos], st["Fsm"][pos])
    assert np.array_equal(keep["G"][pos + 1], full["W"][2, 0] * (full["n0"] / (full["n0"] - 2.0)) + st["G"][0] * 0.0)
    a = cg.finish_ref(st, inputs, [5, 0, 0, 0], [0, 0], 0)
    assert a["bad_count"].tolist() == [0, pos + 1] and np.array_equal(a["W"], cg.finish_ref(st, inputs, [0] * 4, [0, 0], 0)["W"])
    b = cg.finish_ref(a, inputs, [0, 3, 0, 1], [0, 0], 0)
    assert b["bad_count"].tolist() == [1, pos + 1] and b["pos"] == pos + 2 and b["n0"] == a["n0"]
