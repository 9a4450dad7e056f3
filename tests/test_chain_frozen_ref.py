"""CPU tier: pins tests/chain_frozen_ref.py - the NumPy restatement of the finish kernel with bit 3 (parameters frozen) that
tests/test_gpu_chain_frozen.py compares the kernel with - to what the reference itself did at and behind a cluster's estimation
limit: the lists and distributions before and after include_weighted_sample + backwards_pair + bayesian_new_params at N' = E
and N' = E + 1 on the t30 configuration (tests/golden/chain_step_estlimit_t30.npz, make_golden_estlimit.py).  No kernel runs."""
import numpy as np
import pytest

import chain_frozen_ref as fz
import chain_glue_ref as cg
from conftest import golden

LISTS = {"A": "A", "G": "Gamma", "C": "C", "S": "Sigma", "Psm": "cov_f_sm", "P": "cov_f", "F": "f_star", "Fsm": "f_star_sm"}


def step_case(g, Np, room=2):
    """(state before the step as a chain holds it, inputs of the finish, E) of the recorded step N' = Np.  The parameter rows
    behind the lists' end hold the last parameters; part and Snew are NaN and both status words of the MNIW updates are set:
    a frozen finish must not look at them."""
    p = f"s{Np}_pre_"
    E = int(g["estimation_limit"])
    T = g[p + "A"].shape[1]
    L = g[p + "f_star"].shape[0]
    rng = np.random.default_rng(Np)
    st = {}
    for k, name in LISTS.items():
        rows = g[p + name].reshape((-1, T) if k in ("F", "Fsm") else (-1, T, T))
        buf = rng.normal(size=(L + room,) + rows.shape[1:])
        buf[:rows.shape[0]] = rows
        buf[rows.shape[0]:L] = rows[-1]
        st[k] = buf
    st["W"] = np.stack([np.stack([g[f"{p}d0_{k}"], g[f"{p}d1_{k}"]]) for k in ("m_mean", "m_r_cov", "scale")])
    assert float(g[p + "d0_n0"]) == float(g[p + "d1_n0"])
    st.update(n0=float(g[p + "d0_n0"]), Nf=float(Np - 1), pos=L - 1, bad_count=np.array([3, 0], dtype=np.int32))
    q = f"s{Np}_post_"
    inputs = {"f_post": g[q + "f_star"][-1].reshape(-1), "c_post": g[q + "cov_f"][-1], "f_sm_prev": g[q + "f_star_sm"][-2].reshape(-1),
              "P_sm_prev": g[q + "cov_f_sm"][-2], "y": g[f"s{Np}_y"], "part": np.full((2, T, T), np.nan), "Snew": np.full((2, T, T), np.nan)}
    return st, inputs, E


@pytest.mark.parametrize("offset", [0, 1], ids=["at_the_limit", "behind_the_limit"])
def test_frozen_finish_reproduces_the_reference_step(offset):
    g = golden("chain_step_estlimit_t30.npz")
    Np = int(g["estimation_limit"]) + offset
    st, inputs, E = step_case(g, Np)
    new = fz.finish_ref(st, inputs, [0, 0, 5, 5], [7, 7], cg.ANNEAL | fz.FROZEN)
    pos, q, T = st["pos"], f"s{Np}_post_", st["W"].shape[-1]
    # the parameter lists do not grow: the model's lists are the first E rows, unchanged; the row behind holds the last ones
    for k in fz.PARAMS:
        assert g[q + LISTS[k]].shape[0] == E == g[f"s{Np}_pre_" + LISTS[k]].shape[0]
        assert np.array_equal(new[k][:E], g[q + LISTS[k]]) and np.array_equal(new[k][:pos + 1], st[k][:pos + 1])
        assert np.array_equal(new[k][pos + 1], g[q + LISTS[k]][-1])
        assert np.array_equal(new[k][pos + 2:], st[k][pos + 2:])
    # both distributions unchanged (the reference's own objects did not change either: asserted by the generator)
    assert np.array_equal(new["W"], st["W"]) and new["n0"] == st["n0"] == float(g[q + "d0_n0"])
    for d in range(2):
        for i, k in enumerate(("m_mean", "m_r_cov", "scale")):
            assert np.array_equal(new["W"][i, d], g[f"{q}d{d}_{k}"])
    assert new["bad_count"].tolist() == [3, 0] and new["Nf"] == float(Np) and new["pos"] == pos + 1
    # the state rows are the reference's lists after the step, bit for bit
    for k in ("Psm", "P", "F", "Fsm"):
        ref = g[q + LISTS[k]].reshape((-1, T) if k in ("F", "Fsm") else (-1, T, T))
        assert ref.shape[0] == pos + 2
        assert np.array_equal(new[k][:pos + 2], ref), k
        assert np.array_equal(new[k][pos + 2:], st[k][pos + 2:])


def test_frozen_flags_and_latch():
    """Bit 1: rows only (the parameter rows are still copied forward); bit 2: the previous smoothed state stays; info1[0..1]
    latch bad_count[1]; without bit 3 it is chain_glue_ref.finish_ref."""
    g = golden("chain_step_estlimit_t30.npz")
    st, inputs, E = step_case(g, int(g["estimation_limit"]) + 1)
    pos = st["pos"]
    full = fz.finish_ref(st, inputs, [0] * 4, [0, 0], fz.FROZEN)
    dry = fz.finish_ref(st, inputs, [0] * 4, [0, 0], fz.FROZEN | cg.DRY)
    assert (dry["Nf"], dry["pos"], dry["n0"]) == (st["Nf"], st["pos"], st["n0"])
    for k in cg.STACKS:
        assert np.array_equal(dry[k], full[k])
    keep = fz.finish_ref(st, inputs, [0] * 4, [0, 0], fz.FROZEN | cg.KEEP_PREV)
    assert np.array_equal(keep["Psm"][pos], st["Psm"][pos]) and np.array_equal(keep["Fsm"][pos], st["Fsm"][pos])
    assert np.array_equal(keep["P"][pos + 1], inputs["c_post"])
    lat = fz.finish_ref(st, inputs, [0, 2, 0, 0], [0, 0], fz.FROZEN | cg.DRY | cg.KEEP_PREV | cg.ANNEAL)
    assert lat["bad_count"].tolist() == [3, pos + 1]
    ok = dict(inputs, part=np.zeros_like(inputs["part"]), Snew=np.ones_like(inputs["Snew"]))
    a, b = fz.finish_ref(st, ok, [0] * 4, [0, 0], cg.ANNEAL), cg.finish_ref(st, ok, [0] * 4, [0, 0], cg.ANNEAL)
    assert all(np.array_equal(a[k], b[k]) for k in cg.STACKS + ("W",)) and a["n0"] == b["n0"] == st["n0"] + 1.0
