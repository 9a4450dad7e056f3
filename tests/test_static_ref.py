"""The NumPy restatement of the static filter chain (tests/static_ref.py, written from include/hdpgpc_hip_static.h) against the
reference's own recorded run (tests/golden/chain_static_t30.npz, written by tests/golden/make_golden_static.py): a static GPI_model
after full_pass_weighted over 12 beats of record 102 at T = 30.  Gate 1e-12 relative to each list's largest entry, the gate
tests/test_project_host.py holds a restatement to against recorded reference output.

Observed when the fixture was written: worst 7.1e-15 (means), 9.2e-16 (covariances)."""
import numpy as np

import static_ref
from conftest import golden


def replay(g, max_steps=1 << 20, calls=1):
    c, ell, noise = (float(v) for v in g["theta"])
    n, T = g["y"].shape
    Fs, Ps = np.zeros((n + 1, T)), np.zeros((n + 1, T, T))
    Fs[0], Ps[0] = g["f_star"][0], g["cov_f"][0]
    ch = static_ref.Chain(g["A0"], g["C0"], g["Sigma0"], Fs, Ps, 0, g["y"], g["indexes"], first=True, white=(c + noise) - c)
    for _ in range(calls):
        ch.steps(max_steps)
    return ch


def test_fixture_is_a_static_chain_from_the_kernel_gram():
    g = golden("chain_static_t30.npz")
    c, ell, noise = (float(v) for v in g["theta"])
    x = g["x_basis"] / ell
    gram = c * np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2)
    assert static_ref.rel_err(g["cov_f"][0], gram) <= 1e-14            # the prior covariance is the Gram itself: first-step branch
    assert not g["Gamma0"].any() and not g["q_lat"].any()
    assert np.array_equal(g["A0"], np.eye(len(x))) and np.array_equal(g["C0"], np.eye(len(x)))
    assert np.array_equal(g["f_star"], g["f_star_sm"]) and np.array_equal(g["cov_f"], g["cov_f_sm"])   # the same tensors in both lists
    assert len(g["f_star"]) == len(g["indexes"]) + 1 == 13


def test_restatement_reproduces_the_recorded_lists():
    g = golden("chain_static_t30.npz")
    ch = replay(g)
    assert ch.info == 0 and ch.pos == 12
    e_mean = max(static_ref.rel_err(ch.Fs[r], g["f_star"][r]) for r in range(1, 13))
    e_cov = max(static_ref.rel_err(ch.Ps[r], g["cov_f"][r]) for r in range(1, 13))
    print(f"restatement vs recorded reference: means {e_mean:.3e}, covariances {e_cov:.3e}")
    assert e_mean <= 1e-12 and e_cov <= 1e-12
    assert static_ref.rel_err(ch.Fs, g["f_star_sm"]) <= 1e-12 and static_ref.rel_err(ch.Ps, g["cov_f_sm"]) <= 1e-12


def test_restatement_is_resumable_and_reports_a_bad_pivot():
    g = golden("chain_static_t30.npz")
    one, parts = replay(g), replay(g, max_steps=5, calls=3)
    assert parts.pos == one.pos == 12 and np.array_equal(one.Fs, parts.Fs) and np.array_equal(one.Ps, parts.Ps)
    short = replay(g, max_steps=5)
    assert short.pos == 5 and np.array_equal(short.Fs[:6], one.Fs[:6]) and not short.Ps[6:].any()
    bad = {k: g[k] for k in g.files}
    bad["Sigma0"] = g["Sigma0"].copy()
    bad["Sigma0"][4, 4] = -1e9
    ch = replay(bad, max_steps=3)              # the first member uses white I, the second Sigma: fails at member 1
    assert ch.info == 5 and ch.pos == 12 and np.isnan(ch.Fs[2:]).all() and np.isnan(ch.Ps[2:]).all()
    assert np.array_equal(ch.Fs[1], one.Fs[1])
    before = (ch.Fs.copy(), ch.Ps.copy())
    ch.steps(3)                                # a chain that has ended is left alone
    assert np.array_equal(ch.Fs, before[0], equal_nan=True) and np.array_equal(ch.Ps, before[1], equal_nan=True)
