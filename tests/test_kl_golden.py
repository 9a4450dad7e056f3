"""tests/kl_ref.py reproduces every value of tests/golden/kl_states.npz, which tests/golden/make_golden_kl.py recorded from
the reference's own GPI_model.KL_divergence (both `smoothed` flags, another grid, the plot_MDS matrix), to 1e-9 - the
tolerance of test_oracle_golden.py.  This pins the fixture the GPU tests compare with."""
import numpy as np

import conftest
import kl_ref

TOL = 1e-9


def _close(got, ref):
    err = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)))
    assert err <= TOL, err


def test_blocks():
    z = conftest.golden("kl_states.npz")
    for name, p1, p2, sm, xb, t1, t2 in kl_ref.golden_blocks(z):
        c1, c2 = kl_ref.cluster(z, p1), kl_ref.cluster(z, p2)
        t1 = range(len(c1["indexes"])) if t1 is None else t1
        t2 = range(len(c2["indexes"])) if t2 is None else t2
        ref = z[name]
        assert ref.shape == (len(t1), len(t2)) and np.all(np.isfinite(ref))
        for order in ("inv", "chol"):
            got = np.array([[kl_ref.kl_pair(*kl_ref.state_moments(c1, t, sm, xb), *kl_ref.state_moments(c2, u, sm, xb), order)
                             for u in t2] for t in t1])
            _close(got, ref)


def test_matrix_form_and_sensitivity():
    z = conftest.golden("kl_states.npz")
    assert 0.0 <= float(z["ref_sens"]) < 1e-10
    for p in ("L_", "H_"):
        c = kl_ref.cluster(z, p)
        n = len(c["indexes"])
        mom = [kl_ref.state_moments(c, t, False) for t in range(n)]
        got = kl_ref.kl_matrix(np.stack([m for m, _ in mom]), np.stack([0.5 * (s + s.T) for _, s in mom]))
        _close(got, z["kl_" + p[0] + p[0] + "_f"])


def test_plot_mds_matrix():
    z = conftest.golden("kl_states.npz")
    KL, n_seg = z["plot_mds"], int(z["n_seg"])
    assert KL.shape == (n_seg, n_seg) and np.array_equal(KL, KL.T) and np.all(np.diag(KL) == 0.0)
    L, S = kl_ref.cluster(z, "L_"), kl_ref.cluster(z, "S_")
    members = [(c, t, int(i)) for c in (L, S) for t, i in enumerate(c["indexes"])]
    used = {i for _, _, i in members}
    for s in range(n_seg):
        if s not in used:
            assert np.all(KL[s] == 0.0)
    for c1, t, i in members:
        for c2, u, j in members:
            if i < j:
                v = kl_ref.kl_pair(*kl_ref.state_moments(c1, t, False), *kl_ref.state_moments(c2, u, False))
                assert abs(v - KL[i, j]) <= TOL * max(abs(KL[i, j]), 1.0)
    # the blocks and the matrix hold the same numbers
    iL = L["indexes"]
    for a in range(len(iL)):
        for b in range(len(iL)):
            if iL[a] < iL[b]:
                assert KL[iL[a], iL[b]] == z["kl_LL_f"][a, b]


def test_late_states_nearly_identical():
    """What test_near_identical_states on the device relies on: for consecutive stored states of the long cluster the trace
    term is within 1 % of 2T, so that (trace - 2T) loses two to three digits."""
    z = conftest.golden("kl_states.npz")
    c = kl_ref.cluster(z, "L_")
    n, worst = len(c["indexes"]), 0.0
    assert int(z["L_offset"]) >= 30
    for sm in (False, True):
        for t in range(n - 1):
            (m1, c1), (m2, c2) = kl_ref.state_moments(c, t, sm), kl_ref.state_moments(c, t + 1, sm)
            tr = np.trace(np.linalg.inv(c2) @ c1 + np.linalg.inv(c1) @ c2)
            worst = max(worst, abs(tr / (2 * len(m1)) - 1.0))
    assert 0.0 < worst < 1e-2, worst
