"""a13 on the device: hgp_kl_sym_f64 through ops.kl_sym, the model layer on top of it and the plot_MDS drop-in.

Gates.  The sweep and the full-size test compare with tests/kl_ref.py at 50 x the difference between the restatement's two
evaluation orders for the same case (LU inverses in the reference's order against Cholesky inverses), floor 1e-12, both
relative to max(|value|, 1) - the 50 x sensitivity margin of tests/test_gpu_include_batch.py.  Position independence and
symmetry are bit-for-bit.  The parity tests compare with tests/golden/kl_states.npz, recorded from the reference's own
GPI_model.KL_divergence on MIT-BIH clusters, at |a - b| <= tol max(|b|, 1), tol = max(1e-9, 50 ref_sens).
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import conftest
import kl_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def spd_states(rng, n, T, cond=1e4, close=False):
    """n random Gaussians on T points: covariances Q diag(lambda) Q^T with condition numbers up to `cond`; means far apart,
    or (close) within 1e-4 of the norm of one common mean."""
    covs = np.empty((n, T, T))
    for i in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((T, T)))
        lam = np.logspace(0.0, np.log10(cond) * rng.uniform(0.2, 1.0), T) * rng.uniform(0.5, 2.0)
        c = (Q * lam) @ Q.T
        covs[i] = 0.5 * (c + c.T)
    if close:
        base = 5.0 * rng.standard_normal(T)
        means = base[None, :] + 1e-4 * np.linalg.norm(base) / np.sqrt(T) * rng.standard_normal((n, T))
    else:
        means = 5.0 * rng.standard_normal((n, T))
    return means, covs


def gate(ref_a, ref_b):
    scale = np.maximum(np.abs(ref_b), 1.0)
    return max(1e-12, 50.0 * float(np.max(np.abs(ref_a - ref_b) / scale)))


def check(got, ref_inv, ref_chol, what):
    tol = gate(ref_inv, ref_chol)
    err = float(np.max(np.abs(got - ref_chol) / np.maximum(np.abs(ref_chol), 1.0)))
    conftest._note(err)
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert np.all(np.isfinite(got))
    assert err <= tol, (what, err, tol)


SWEEP_T = [1, 8, 17, 45, 90, 128, 129, 200, 256]
SWEEP_N = [(1, None), (3, None), (70, None), (300, None), (1, 1), (3, 70), (70, 3), (300, 70), (1, 300)]


@pytest.mark.parametrize("T", SWEEP_T)
def test_sweep_against_kl_ref(T):
    from hdpgpc_amd import ops
    rng = np.random.default_rng(1000 + T)
    for nA, nB, close in [(a, b, c) for a, b in SWEEP_N for c in (False, True)]:
        mA, cA = spd_states(rng, nA, T, close=close)
        if nB is None:
            got = ops.kl_sym(dev(mA), dev(cA)).cpu().numpy()
            r_inv, r_chol = kl_ref.kl_matrix(mA, cA, order="inv"), kl_ref.kl_matrix(mA, cA, order="chol")
            assert np.array_equal(got, got.T)
        else:
            mB, cB = spd_states(rng, nB, T, close=close)
            if close:
                mB += mA[0] - mB[0] + 1e-5 * rng.standard_normal(T)     # the two sets around the same mean
            got = ops.kl_sym(dev(mA), dev(cA), dev(mB), dev(cB)).cpu().numpy()
            r_inv, r_chol = kl_ref.kl_matrix(mA, cA, mB, cB, order="inv"), kl_ref.kl_matrix(mA, cA, mB, cB, order="chol")
        assert got.shape == r_chol.shape
        check(got, r_inv, r_chol, f"T={T} nA={nA} nB={nB} close={close}")


def test_matches_reference_order_pairwise():
    """A handful of pairs against the reference's exact sequence of operations (kl_ref.kl_pair), T = 45 and 90."""
    from hdpgpc_amd import ops
    rng = np.random.default_rng(5)
    for T in (45, 90):
        m, c = spd_states(rng, 6, T, cond=1e3)
        got = ops.kl_sym(dev(m), dev(c)).cpu().numpy()
        r_inv = np.array([[kl_ref.kl_pair(m[i], c[i], m[j], c[j], "inv") for j in range(6)] for i in range(6)])
        r_chol = np.array([[kl_ref.kl_pair(m[i], c[i], m[j], c[j], "chol") for j in range(6)] for i in range(6)])
        check(got, r_inv, r_chol, f"pairwise T={T}")
        assert np.all(np.abs(np.diag(got)) <= 1e-12 * T)


def test_position_independence():
    """Entry (i, j) of the self call, of rectangular calls that hold the pair at other positions (and swapped) and of the
    1 x 1 call are the same bits; the self call is bitwise symmetric."""
    from hdpgpc_amd import ops
    rng = np.random.default_rng(7)
    for T, n in ((45, 300), (90, 140), (17, 270)):
        m, c = spd_states(rng, n, T, cond=1e3, close=(T == 90))
        M, C = dev(m), dev(c)
        D = ops.kl_sym(M, C)
        assert torch.equal(D, D.T)
        lo, hi = n // 3, n - 5
        R = ops.kl_sym(M[lo:].contiguous(), C[lo:].contiguous(), M[:hi].contiguous(), C[:hi].contiguous())
        assert torch.equal(R, D[lo:, :hi])
        Rt = ops.kl_sym(M[:hi].contiguous(), C[:hi].contiguous(), M[lo:].contiguous(), C[lo:].contiguous())
        assert torch.equal(Rt, D[:hi, lo:])
        for i, j in ((0, 1), (3, n - 1), (n - 1, 129 % n), (n // 2, n // 2), (130 % n, 2)):
            one = ops.kl_sym(M[i:i + 1].contiguous(), C[i:i + 1].contiguous(), M[j:j + 1].contiguous(), C[j:j + 1].contiguous())
            assert one[0, 0].item() == D[i, j].item(), (T, i, j)


def _model(rng, T, n_members, indexes, dynamic=True, estimation_limit=None):
    """A GPI_model with a synthetic state of n_members steps (stacks of n_members + 1 rows, as the recursion leaves them)."""
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    S = n_members + 1
    f, P = spd_states(rng, S, T, cond=50.0)
    fsm, Psm = spd_states(rng, S, T, cond=50.0)
    _, Sig = spd_states(rng, S, T, cond=20.0)
    C = np.eye(T)[None] + 0.1 * rng.standard_normal((S, T, T))
    A = np.tile(np.eye(T), (S, 1, 1))
    _, G = spd_states(rng, S, T, cond=5.0)
    if not dynamic:
        G[-1] = 0.0
    gm = GPI_model(RBFWhiteKernel(300.0, 1.2, 4.0, device=DEV), np.arange(float(T)), estimation_limit=estimation_limit)
    gm.load_state(f, Sig, C, indexes, f_star_sm=fsm, cov_f_sm=Psm, A=A, Gamma=G, cov_f=P)
    host = dict(f=f, P=P, fsm=fsm, Psm=Psm, Sig=Sig, C=C)
    return gm, host


def _observed(host, t, smoothed, tc=None):
    tc = t if tc is None else tc
    f, P = (host["fsm"], host["Psm"]) if smoothed else (host["f"], host["P"])
    C, S = host["C"][tc], host["Sig"][tc]
    return C @ f[t + 1], C @ P[t + 1] @ C.T + S


def test_model_layer():
    """GPI_model.KL_divergence reads f_star[t+1] / cov_f[t+1] with C[t] / Sigma[t], clamps at estimation_limit, is the 1 x 1
    case of kl_states bit for bit, and compares latent states when Gamma[-1] is all zero."""
    rng = np.random.default_rng(11)
    T = 17
    g1, h1 = _model(rng, T, 6, [0, 2, 3, 5, 8, 9])
    g2, h2 = _model(rng, T, 4, [1, 4, 6, 7], estimation_limit=2)
    for smoothed in (False, True):
        D = g1.kl_states(range(6), g2, range(4), smoothed=smoothed)
        for t in range(6):
            for u in range(4):
                v = g1.KL_divergence(t, g2, u, smoothed=smoothed)
                assert v == D[t, u].item()
                ref = kl_ref.kl_pair(*_observed(h1, t, smoothed), *_observed(h2, u, smoothed, tc=(-1 if u >= 2 else u)), "inv")
                assert abs(v - ref) <= 1e-9 * max(abs(ref), 1.0), (t, u, v, ref)
        mo, co = g1.observed_moments(range(6), smoothed=smoothed)
        assert mo.shape == (6, T) and co.shape == (6, T, T) and torch.equal(co, co.transpose(1, 2))
        S = g1.kl_states(range(6), smoothed=smoothed)
        assert torch.equal(S, S.T)
    # x_bas equal to the basis is the same route
    assert g1.KL_divergence(1, g2, 1, smoothed=False, x_bas=np.arange(float(T))) == g1.KL_divergence(1, g2, 1, smoothed=False)
    # static branch
    s1, hs1 = _model(rng, T, 3, [0, 1, 2], dynamic=False)
    v = s1.KL_divergence(0, g1, 2, smoothed=True)
    ref = kl_ref.kl_pair(hs1["fsm"][1], hs1["Psm"][1], h1["fsm"][3], h1["Psm"][3], "inv")
    assert abs(v - ref) <= 1e-9 * max(abs(ref), 1.0)
    # GPI level
    m, c = spd_states(rng, 2, T)
    v = g1.gp.KL_divergence(m[0], c[0], m[1], c[1])
    assert isinstance(v, float) and abs(v - kl_ref.kl_pair(m[0], c[0], m[1], c[1])) <= 1e-9 * max(abs(v), 1.0)


def test_edges():
    from hdpgpc_amd import ops
    rng = np.random.default_rng(13)
    m, c = spd_states(rng, 3, 8)
    assert tuple(ops.kl_sym(dev(m[:0]), dev(c[:0])).shape) == (0, 0)
    assert tuple(ops.kl_sym(dev(m[:0]), dev(c[:0]), dev(m), dev(c)).shape) == (0, 3)
    assert tuple(ops.kl_sym(dev(m), dev(c), dev(m[:0]), dev(c[:0])).shape) == (3, 0)
    bad = c.copy()
    bad[1] = -bad[1]
    with pytest.raises(torch.linalg.LinAlgError):
        ops.kl_sym(dev(m), dev(bad))
    with pytest.raises(torch.linalg.LinAlgError):
        ops.kl_sym(dev(m), dev(c), dev(m), dev(bad))
    big = np.tile(np.eye(257), (2, 1, 1))
    with pytest.raises(NotImplementedError):
        ops.kl_sym(dev(np.zeros((2, 257))), dev(big))


def test_distance_matrix_dropin(capsys):
    """kl_distance_matrix places every pair of member states at their segment indices (util_plots.py:606-616)."""
    import hdpgpc.util_plots as up
    from hdpgpc_amd import util_plots as upa
    rng = np.random.default_rng(17)
    T, n_seg = 8, 14
    g1, h1 = _model(rng, T, 5, [0, 3, 4, 9, 12])
    g2, h2 = _model(rng, T, 4, [1, 5, 6, 11])
    g3, _ = _model(rng, T, 0, [])
    sw = types.SimpleNamespace(T=n_seg, M=3, gpmodels=[[g1, g2, g3]], x_basis=[np.arange(float(T))],
                               cond_to_torch=lambda x: torch.as_tensor(x, dtype=torch.float64, device=DEV))
    KL = upa.kl_distance_matrix(sw)
    assert KL.shape == (n_seg, n_seg) and KL.dtype == np.float64
    assert np.array_equal(KL, KL.T) and np.all(np.diag(KL) == 0.0)
    for s in (2, 7, 8, 10, 13):                       # segments of no cluster
        assert np.all(KL[s] == 0.0) and np.all(KL[:, s] == 0.0)
    members = [(g, h, t, ind) for g, h in ((g1, h1), (g2, h2)) for t, ind in enumerate(g.indexes)]
    for ga, ha, ta, ia in members:
        for gb, hb, tb, ib in members:
            if ia < ib:
                ref = kl_ref.kl_pair(*_observed(ha, ta, False), *_observed(hb, tb, False), "inv")
                assert abs(KL[ia, ib] - ref) <= 1e-9 * max(abs(ref), 1.0)
                assert KL[ia, ib] == ga.KL_divergence(ta, gb, tb, smoothed=False, x_bas=sw.x_basis[0])
    for fn in (up.plot_MDS_plotly, up.plot_MDS):
        out = fn(sw, None, None, 0, lead=0)
        assert np.array_equal(out, KL)
    assert "figures are not part of" in capsys.readouterr().out


def _golden_model(c):
    """A GPI_model rebuilt from one cluster's stacks of kl_states.npz."""
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    gm = GPI_model(RBFWhiteKernel(*[float(v) for v in c["theta"]], device=DEV), c["x_basis"])
    T = len(c["x_basis"])
    gm.load_state(c["f_star"], c["Sigma"], c["C"], c["indexes"], f_star_sm=c["f_star_sm"], cov_f_sm=c["cov_f_sm"],
                  A=np.eye(T)[None], Gamma=c["Gamma_last"][None], cov_f=c["cov_f"])
    return gm


def _golden_tol(z):
    return max(1e-9, 50.0 * float(z["ref_sens"]))


def _parity(got, ref, tol, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0)))
    conftest.rel_err(got[np.abs(ref) > 1.0], ref[np.abs(ref) > 1.0])     # recorded in parity_observed.json
    print(f"{what}: err {err:.3e} tol {tol:.3e}")
    assert got.shape == ref.shape and err <= tol, (what, err, tol)


def test_golden_parity():
    """Every pair within and across the reference's clusters, both `smoothed` flags, and the blocks on another grid."""
    z = conftest.golden("kl_states.npz")
    tol = _golden_tol(z)
    models = {p: _golden_model(kl_ref.cluster(z, p)) for p in ("L_", "S_", "H_")}
    for name, p1, p2, sm, xb, t1, t2 in kl_ref.golden_blocks(z):
        g1, g2 = models[p1], models[p2]
        t1 = list(range(len(g1.indexes))) if t1 is None else [int(t) for t in t1]
        t2 = list(range(len(g2.indexes))) if t2 is None else [int(t) for t in t2]
        D = g1.kl_states(t1, g2, t2, smoothed=sm, x_bas=xb)
        _parity(D.cpu().numpy(), z[name], tol, name)
        v = g1.KL_divergence(t1[-1], g2, t2[0], smoothed=sm, x_bas=xb)      # the scalar is the 1 x 1 case, bit for bit
        assert v == D[len(t1) - 1, 0].item()
        if p1 == p2 and xb is None:
            S = g1.kl_states(t1, smoothed=sm)
            assert torch.equal(S, S.T)
            _parity(S.cpu().numpy(), z[name], tol, name + " self")


def test_near_identical_states():
    """Consecutive late states of the long cluster: the trace term nearly cancels against 2T."""
    z = conftest.golden("kl_states.npz")
    tol = _golden_tol(z)
    g = _golden_model(kl_ref.cluster(z, "L_"))
    n = len(g.indexes)
    late = list(range(n))        # the stored states are the last ones of a 62-member cluster (trace term within 1 % of 2T)
    for sm, tag in ((False, "f"), (True, "s")):
        ref = z["kl_LL_" + tag]
        D = g.kl_states(late, smoothed=sm).cpu().numpy()
        got = np.array([D[k, k + 1] for k in range(len(late) - 1)])
        want = np.array([ref[t, t + 1] for t in late[:-1]])
        _parity(got, want, tol, "consecutive late states " + tag)
        for t in late[:-1]:
            v = g.KL_divergence(t, g, t + 1, smoothed=sm)
            assert abs(v - ref[t, t + 1]) <= tol * max(abs(ref[t, t + 1]), 1.0)


def test_distance_matrix_golden(capsys):
    """kl_distance_matrix on the reference's two clusters of one lead against the matrix its plot_MDS loop produced."""
    import hdpgpc.util_plots as up
    from hdpgpc_amd import util_plots as upa
    z = conftest.golden("kl_states.npz")
    gL, gS = _golden_model(kl_ref.cluster(z, "L_")), _golden_model(kl_ref.cluster(z, "S_"))
    sw = types.SimpleNamespace(T=int(z["n_seg"]), M=2, gpmodels=[[gL, gS]], x_basis=[z["L_x_basis"]],
                               cond_to_torch=lambda x: torch.as_tensor(x, dtype=torch.float64, device=DEV))
    KL = upa.kl_distance_matrix(sw)
    _parity(KL, z["plot_mds"], _golden_tol(z), "plot_MDS matrix")
    assert np.array_equal(KL, KL.T) and np.all(np.diag(KL) == 0.0)
    assert np.array_equal(KL == 0.0, z["plot_mds"] == 0.0)                 # same placement, same empty rows
    assert np.array_equal(up.plot_MDS_plotly(sw, None, None, 0), KL)
    assert "figures are not part of" in capsys.readouterr().out


def test_static_dynamic_mix():
    """The caller's Gamma decides for both sides (GPI_model.py:918-921), in the scalar, the batched and the matrix path."""
    from hdpgpc_amd import util_plots as upa
    rng = np.random.default_rng(23)
    T = 8
    gs, hs = _model(rng, T, 3, [0, 2, 5], dynamic=False)
    gd, hd = _model(rng, T, 2, [1, 4])
    D = gs.kl_states(range(3), gd, range(2), smoothed=False)
    E = gd.kl_states(range(2), gs, range(3), smoothed=False)
    for t in range(3):
        for u in range(2):
            lat = kl_ref.kl_pair(hs["f"][t + 1], hs["P"][t + 1], hd["f"][u + 1], hd["P"][u + 1])
            obs = kl_ref.kl_pair(*_observed(hd, u, False), *_observed(hs, t, False))
            assert abs(D[t, u].item() - lat) <= 1e-9 * max(abs(lat), 1.0)
            assert abs(E[u, t].item() - obs) <= 1e-9 * max(abs(obs), 1.0)
            assert gs.KL_divergence(t, gd, u, smoothed=False) == D[t, u].item()
            assert gd.KL_divergence(u, gs, t, smoothed=False) == E[u, t].item()
    sw = types.SimpleNamespace(T=6, M=2, gpmodels=[[gs, gd]], x_basis=[np.arange(float(T))])
    KL = upa.kl_distance_matrix(sw)
    assert np.array_equal(KL, KL.T) and np.all(KL[3] == 0.0)
    assert KL[0, 1] == D[0, 0].item() and KL[1, 2] == E[0, 1].item() and KL[4, 5] == E[1, 2].item()


def test_full_size_record100_shape():
    """n = 2 272 states at T = 90 (the shape of record 100), in a child process under its own time limit: finite, 64 sampled
    pairs at the sweep's gate, and the same pairs as 1 x 1 calls bit for bit."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = f"import sys; sys.path.insert(0, {here!r}); import test_gpu_kl as t; t._full_size_body()"
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(here), capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stderr[-4000:]
    assert "full size ok" in r.stdout


def _full_size_body():
    import time
    from hdpgpc_amd import ops
    rng = np.random.default_rng(19)
    n, T = 2272, 90
    m, c = spd_states(rng, n, T, cond=1e3)
    m[n // 2:] = m[0] + 1e-3 * rng.standard_normal((n - n // 2, T))      # half of the states around one mean
    M, C = dev(m), dev(c)
    t0 = time.time()
    D = ops.kl_sym(M, C)
    torch.cuda.synchronize()
    print(f"kl_sym n={n} T={T}: {time.time() - t0:.3f} s (first call)")
    assert bool(torch.isfinite(D).all()) and torch.equal(D, D.T)
    Dh = D.cpu().numpy()
    ii, jj = rng.integers(0, n, 64), rng.integers(0, n, 64)
    ii[:4], jj[:4] = [0, n - 1, 127, 2271], [n - 1, 0, 128, 2144]
    r_inv = np.array([kl_ref.kl_pair(m[i], c[i], m[j], c[j], "inv") for i, j in zip(ii, jj)])
    r_chol = np.array([kl_ref.kl_pair(m[i], c[i], m[j], c[j], "chol") for i, j in zip(ii, jj)])
    check(Dh[ii, jj], r_inv, r_chol, "full size")
    for i, j in zip(ii, jj):
        one = ops.kl_sym(M[i:i + 1].contiguous(), C[i:i + 1].contiguous(), M[j:j + 1].contiguous(), C[j:j + 1].contiguous())
        assert one[0, 0].item() == Dh[i, j]
    print("full size ok")
