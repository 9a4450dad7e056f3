"""a14, curves drawn from the Gaussians of many states at once: hgp_sample_states_f64 through ops.sample_states,
GPI_model.sample_states / sample_last, IterativeGaussianProcess.sample_y and util_plots.model_samples.

Reference: CPU double precision, mean + z @ numpy.linalg.cholesky(0.5 (cov + cov^T))^T.  Gate: max|out - ref| <= 1e-10 max|ref|
per state (the project's a3 gate), on inputs whose covariance has condition number <= 1e4 (asserted on the
host before every comparison).  Position independence, containment and the exact zeros of the factor are bit for bit.
"""
import types

import numpy as np
import pytest
import torch

from conftest import golden, relclose

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-10
COND_MAX = 1e4

if torch.cuda.is_available():
    from hdpgpc_amd import ops
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def model_from(g, prefix="st_"):
    """As tests/test_gpu_mirror_api.py loads the reference's cluster state."""
    c, ell, noise = (float(v) for v in g[prefix + "theta"])
    m = GPI_model(RBFWhiteKernel(c, ell, noise), g[prefix + "x_basis"][:, None], bayesian=True)
    m.load_state(g[prefix + "f_star"], g[prefix + "Sigma"], g[prefix + "C"], g[prefix + "indexes"],
                 f_star_sm=g[prefix + "f_star_sm"], cov_f_sm=g[prefix + "cov_f_sm"], A=g[prefix + "A"],
                 Gamma=g[prefix + "Gamma"], A_def=g[prefix + "A_def"], Gamma_def=g[prefix + "Gamma_def"],
                 C_def=g[prefix + "C_def"], Sigma_def=g[prefix + "Sigma_def"], n0=float(g[prefix + "n0"]))
    return m


def synthetic(rng, T, S):
    """SPD covariances with a non-constant diagonal, fewer of them than states (repeated, out-of-order cov_idx) - as
    synthetic() of tests/test_gpu_bands.py builds its Sigma stack."""
    nC = max(2, S // 2 + 1)
    B = rng.standard_normal((nC, T, 6))
    cov = 0.05 * B @ B.transpose(0, 2, 1) + np.stack([np.diag(rng.uniform(0.1, 0.4, T)) for _ in range(nC)])
    idx = rng.integers(0, nC, S)
    idx[0] = nC - 1
    if S >= 3:
        idx[2] = idx[1]
    t = np.arange(float(T)) / T
    mean = np.stack([a * np.sin(2 * np.pi * (f * t + p)) + 0.3
                     for a, f, p in zip(rng.uniform(0.5, 3, S), rng.uniform(1, 4, S), rng.uniform(0, 1, S))])
    return mean, cov, idx.astype(np.int32)


def factor(cov):
    """Lower Cholesky factor of 0.5 (cov + cov^T) on the CPU; the condition number is asserted first."""
    A = 0.5 * (cov + cov.T)
    assert np.linalg.cond(A) <= COND_MAX
    return np.linalg.cholesky(A)


def assert_gate(out, ref, what):
    for s in range(ref.shape[0]):
        err = float(np.max(np.abs(out[s] - ref[s])) / np.max(np.abs(ref[s])))
        print(f"{what} state {s}: {err:.3e}")
        assert relclose(out[s], ref[s], GATE), (what, s, err)


# ------------------------------------------------------------------------------------------ 1. synthetic sweep
@pytest.mark.parametrize("T", [1, 15, 16, 17, 45, 64, 65, 90, 128, 129, 200, 256])
def test_synthetic_sweep(T):
    rng = np.random.default_rng(100 + T)
    S = 5
    mean, cov, idx = synthetic(rng, T, S)
    Ls = [factor(c) for c in cov]
    d_mean, d_cov, d_idx = dev(mean), dev(cov), dev(idx, torch.int32)
    for n in ((1, 63, 64, 65, 130) if T <= 128 else (1, 31, 33)):
        z = rng.standard_normal((S, n, T))
        for shared in (True, False):
            zz = z[0] if shared else z
            out, info = ops.sample_states(d_mean, d_cov, dev(zz), cov_idx=d_idx)
            assert tuple(out.shape) == (S, n, T) and not info.cpu().numpy().any()
            ref = np.stack([mean[s] + (z[0] if shared else z[s]) @ Ls[idx[s]].T for s in range(S)])
            assert_gate(out.cpu().numpy(), ref, f"T={T} n={n} shared={shared}")


# ------------------------------------------------------------------------------------------ 2. factor identity
@pytest.mark.parametrize("T", [45, 129])
def test_factor_identity(T):
    rng = np.random.default_rng(200 + T)
    S = 3
    mean, cov, idx = synthetic(rng, T, S)
    for c in cov:
        factor(c)                                              # the condition number
    d_mean, d_cov, d_idx = dev(mean), dev(cov), dev(idx, torch.int32)
    out, info = ops.sample_states(d_mean, d_cov, torch.eye(T, dtype=torch.float64, device=DEV), cov_idx=d_idx)
    assert not info.cpu().numpy().any()
    D = (out - d_mean[:, None, :]).cpu().numpy()               # D[s, j, t] = L_s[t, j]: the rows of L^T
    ju, tu = np.triu_indices(T, 1)
    for s in range(S):
        assert not D[s][tu, ju].any()                          # j > t: exactly zero
        A = 0.5 * (cov[idx[s]] + cov[idx[s]].T)
        err = float(np.max(np.abs(D[s].T @ D[s] - A)))
        print(f"T={T} state {s}: L L^T - A {err:.3e} (max diag {A.diagonal().max():.3e})")
        assert err <= GATE * A.diagonal().max()
    zero, _ = ops.sample_states(d_mean, d_cov, torch.zeros((4, T), dtype=torch.float64, device=DEV), cov_idx=d_idx)
    assert torch.equal(zero, d_mean[:, None, :].expand(S, 4, T))


# ------------------------------------------------------------------------------------------ 3. the reference's states
@pytest.mark.parametrize("tag", ["t30", "t45", "t90"])
def test_reference_states(tag):
    g = golden(f"state_{tag}.npz")
    m = model_from(g)
    T = len(g["st_x_basis"])
    rng = np.random.default_rng(300 + T)
    z = rng.standard_normal((70, T))

    def want(C, f, P, Sigma):
        return (C @ f.reshape(T)) + z @ factor(C @ P @ C.T + Sigma).T

    out = m.sample_states(ts=None, z=z)
    assert tuple(out.shape) == (1, 70, T)
    ref = want(g["st_C"][-1], g["st_f_star_sm"][-1], g["st_cov_f_sm"][-1], g["st_Sigma"][-1])
    assert_gate(out.cpu().numpy(), ref[None], f"{tag} last")
    # observed_moments: state t reads f_star_sm[t + 1] / cov_f_sm[t + 1] with C[t] / Sigma[t] (the last ones from estimation_limit on)
    n, nC = len(m.indexes), len(g["st_C"])
    ts = [0, n // 2, n - 1]
    ci = [(t if m.estimation_limit > t else -1) % nC for t in ts]
    out = m.sample_states(ts=ts, z=z)
    ref = np.stack([want(g["st_C"][c], g["st_f_star_sm"][t + 1], g["st_cov_f_sm"][t + 1], g["st_Sigma"][c]) for t, c in zip(ts, ci)])
    assert_gate(out.cpu().numpy(), ref, f"{tag} steps {ts}")
    zs = rng.standard_normal((3, 5, T))                        # per-state normals
    out = m.sample_states(ts=ts, z=zs)
    mom = m.observed_moments(ts, True, False)
    one = ops.sample_states(mom[0].contiguous(), mom[1].contiguous(), dev(zs))[0]
    assert torch.equal(out, one)


# ------------------------------------------------------------------------------------------ 4. public shapes and seeding
def test_public_shapes_and_seeding():
    g = golden("state_t45.npz")
    m = model_from(g)
    T = len(g["st_x_basis"])
    a = m.sample_last(3, random_state=7)
    b = m.sample_last(3, random_state=7)
    c = m.sample_last(3, random_state=8)
    assert isinstance(a, list) and len(a) == 3 and all(tuple(v.shape) == (T,) for v in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(torch.equal(x, y) for x, y in zip(a, c))
    full = m.sample_states(ts=None, num_samples=3, random_state=7)
    assert tuple(full.shape) == (1, 3, T) and torch.equal(torch.stack(a), full[0])
    assert tuple(m.sample_states(ts=[], num_samples=3).shape) == (0, 3, T)
    f, P, C, Sig = m.f_star_sm[-1], m.cov_f_sm[-1], m.C[-1], m.Sigma[-1]
    y1 = m.gp.sample_y(f.reshape(-1), P, C, Sig, n_samples=3, random_state=7)
    # the same seeding and the same state; the mean is formed as (C f)^T there, so its sum may round differently (T eps)
    assert tuple(y1.shape) == (T, 3) and relclose(y1.cpu().numpy(), full[0].T.cpu().numpy(), 1e-12)
    F2 = torch.stack([f.reshape(-1), 2.0 * f.reshape(-1)], 1)
    y2 = m.gp.sample_y(F2, P, C, Sig, n_samples=4, random_state=1)
    assert tuple(y2.shape) == (T, 2, 4) and bool(torch.isfinite(y2).all())
    y3 = m.gp.sample_y(f.reshape(-1, 1), P, C, Sig, n_samples=4, random_state=1)
    assert tuple(y3.shape) == (T, 1, 4) and torch.equal(y3, m.gp.sample_y(f.reshape(-1, 1), P, C, Sig, n_samples=4, random_state=1))


def test_driver_surface():
    import hdpgpc.util_plots as up
    from hdpgpc_amd import util_plots as upa
    gps = [model_from(golden("state_t45.npz")), model_from(golden("state_t45l3.npz"))]
    sw = types.SimpleNamespace(T=0, M=2, gpmodels=[gps], selected_gpmodels=lambda: [0, 1])
    assert up.model_samples is upa.model_samples
    res = upa.model_samples(sw, num_samples=7, random_state=3)
    T = gps[0].x_basis.shape[0]
    assert sorted(res) == ["clusters", "mean", "samples", "x_basis"]
    assert list(res["clusters"]) == [0, 1] and res["mean"].shape == (2, T) and res["samples"].shape == (2, 7, T)
    assert np.array_equal(res["x_basis"], gps[0].x_basis.reshape(-1).cpu().numpy())
    for k, gp in enumerate(gps):                               # per cluster what sample_states returns for it alone: bit for bit
        alone = gp.sample_states(ts=None, num_samples=7, random_state=3)[0]
        assert np.array_equal(res["samples"][k], alone.cpu().numpy())
    only = upa.model_samples(sw, [1], num_samples=7, random_state=3)
    assert list(only["clusters"]) == [1] and np.array_equal(only["samples"][0], res["samples"][1])
    mixed = types.SimpleNamespace(gpmodels=[[gps[0], model_from(golden("state_t30.npz"))]])   # two basis lengths: grouped by T
    res2 = upa.model_samples(mixed, num_samples=7, random_state=3)
    assert np.array_equal(res2["samples"][0], res["samples"][0]) and res2["samples"][1].shape == (7, 30)


# ------------------------------------------------------------------------------------------ 5. position independence
def test_position_independence():
    rng = np.random.default_rng(5)
    T, S, n = 90, 6, 130
    mean, cov, idx = synthetic(rng, T, S)
    d_mean, d_cov, d_idx = dev(mean), dev(cov), dev(idx, torch.int32)
    z = dev(rng.standard_normal((n, T)))
    full, _ = ops.sample_states(d_mean, d_cov, z, cov_idx=d_idx)
    bc, _ = ops.sample_states(d_mean, d_cov, z[None].expand(S, n, T).contiguous(), cov_idx=d_idx)
    assert torch.equal(full, bc)                               # z_shared = the same z broadcast
    for st in ([3], [5, 0], list(rng.permutation(S))):         # subsets and permutations of the states
        i = dev(np.asarray(st), torch.int64)
        got, _ = ops.sample_states(d_mean[i].contiguous(), d_cov, z, cov_idx=d_idx[i].contiguous())
        assert torch.equal(got, full[i]), st
    own, _ = ops.sample_states(d_mean[2:3].contiguous(), d_cov[idx[2]:idx[2] + 1].contiguous(), z)   # a state alone, no cov_idx
    assert torch.equal(own[0], full[2])
    for dr in ([129], [64, 63], list(range(17, 82)), list(rng.permutation(n))):   # subsets and permutations of the draws
        j = dev(np.asarray(dr), torch.int64)
        got, _ = ops.sample_states(d_mean, d_cov, z[j].contiguous(), cov_idx=d_idx)
        assert torch.equal(got, full[:, j]), dr
    zs = dev(rng.standard_normal((S, n, T)))                   # per-state normals: a draw alone, a state alone
    per, _ = ops.sample_states(d_mean, d_cov, zs, cov_idx=d_idx)
    got, _ = ops.sample_states(d_mean[4:5].contiguous(), d_cov, zs[4, 77:78].contiguous(), cov_idx=d_idx[4:5].contiguous())
    assert torch.equal(got[0, 0], per[4, 77])


# ------------------------------------------------------------------------------------------ 6. failure containment
@pytest.mark.parametrize("T", [90, 144])
def test_failure_containment(T):
    rng = np.random.default_rng(600 + T)
    S, n = 5, 70
    mean, cov, idx = synthetic(rng, T, S)
    cov = np.stack([cov[i] for i in idx])                      # one covariance per state
    good = [0, 2, 4]
    z = dev(rng.standard_normal((n, T)))
    ok, i0 = ops.sample_states(dev(mean[good]), dev(cov[good]), z)
    cov[1][7, 7] = -1.0                                        # not positive-definite
    cov[3][5, 5] = np.nan                                      # not finite
    out, info = ops.sample_states(dev(mean), dev(cov), z, check=False)
    torch.cuda.synchronize()
    info = info.cpu().numpy()
    assert torch.isnan(out[1]).all() and torch.isnan(out[3]).all()
    assert info[1] > 0 and info[3] == -1 and not info[good].any() and not i0.cpu().numpy().any()
    assert torch.equal(out[good], ok)
    with pytest.raises(torch.linalg.LinAlgError):
        ops.sample_states(dev(mean), dev(cov), z, check=True)
    torch.cuda.synchronize()


def test_input_is_symmetrised_and_untouched():
    rng = np.random.default_rng(7)
    T, S = 45, 3
    mean, cov, idx = synthetic(rng, T, S)
    skew = cov + np.triu(0.02 * rng.standard_normal((len(cov), T, T)), 1)
    sym = 0.5 * (skew + skew.transpose(0, 2, 1))
    for c in sym:
        factor(c)
    z = dev(rng.standard_normal((33, T)))
    d_skew = dev(skew)
    keep = d_skew.clone()
    a, _ = ops.sample_states(dev(mean), d_skew, z, cov_idx=dev(idx, torch.int32))
    b, _ = ops.sample_states(dev(mean), dev(sym), z, cov_idx=dev(idx, torch.int32))
    assert torch.equal(a, b) and torch.equal(d_skew, keep)
    jit, _ = ops.sample_states(dev(mean), dev(sym), z, cov_idx=dev(idx, torch.int32), jitter_rel=1e-2)
    ref = np.stack([mean[s] + z.cpu().numpy() @ factor(sym[idx[s]] + 1e-2 * np.mean(np.abs(np.diag(sym[idx[s]]))) * np.eye(T)).T
                    for s in range(S)])
    assert_gate(jit.cpu().numpy(), ref, "jitter_rel 1e-2")


# ------------------------------------------------------------------------------------------ the caller's workspace
@pytest.mark.parametrize("T", [16, 129])
def test_direct_call_stays_inside_the_reported_workspace(T):
    """hgp_sample_states_f64 on exactly hgp_sample_states_ws_bytes(S, T) bytes between two guard pads: the pads keep their bits
    and the outputs are the wrapper's, bit for bit."""
    import ws_guard
    from hdpgpc_amd import _ffi
    S, n = 2, 3
    rng = np.random.default_rng(500 + T)
    mean, cov, idx = synthetic(rng, T, S)
    mean, cov, idx, z = dev(mean), dev(cov), dev(idx, torch.int32), dev(rng.standard_normal((n, T)))
    want = ops.sample_states(mean, cov, z, cov_idx=idx)
    need = _ffi.lib.hgp_sample_states_ws_bytes(S, T)
    buf, ws = ws_guard.guarded(need, DEV)
    out, info = torch.empty_like(want[0]), torch.zeros(S, dtype=torch.int32, device=DEV)
    P = ops._ptr
    assert _ffi.lib.hgp_sample_states_f64(P(mean), P(cov), P(idx), T, S, P(z), n, 1, 0.0, P(out), P(info), ws, need, ops._stream()) == 0
    torch.cuda.synchronize()
    ws_guard.assert_pads_untouched(buf)
    assert not info.cpu().numpy().any()
    for got, ref in zip((out, info), want):
        ws_guard.assert_same_bits(got, ref)
