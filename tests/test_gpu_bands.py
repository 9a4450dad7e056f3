"""a2 on a query grid for many states at once: hgp_pred_bands_f64 through ops.pred_bands, GPI_model.bands and the
util_plots drivers (model_bands, model_evolution, plot_models*).

Gates.  Reference parity (the reference's own observe_last on the dense grid, state_*.npz) and the mirror API: relclose 1e-9,
the gate test_gpu_mirror_api applies to the composed path on the same data.  Oracle sweep: the project's a2 row - relclose
1e-8 for the mean, element-wise relative 1e-8 for the variance, on inputs whose oracle variance is at least 1e-3 (c + noise)
(asserted on the host).  Position independence, containment and the basis-grid short-circuit are bit for bit.
"""
import types

import numpy as np
import pytest
import torch

import conftest
import kl_ref
from conftest import golden, rel_err, relclose
from oracle import hdpgpc_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

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


def kl_model(c):
    """As tests/test_gpu_kl.py rebuilds a cluster of kl_states.npz."""
    gm = GPI_model(RBFWhiteKernel(*[float(v) for v in c["theta"]], device=DEV), c["x_basis"])
    T = len(c["x_basis"])
    gm.load_state(c["f_star"], c["Sigma"], c["C"], c["indexes"], f_star_sm=c["f_star_sm"], cov_f_sm=c["cov_f_sm"],
                  A=np.eye(T)[None], Gamma=c["Gamma_last"][None], cov_f=c["cov_f"])
    return gm


class Case:
    """Inputs of one call on the host: xb [T], theta [S,3], mean [S,T], Sig [nSig,T,T], idx [S], xq [Q]."""

    def __init__(self, xb, theta, mean, Sig, idx, xq):
        self.xb, self.theta, self.mean, self.Sig, self.idx, self.xq = xb, theta, mean, Sig, np.asarray(idx, dtype=np.int32), xq

        self._d = None

    def reset(self):
        self._d = None                                         # after a change of the host arrays

    def run(self, states=None, xq=None):
        if self._d is None:
            self._d = (dev(self.xb), dev(self.theta), dev(self.mean), dev(self.Sig), dev(self.idx, torch.int32), dev(self.xq))
        xb, theta, mean, Sig, idx, xq0 = self._d
        if states is not None:
            st = dev(np.asarray(states), torch.int64)
            theta, mean, idx = theta[st].contiguous(), mean[st].contiguous(), idx[st].contiguous()
        return ops.pred_bands(xb, theta, mean, Sig, xq0 if xq is None else dev(xq), sigma_idx=idx)

    def oracle(self, states=None, xq=None):
        st = range(len(self.idx)) if states is None else states
        xq = self.xq if xq is None else xq
        m, v = [], []
        for s in st:
            f, cov = orc.pred_dist(xq, self.xb, self.mean[s], self.Sig[self.idx[s]], tuple(self.theta[s]))
            m.append(f[:, 0])
            v.append(np.diag(cov))
        return np.array(m), np.array(v)


def queries(rng, xb, Q):
    """Unsorted query points over the basis range and a little beyond; some of them coincide with basis points."""
    xq = rng.uniform(xb.min() - 1.5, xb.max() + 1.5, Q)
    if Q >= 3:
        hit = rng.choice(Q, size=max(1, Q // 8), replace=False)
        xq[hit] = rng.choice(xb, size=len(hit))
    return xq


def synthetic(rng, T, S, Q, ell=None):
    """Per-state theta, SPD Sigma with a non-constant diagonal, fewer Sigma matrices than states (repeated, out-of-order
    sigma_idx), unsorted queries."""
    xb = np.arange(float(T))
    theta = np.stack([rng.uniform(0.5, 2.0, S), np.full(S, ell) if ell else rng.uniform(1.0, 1.5, S), rng.uniform(0.01, 0.1, S)], 1)
    nS = max(2, S // 2 + 1)
    B = rng.standard_normal((nS, T, 6))
    Sig = 0.05 * B @ B.transpose(0, 2, 1) + np.stack([np.diag(rng.uniform(0.1, 0.4, T)) for _ in range(nS)])
    idx = rng.integers(0, nS, S)
    idx[0] = nS - 1
    if S >= 3:
        idx[2] = idx[1]
    t = xb / T
    mean = np.stack([a * np.sin(2 * np.pi * (f * t + p)) for a, f, p in zip(rng.uniform(0.5, 3, S), rng.uniform(1, 4, S), rng.uniform(0, 1, S))])
    return Case(xb, theta, mean, Sig, idx, queries(rng, xb, Q))


def golden_case(rng, prefixes, Q):
    """States of the reference's clusters (kl_states.npz): C f_star_sm and Sigma of every stored step, each with its cluster's theta."""
    z = golden("kl_states.npz")
    xb = z[prefixes[0] + "x_basis"]
    theta, mean, Sig = [], [], []
    for p in prefixes:
        assert np.array_equal(z[p + "x_basis"], xb)
        n = z[p + "Sigma"].shape[0]
        mean.append(np.einsum("sij,sj->si", z[p + "C"], z[p + "f_star_sm"]))
        Sig.append(z[p + "Sigma"])
        theta.append(np.repeat(z[p + "theta"][None], n, 0))
    mean, Sig, theta = np.concatenate(mean), np.concatenate(Sig), np.concatenate(theta)
    return Case(xb, theta, mean, Sig, rng.permutation(len(mean)), queries(rng, xb, Q))


def check_oracle(case, what):
    want_m, want_v = case.oracle()
    floor = 1e-3 * (case.theta[:, 0] + case.theta[:, 2])
    assert np.all(want_v >= floor[:, None]), what            # the element-wise measure below is meaningful
    mq, vq, info = case.run()
    mq, vq = mq.cpu().numpy(), vq.cpu().numpy()
    assert not info.cpu().numpy().any()
    em = float(np.max(np.abs(mq - want_m)) / max(float(np.max(np.abs(want_m))), 1e-300))
    ev = rel_err(vq, want_v)
    conftest._note(em)
    print(f"{what}: mean {em:.3e} var {ev:.3e}")
    assert mq.shape == want_m.shape and vq.shape == want_v.shape
    assert relclose(mq, want_m, 1e-8), (what, em)
    assert ev <= 1e-8, (what, ev)


# ------------------------------------------------------------------------------------------ 1. reference parity
@pytest.mark.parametrize("tag", ["t30", "t45", "t90", "t45l3"])
def test_reference_parity(tag):
    """The reference's own observe_last on the dense grid (T* = 2T - 1), length-scale 3.0 included."""
    g = golden(f"state_{tag}.npz")
    m = model_from(g)
    mean, var = m.bands(g["x_dense"][:, None])
    mean, var = mean.cpu().numpy()[0], var.cpu().numpy()[0]
    want_v = np.diag(g["obs_last_cov"])
    print(f"{tag}: mean {rel_err(mean, g['obs_last_f']):.3e} var {rel_err(var, want_v):.3e} (element-wise)")
    assert relclose(mean, g["obs_last_f"], 1e-9)
    assert relclose(var, want_v, 1e-9)


# ------------------------------------------------------------------------------------------ 2. oracle sweep
# every T of {8, 45, 90, 128, 129, 144, 256}, every Q of {1, 15, 16, 17, 100, 891}, every S of {1, 3, 70}
SWEEP = [(8, 1, 1), (8, 17, 3), (8, 100, 70), (45, 15, 3), (45, 891, 70), (90, 16, 1), (90, 891, 3), (128, 100, 3), (128, 17, 70),
         (129, 15, 3), (129, 100, 1), (144, 891, 3), (144, 16, 70), (256, 1, 3), (256, 17, 1), (256, 100, 3)]


@pytest.mark.parametrize("T,Q,S", SWEEP)
def test_oracle_sweep(T, Q, S):
    rng = np.random.default_rng(1000 * T + 10 * Q + S)
    check_oracle(synthetic(rng, T, S, Q, ell=1.2 if T == 256 else None), f"synthetic T={T} Q={Q} S={S}")


@pytest.mark.parametrize("prefixes,Q", [(("L_", "S_"), 100), (("L_", "S_"), 17), (("H_",), 100), (("H_",), 891)])
def test_oracle_golden_states(prefixes, Q):
    rng = np.random.default_rng(7 + Q)
    check_oracle(golden_case(rng, prefixes, Q), f"kl_states {prefixes} Q={Q}")


# ------------------------------------------------------------------------------------------ 3. far queries
def test_far_query():
    rng = np.random.default_rng(3)
    case = synthetic(rng, 45, 3, 40)
    ell_max = float(case.theta[:, 1].max())
    far_pos = np.array([0, 5, 17, 18, 39])
    xq = case.xq.copy()
    xq[far_pos] = [case.xb.min() - 40.0 * ell_max, case.xb.max() + 40.0 * ell_max, case.xb.max() + 1e3, case.xb.min() - 65.0,
                   case.xb.max() + 47.0 * ell_max]
    keep = np.setdiff1d(np.arange(40), far_pos)
    mq, vq, _ = case.run(xq=xq)
    m0, v0, _ = case.run(xq=xq[keep])
    scale = float(np.abs(case.mean).max())
    assert torch.all(mq[:, far_pos].abs() <= 1e-300 * scale)
    want = torch.as_tensor(case.theta[:, 0] + case.theta[:, 2] + 1e-6, device=DEV)[:, None]
    assert torch.all((vq[:, far_pos] - want).abs() <= 1e-15 * want)
    assert torch.equal(mq[:, keep], m0) and torch.equal(vq[:, keep], v0)     # neighbours in the same 16-tile: bit for bit


# ------------------------------------------------------------------------------------------ 4. the iso branch and its edge
@pytest.mark.parametrize("sigma,T", [(0.25, 45), (0.7, 45), (0.7, 144)])
def test_iso_branch(sigma, T):
    rng = np.random.default_rng(4)
    case = synthetic(rng, T, 4, 33)
    band = 1e-8 + 1e-5 * sigma
    delta = {1: 0.9, 2: 1.1}                                   # state 1 just inside the isclose band, state 2 just outside
    Sig = np.stack([sigma * np.eye(T) for _ in range(4)])
    for s, f in delta.items():
        Sig[s][0, 0] += f * band / (1.0 - 1.0 / T)
    Sig[3] = case.Sig[0]                                       # an ordinary state in the same call
    case.Sig, case.idx = Sig, np.arange(4, dtype=np.int32)
    want_m, want_v = case.oracle()
    assert np.all(np.abs(want_v[0] - sigma) <= 1e-15 * sigma) and np.ptp(want_v[1]) == 0.0 and np.ptp(want_v[2]) > 1e-3 and np.ptp(want_v[3]) > 1e-3
    mq, vq, info = case.run()
    mq, vq = mq.cpu().numpy(), vq.cpu().numpy()
    assert not info.cpu().numpy().any()
    assert np.all(np.abs(vq[0] - sigma) <= 1e-15 * sigma)
    assert relclose(mq, want_m, 1e-8)                          # the mean is still computed
    assert rel_err(vq, want_v) <= 1e-8                         # every state took the branch the oracle took


# ------------------------------------------------------------------------------------------ 5. position independence
@pytest.mark.parametrize("T,Q", [(90, 891), (144, 100)])
def test_position_independence(T, Q):
    rng = np.random.default_rng(5)
    S = 70
    case = synthetic(rng, T, S, Q)
    mq, vq, _ = case.run()
    for s in range(S):                                         # every state alone
        m1, v1, _ = case.run(states=[s])
        assert torch.equal(m1[0], mq[s]) and torch.equal(v1[0], vq[s]), s
    perm = rng.permutation(Q)                                  # the queries permuted
    mp, vp, _ = case.run(xq=case.xq[perm])
    assert torch.equal(mp, mq[:, perm]) and torch.equal(vp, vq[:, perm])
    for chunk in (1, 17, 64):                                  # the queries in chunks
        got = [case.run(xq=case.xq[q0:q0 + chunk]) for q0 in range(0, Q, chunk)]
        assert torch.equal(torch.cat([r[0] for r in got], 1), mq) and torch.equal(torch.cat([r[1] for r in got], 1), vq), chunk
    rev = list(range(S))[::-1]                                 # the states reversed
    mr, vr, _ = case.run(states=rev)
    assert torch.equal(mr, mq.flip(0)) and torch.equal(vr, vq.flip(0))


# ------------------------------------------------------------------------------------------ 6. NaN containment
def test_nan_containment():
    rng = np.random.default_rng(6)
    case = synthetic(rng, 90, 5, 100)
    case.Sig = np.stack([case.Sig[i] for i in case.idx])
    case.idx = np.arange(5, dtype=np.int32)
    good = [0, 1, 3, 4]
    m0, v0, i0 = case.run(states=good)
    case.Sig[2][7, 7] = np.nan
    case.reset()
    mq, vq, info = case.run()
    torch.cuda.synchronize()
    assert torch.all(torch.isnan(mq[2])) and torch.all(torch.isnan(vq[2])) and int(info[2]) != 0
    assert torch.equal(mq[good], m0) and torch.equal(vq[good], v0)
    assert not info[good].any() and not i0.any()
    with pytest.raises(torch.linalg.LinAlgError):
        ops.pred_bands(dev(case.xb), dev(case.theta), dev(case.mean), dev(case.Sig), dev(case.xq), check=True)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 7. mirror API
def test_mirror_api():
    g = golden("state_t45.npz")
    m = model_from(g)
    x = g["x_dense"][:, None]
    n = len(m.indexes)
    ts = [0, 1, n // 2, n - 2, n - 1, n, n + 3]                # t < len(indexes), t == len(indexes) - 1, t >= len(indexes)
    mean, var = m.bands(x, ts)
    assert tuple(mean.shape) == tuple(var.shape) == (len(ts), len(x))
    for row, t in enumerate(ts):
        f, cov = m.observe(x, t)
        assert relclose(mean[row].cpu().numpy(), f.cpu().numpy()[:, 0], 1e-9), t
        assert relclose(var[row].cpu().numpy(), np.diag(cov.cpu().numpy()), 1e-9), t
    f, cov = m.observe_last(x)
    mean, var = m.bands(x)
    assert relclose(mean[0].cpu().numpy(), f.cpu().numpy()[:, 0], 1e-9)
    assert relclose(var[0].cpu().numpy(), np.diag(cov.cpu().numpy()), 1e-9)
    xb = g["st_x_basis"][:, None]                              # the basis grid itself: C f and diag Sigma, no kernel
    mean, var = m.bands(xb, ts)
    for row, t in enumerate(ts):
        f, cov = m.observe(xb, t)
        assert torch.equal(mean[row], f[:, 0]) and torch.equal(var[row], torch.diagonal(cov)), t
    f, cov = m.observe_last(xb)
    mean, var = m.bands(xb)
    assert torch.equal(mean[0], f[:, 0]) and torch.equal(var[0], torch.diagonal(cov))
    e1, e2 = m.bands(x, [])
    assert tuple(e1.shape) == tuple(e2.shape) == (0, len(x))


# ------------------------------------------------------------------------------------------ 8. the drivers' surface
def test_driver_surface(capsys):
    import hdpgpc.util_plots as up
    from hdpgpc_amd import util_plots as upa
    z = golden("kl_states.npz")
    gL, gS = kl_model(kl_ref.cluster(z, "L_")), kl_model(kl_ref.cluster(z, "S_"))
    sw = types.SimpleNamespace(T=int(z["n_seg"]), M=2, gpmodels=[[gL, gS]], x_basis=[z["L_x_basis"]],
                               cond_to_torch=lambda x: torch.as_tensor(x, dtype=torch.float64, device=DEV))
    out = upa.model_bands(sw)
    assert sorted(out) == [0, 1]
    for k, gp in enumerate((gL, gS)):
        d = out[k]
        xb = gp.x_basis.reshape(-1).cpu()
        x = torch.arange(float(xb.min()), float(xb.max()), 0.1, dtype=torch.float64)
        assert np.array_equal(d["x"], x.numpy()) and np.array_equal(d["x_basis"], xb.numpy())
        assert np.array_equal(d["lower"], d["mean"] - 1.9 * np.sqrt(d["var"]))
        assert np.array_equal(d["upper"], d["mean"] + 1.9 * np.sqrt(d["var"]))
        f, cov = gp.observe_last(x[:, None])
        assert relclose(d["mean"], f.cpu().numpy()[:, 0], 1e-9)
        assert relclose(d["var"], np.diag(cov.cpu().numpy()), 1e-9)
        assert np.array_equal(d["mean_latent"], gp.f_star_sm[-1].reshape(-1).cpu().numpy())
        assert np.array_equal(d["noise_latent"], 1.9 * np.sqrt(np.diag(gp.Gamma[-1].cpu().numpy())))
    only = upa.model_bands(sw, [1])
    assert sorted(only) == [1] and all(np.array_equal(only[1][k], out[1][k]) for k in out[1])
    for fn in (up.plot_models_plotly, up.plot_models):
        got = fn(sw, [0, 1], None, None, 0)
        assert sorted(got) == [0, 1] and all(np.array_equal(got[m][k], out[m][k]) for m in out for k in out[m])
    assert "figures are not part of" in capsys.readouterr().out
    ev = upa.model_evolution(sw, 0)
    n = len(gL.indexes)
    assert ev["mean"].shape == ev["var"].shape == (n, len(out[0]["x"])) and np.array_equal(ev["indexes"], gL.indexes)
    for j in range(n):                                         # one row per member, row j = bands(x, [j])
        mj, vj = gL.bands(ev["x"], [j])
        assert np.array_equal(ev["mean"][j], mj[0].cpu().numpy()) and np.array_equal(ev["var"][j], vj[0].cpu().numpy())
    part = up.plot_partial_models(sw, [0], None, None, 0, time_instant=[1, n - 1])
    assert np.array_equal(part[0]["mean"], ev["mean"][[1, n - 1]])


# ------------------------------------------------------------------------------------------ the caller's workspace
@pytest.mark.parametrize("T", [16, 128, 129])
def test_direct_call_stays_inside_the_reported_workspace(T):
    """hgp_pred_bands_f64 on exactly hgp_pred_bands_ws_bytes(S, T) bytes between two guard pads, both layouts (the factor's
    scratch exists for T > 128 only): the pads keep their bits and the outputs are the wrapper's, bit for bit."""
    import ws_guard
    from hdpgpc_amd import _ffi
    S, Q = 2, 3
    case = synthetic(np.random.default_rng(500 + T), T, S, Q)
    want = case.run()
    xb, theta, mean, Sig, idx, xq = case._d
    need = _ffi.lib.hgp_pred_bands_ws_bytes(S, T)
    buf, ws = ws_guard.guarded(need, DEV)
    mean_q, var_q = torch.empty_like(want[0]), torch.empty_like(want[1])
    info = torch.zeros(S, dtype=torch.int32, device=DEV)
    P = ops._ptr
    assert _ffi.lib.hgp_pred_bands_f64(P(xb), T, P(theta), P(mean), P(Sig), P(idx), S, P(xq), Q, P(mean_q), P(var_q), P(info), ws, need,
                                       ops._stream()) == 0
    torch.cuda.synchronize()
    ws_guard.assert_pads_untouched(buf)
    assert not info.cpu().numpy().any()
    for got, ref in zip((mean_q, var_q, info), want):
        ws_guard.assert_same_bits(got, ref)
