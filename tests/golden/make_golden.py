#!/usr/bin/env python3
"""Generate golden input/output vectors for the GP-emission hot path by RUNNING THE REFERENCE.

Build-container only: imports the read-only reference at /root/reference (never copied), with
in-memory stand-ins for the four third-party packages that are absent here (gpytorch,
torchmetrics, pyro, wfdb) and with kernel hyper-parameters injected in place of the gpytorch fit
 - every vector is taken downstream of that injection.

Usage (from the repo root):   python tests/golden/make_golden.py
Writes tests/golden/*.npz - data only (inputs + the reference's outputs, fp64).
"""
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference/hdpgpc"
OUT = os.path.dirname(os.path.abspath(__file__))
THETA_INJECT = (341.0, 1.2, 4.66)  # outputscale, lengthscale (GPI.py:711 forces 1.2), noise before clamping


def _register_standins():
    def _mod(n):
        m = types.ModuleType(n)
        sys.modules[n] = m
        return m

    g = _mod("gpytorch")
    for s in ["models", "variational", "means", "kernels", "likelihoods", "constraints", "mlls",
              "distributions", "settings"]:
        setattr(g, s, _mod("gpytorch." + s))

    class _B(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()

    g.models.ExactGP = g.models.ApproximateGP = g.means.Mean = _B
    g.variational.CholeskyVariationalDistribution = g.variational.VariationalStrategy = _B
    tm = _mod("torchmetrics")
    tm.audio = _mod("torchmetrics.audio")

    class SignalNoiseRatio:  # torchmetrics.functional.audio.signal_noise_ratio, zero_mean=False
        def __call__(self, preds, target):
            eps = torch.finfo(preds.dtype).eps
            noise = target - preds
            return 10 * torch.log10((torch.sum(target ** 2, -1) + eps) / (torch.sum(noise ** 2, -1) + eps))

    tm.audio.SignalNoiseRatio = SignalNoiseRatio
    p = _mod("pyro")
    p.contrib = _mod("pyro.contrib")
    p.contrib.gp = _mod("pyro.contrib.gp")
    p.distributions = _mod("pyro.distributions")
    w = _mod("wfdb")
    w.processing = _mod("wfdb.processing")


_register_standins()
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
import hdpgpc.GPI as GPI  # noqa: E402
import hdpgpc.GPI_model as GM  # noqa: E402
import hdpgpc.GPI_HDP as HDP  # noqa: E402
from hdpgpc.get_data import compute_estimators_LDS  # noqa: E402
from hdpgpc.amtgp_warping_system import WarpPriorAMTGP, Warping_system  # noqa: E402
from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel  # noqa: E402


def _fit_torch_fixed(self, x, y, alpha_ini, gamma_ini, reduced_points=False, verbose=False):
    """Harness-only replacement of the gpytorch fit: inject fixed theta."""
    if not self.fitted:
        k = self.kernel
        k.k1.k1.theta = np.log([THETA_INJECT[0]])
        k.k1.k2.theta = np.log([THETA_INJECT[1]])
        lo, hi = k.k2.noise_level_bounds
        k.k2.theta = np.log([min(max(THETA_INJECT[2], lo), hi)])
        x_ = self.cond_to_numpy(self.x_basis)
        self.K_X_X = self.cond_to_torch(self.kernel(x_, x_))
        self.K_inv = self.inv_r("kernelMat", self.K_X_X)
        self.fitted = True
        eye = torch.eye(self.x_basis.shape[0])
        self.assign_alpha_ini(torch.mul(self.cond_to_torch(k.k2.noise_level), eye),
                              torch.mul(self.cond_to_torch(gamma_ini), eye))
    return self.fitted


GPI.IterativeGaussianProcess.fit_torch = _fit_torch_fixed
torch.set_default_dtype(torch.float64)


def npy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def kernel_theta(k):
    return np.array([k.k1.k1.constant_value, k.k1.k2.length_scale, k.k2.noise_level], dtype=np.float64)


def make_kernel(c, ell, noise, nb=(1e-10, 1e10)):
    return ConstantKernel(c, (c, c * 5.0)) * RBF(ell, (1.0, 20.0)) + WhiteKernel(noise, nb)


# ----------------------------------------------------------------------------- a1
def gen_gram():
    rng = np.random.default_rng(1)
    out = {}
    cases = [(8, 8, 2.5, 1.2, 0.3), (33, 20, 341.0, 1.2, 0.9), (90, 178, 300.0, 3.0, 1e-3), (128, 128, 17.0, 0.7, 2.0)]
    for i, (n, m, c, ell, noise) in enumerate(cases):
        k = make_kernel(c, ell, noise)
        X = (np.arange(n) + rng.uniform(-0.3, 0.3, n))[:, None]
        Y = (np.linspace(0, n - 1, m) + rng.uniform(-0.2, 0.2, m))[:, None]
        out[f"c{i}_theta"] = np.array([c, ell, noise])
        out[f"c{i}_X"] = X[:, 0]
        out[f"c{i}_Y"] = Y[:, 0]
        out[f"c{i}_K_one"] = k(X)          # one-argument call: white noise on the diagonal
        out[f"c{i}_K_two"] = k(X, Y)       # two-argument call: no white noise
        out[f"c{i}_K_self"] = k(X, X)
    out["n_cases"] = np.array(len(cases))
    np.savez_compressed(os.path.join(OUT, "gram.npz"), **out)


# ------------------------------------------------------------------------ a3, a4
def gen_score_shared():
    rng = np.random.default_rng(2)
    xb = np.arange(8.0)[:, None]
    gm = GM.GPI_model(make_kernel(1.0, 1.0, 0.1), xb, verbose=False)
    out = {}
    i = 0
    for T in (8, 33, 90, 128):
        for B in (1, 7, 64):
            for kind in ("iso", "dense"):
                if kind == "iso":
                    cov = 2.3 * np.eye(T)
                else:
                    Q = rng.normal(size=(T, T))
                    cov = Q @ Q.T / T + np.diag(rng.uniform(0.5, 2.0, T))
                    cov = cov + 1e-3 * rng.normal(size=(T, T))  # slightly non-symmetric on purpose (a3 symmetrises)
                mean = rng.normal(size=(T, 1)) * 10
                Y = rng.normal(size=(B, T, 1)) * 3 + mean[None]
                sc = gm._gaussian_score_shared_cov(torch.from_numpy(Y), torch.from_numpy(mean), torch.from_numpy(cov))
                L = gm._chol_spd(torch.from_numpy(cov))
                out[f"c{i}_cov"], out[f"c{i}_mean"], out[f"c{i}_Y"] = cov, mean[:, 0], Y[..., 0]
                out[f"c{i}_score"], out[f"c{i}_L"] = npy(sc), npy(L)
                i += 1
    out["n_cases"] = np.array(i)
    np.savez_compressed(os.path.join(OUT, "score_shared.npz"), **out)


# ----------------------------------------------------------------------------- a2
def gen_pred_dist():
    rng = np.random.default_rng(3)
    out = {}
    i = 0
    for (T, Ts, c, ell, noise) in [(8, 8, 5.0, 1.2, 0.5), (33, 33, 341.0, 1.2, 0.9), (33, 50, 341.0, 1.2, 0.9),
                                   (90, 178, 341.0, 1.2, 0.9), (128, 128, 358.05, 1.2, 0.9), (48, 48, 100.0, 3.0, 0.2)]:
        xb = np.arange(float(T))[:, None]
        gp = GPI.IterativeGaussianProcess(make_kernel(c, ell, noise), xb, verbose=False)
        if Ts == T:
            xp = xb + rng.uniform(-0.3, 0.3, (T, 1))
        else:
            xp = np.linspace(0, T - 1, Ts)[:, None]
        for kind in ("dense", "iso"):
            if kind == "iso":
                Sig = 1.7 * np.eye(T)
            else:
                v = rng.normal(size=T)
                Sig = rng.uniform(0.5, 5.0) * (np.eye(T) + 0.1 * np.outer(v, v))
            mean = 50 * np.exp(-0.5 * ((xb - T / 2) / (0.1 * T)) ** 2) + rng.normal(size=(T, 1))
            f, cov = gp.pred_dist(torch.from_numpy(xp), torch.from_numpy(xb), torch.from_numpy(mean), torch.from_numpy(Sig))
            fl, covl = gp.pred_latent_dist(torch.from_numpy(xp), torch.from_numpy(xb), torch.from_numpy(mean),
                                           torch.from_numpy(Sig))
            out[f"c{i}_theta"] = np.array([c, ell, noise])
            out[f"c{i}_xb"], out[f"c{i}_xp"], out[f"c{i}_mean"], out[f"c{i}_Sigma"] = xb[:, 0], xp[:, 0], mean[:, 0], Sig
            out[f"c{i}_f"], out[f"c{i}_cov"] = npy(f)[:, 0], npy(cov)
            out[f"c{i}_f_lat"], out[f"c{i}_cov_lat"] = npy(fl)[:, 0], npy(covl)
            i += 1
    out["n_cases"] = np.array(i)
    np.savez_compressed(os.path.join(OUT, "pred_dist.npz"), **out)



# ------------------------------------------- a2 + a5 at the drivers' ini_lengthscale (ill-conditioned K~)
def gen_pairs_ill():
    """Per-pair path (pred_dist + log_sq_error score) where K~ is ill-conditioned: the length-scale every driver
    constructs its kernels with (ini_lengthscale = 3.0, hdpgpc/tests/test_offline.py:51, test_online.py:53) and 2.5, on
    irregular grids at T = 45 / 90 / 128 (plus one case with T* != T).  Scores come from the reference's own
    GPI_model.log_sq_error(mean=, C=, Sigma=, i=0) -> observe(params) -> pred_dist (GPI_model.py:250-286,657-662)."""
    rng = np.random.default_rng(21)
    out = {}
    i = 0
    for (T, Ts) in [(45, 45), (90, 90), (128, 128), (90, 64)]:
        for ell in (2.5, 3.0):
            xb = np.arange(float(T))[:, None]
            K, N = 3, 5
            thetas, means, Sigs = [], [], []
            for k in range(K):
                c, noise = 300.0 * (1 + 0.1 * k), 0.9 * (1 + 0.5 * k)
                thetas.append((c, ell, noise))
                v = rng.normal(size=T)
                Sigs.append(rng.uniform(0.5, 5.0) * (np.eye(T) + 0.1 * np.outer(v, v)))
                means.append((100 + 50 * k) * np.exp(-0.5 * ((xb[:, 0] - T * (0.3 + 0.2 * k)) / (0.08 * T)) ** 2)
                             + rng.normal(size=T))
            if Ts == T:
                x = xb[None, :, 0] + rng.uniform(-0.3, 0.3, (N, T))
            else:
                x = np.linspace(0, T - 1, Ts)[None, :] + rng.uniform(-0.2, 0.2, (N, Ts))
            z = rng.integers(0, K, N)
            y = np.stack([np.interp(x[n], xb[:, 0], means[z[n]]) for n in range(N)]) + rng.normal(0, 3.0, (N, Ts))
            score = np.zeros((N, K))
            score_first = np.zeros((N, K))
            eyeT = torch.eye(T)
            for k in range(K):
                c, _, noise = thetas[k]
                gm = GM.GPI_model(make_kernel(c, ell, noise), xb, verbose=False)
                cond = gm.GPR_dynamic(0.5, 2.0)
                gm.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
                for n in range(N):
                    xt, yt = torch.from_numpy(x[n][:, None]), torch.from_numpy(y[n][:, None])
                    kw = dict(mean=torch.from_numpy(means[k][:, None]), cov=eyeT, C=eyeT, Sigma=torch.from_numpy(Sigs[k]), i=0)
                    score[n, k] = float(gm.log_sq_error(xt, yt, **kw))
                    score_first[n, k] = float(gm.log_sq_error(xt, yt, first=True, **kw))
            out[f"c{i}_xb"], out[f"c{i}_x"], out[f"c{i}_y"] = xb[:, 0], x, y
            out[f"c{i}_theta"], out[f"c{i}_mean"], out[f"c{i}_Sigma"] = np.array(thetas), np.stack(means), np.stack(Sigs)
            out[f"c{i}_score"], out[f"c{i}_score_first"] = score, score_first
            out[f"c{i}_ini_noise"] = np.array(1e-2 * 2.0)          # first: 1e-2 mean diag Sigma[0], Sigma[0] = 2.0 I
            i += 1
    out["n_cases"] = np.array(i)
    np.savez_compressed(os.path.join(OUT, "pairs_ill.npz"), **out)
    print(f"pairs_ill: {i} cases")

# --------------------------------------------------------- a5-a9 on a real LDS state
def load_beats(rec, n, stride=1, lead=0):
    d = np.load(os.path.join(REF, "data", "mitbih", f"{rec}.npy"))[:n, ::stride, [lead]]
    return np.ascontiguousarray(d)


def build_model(data, members, free_deg=5):
    """One GPI_model driven through the reference's own full_pass_weighted on ``members``."""
    N, T, _ = data.shape
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    kern = ConstantKernel(300.0, (300.0, 1500.0)) * RBF(3.0, (1.0, 20.0)) + WhiteKernel(bound_sigma[0], bound_sigma)
    gm = GM.GPI_model(kern, xb, annealing=True, bayesian=True, free_deg_MNIV=free_deg, verbose=False)
    cond = gm.GPR_dynamic(std_dif, std)
    gm.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    x_trains = torch.from_numpy(np.array([xb] * N))
    y_trains = torch.from_numpy(data)
    resp = torch.zeros(N)
    resp[list(members)] = 1.0
    q, q_lat = gm.full_pass_weighted(x_trains, y_trains, resp)
    return gm, x_trains, y_trains, q, q_lat


def dump_state(gm, prefix, out):
    out[prefix + "theta"] = kernel_theta(gm.gp.kernel)
    out[prefix + "x_basis"] = npy(gm.x_basis)[:, 0]
    out[prefix + "indexes"] = np.array(gm.indexes, dtype=np.int64)
    for name in ("f_star", "f_star_sm"):
        out[prefix + name] = np.stack([npy(f).reshape(-1) for f in getattr(gm, name)])
    for name in ("cov_f_sm", "A", "Gamma", "C", "Sigma"):
        out[prefix + name] = np.stack([npy(m) for m in getattr(gm, name)])
    for name in ("A_def", "Gamma_def", "C_def", "Sigma_def"):
        out[prefix + name] = npy(getattr(gm, name))
    out[prefix + "n0"] = np.array(float(gm.internal_params.n0))


def gen_state(tag, rec, n, stride, members, seed, theta=None):
    """theta overrides the injected kernel hyper-parameters (e.g. the drivers' ini_lengthscale = 3.0 in place of the
    1.2 that GPI.py:711 forces after a valid fit: the state of a model whose kernel was never (validly) fitted)."""
    global THETA_INJECT
    keep = THETA_INJECT
    if theta is not None:
        THETA_INJECT = theta
    try:
        _gen_state(tag, rec, n, stride, members, seed)
    finally:
        THETA_INJECT = keep


def _gen_state(tag, rec, n, stride, members, seed):
    rng = np.random.default_rng(seed)
    data = load_beats(rec, n, stride)
    gm, x_trains, y_trains, q, q_lat = build_model(data, members)
    T = data.shape[1]
    out = {"y": data[..., 0]}
    dump_state(gm, "st_", out)
    out["q_shared"] = npy(q)
    out["q_lat"] = npy(q_lat)
    out["q_shared_nofirst"] = npy(gm.compute_sq_err_all(x_trains, y_trains, no_first=True))
    # irregular grids: per-segment general path (3 Gram builds + 2 Cholesky per evaluation)
    x_irr = np.arange(float(T))[None, :, None] + rng.uniform(-0.3, 0.3, (n, T, 1))
    out["x_irr"] = x_irr[..., 0]
    out["q_irr"] = npy(gm.compute_sq_err_all(torch.from_numpy(x_irr), y_trains))
    # online-style calls against the last state (i=-1) and with explicit params / first
    out["lse_last"] = np.array([float(gm.log_sq_error(torch.from_numpy(x_irr[j]), y_trains[j], i=-1)) for j in range(n)])
    out["lse_last_shared"] = np.array([float(gm.log_sq_error(x_trains[j], y_trains[j], i=-1)) for j in range(n)])
    out["lse_none"] = np.array([float(gm.log_sq_error(torch.from_numpy(x_irr[j]), y_trains[j])) for j in range(n)])
    pm, pc, pC, pS = gm.f_star_sm[-2], gm.cov_f_sm[-2], gm.C[-2], gm.Sigma[-2]
    out["lse_params_first"] = np.array([float(gm.log_sq_error(torch.from_numpy(x_irr[j]), y_trains[j], mean=pm, cov=pc,
                                                              C=pC, Sigma=pS, i=0, first=True)) for j in range(n)])
    out["lds_lik"] = np.array(float(gm.return_LDS_param_likelihood()))
    out["lds_lik_first"] = np.array(float(gm.return_LDS_param_likelihood(first=True)))
    # raw MNIW terms
    ip = GM.matrix_normal_inv_wishart(gm.C_def, torch.eye(T), gm.free_deg_MNIV, gm.Sigma_def)
    out["mniw_obs"] = np.array(float(ip.log_likelihood_MNIW(gm.C[-1], gm.Sigma[-1], gm.internal_params.n0)))
    # observe_last on a denser grid (util_plots.py:755-758 does this with step 0.5)
    xd = np.arange(0, T - 1 + 1e-9, 0.5)[:, None]
    f, cov = gm.observe_last(torch.from_numpy(xd))
    out["x_dense"], out["obs_last_f"], out["obs_last_cov"] = xd[:, 0], npy(f)[:, 0], npy(cov)
    np.savez_compressed(os.path.join(OUT, f"state_{tag}.npz"), **out)
    print(f"state_{tag}: T={T} members={list(members)} q_irr[:3]={out['q_irr'][:3]}")


# ---------------------------------------------------------------------------- a10
def gen_lml():
    rng = np.random.default_rng(5)
    out = {}
    for i, (T, c, ell, noise) in enumerate([(16, 3.0, 1.5, 0.2), (60, 341.0, 1.2, 0.9), (90, 300.0, 3.0, 0.5)]):
        xb = np.arange(float(T))[:, None]
        k = make_kernel(c, ell, noise)
        gp = GPI.IterativeGaussianProcess(k, xb, verbose=False)
        y = np.sin(xb / 5.0) * 10 + rng.normal(size=(T, 1))
        val = gp.log_marginal_likelihood(torch.from_numpy(xb), torch.from_numpy(y), None, theta=k.theta)
        out[f"c{i}_theta"], out[f"c{i}_x"], out[f"c{i}_y"] = np.array([c, ell, noise]), xb[:, 0], y[:, 0]
        out[f"c{i}_lml"] = np.array(float(np.asarray(val).reshape(-1)[0]))
        # value + gradient w.r.t. the log-parameters (GPI.py:1046-1051)
        val2, grad = gp.log_marginal_likelihood(torch.from_numpy(xb), torch.from_numpy(y), None, theta=k.theta, eval_gradient=True)
        assert abs(float(np.asarray(val2).reshape(-1)[0]) - float(out[f"c{i}_lml"])) < 1e-9 * abs(float(out[f"c{i}_lml"]))
        out[f"c{i}_grad"] = np.asarray(grad, dtype=np.float64).reshape(-1)
    out["n_cases"] = np.array(3)
    np.savez_compressed(os.path.join(OUT, "lml.npz"), **out)


# ---------------------------------------------------------------------------- a11
def gen_warp_prior():
    rng = np.random.default_rng(6)
    out = {}
    i = 0
    for (T, B, rho, omega, noise) in [(16, 5, 0.3, 1.0, 0.05), (45, 128, 0.2, 2.0, 0.01), (90, 33, 0.5, 0.7, 0.1)]:
        x = np.arange(float(T)) * 2.0
        wp = WarpPriorAMTGP(noise_warp=noise, bound_noise_warp=(1e-10, 1e10))
        wp.theta = (rho, omega)
        W = x[None, :] + rng.normal(size=(B, T)) * 0.3
        val = wp.log_sq_error_batch(torch.from_numpy(x), torch.from_numpy(W))
        one = wp.log_sq_error(torch.from_numpy(x), torch.from_numpy(W[0]))
        r, o = wp._parse_theta()
        out[f"c{i}_x"], out[f"c{i}_W"] = x, W
        out[f"c{i}_par"] = np.array([r, o, float(wp._clamped_noise("cpu", torch.float64)), wp.jitter, float(wp.normalize_x)])
        out[f"c{i}_val"], out[f"c{i}_one"] = npy(val), np.array(float(one))
        i += 1
    out["n_cases"] = np.array(i)
    np.savez_compressed(os.path.join(OUT, "warp_prior.npz"), **out)


# -------------------------------------------------- end-to-end: offline include_batch
def gen_offline(tag, rec, n, stride):
    data = load_beats(rec, n, stride)
    N, T, _ = data.shape
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic",
                     ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std,
                     ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                     bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False, method_compute_warp="greedy",
                     verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                     inducing_points=False, reestimate_initial_params=True, n_explore_steps=5, free_deg_MNIV=5)
    sw.include_batch(x_trains, data, warp=False)
    xt, yt = torch.from_numpy(x_trains), torch.from_numpy(data)
    models = [g for g in sw.gpmodels[0] if len(g.indexes) > 0]
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "M": np.array(len(models)),
           "resp_assigned": npy(sw.resp_assigned[-1]).astype(np.int64)}
    qs = []
    for m, g in enumerate(models):
        q = g.compute_sq_err_all(xt, yt)
        qs.append(npy(q))
        # per-step observation state actually read by compute_sq_err_all: mean_i = C_i f_i , Sigma_i
        S = len(g.f_star)
        means = np.stack([npy(torch.matmul(g.C[min(i, len(g.C) - 1)], g.f_star[i])).reshape(-1) for i in range(S)])
        out[f"m{m}_means"] = means
        out[f"m{m}_Sigma"] = np.stack([npy(s) for s in g.Sigma])
        out[f"m{m}_indexes"] = np.array(g.indexes, dtype=np.int64)
        out[f"m{m}_theta"] = kernel_theta(g.gp.kernel)
        out[f"m{m}_q_lat"] = npy(g.compute_q_lat_all(xt))
        # what a fresh model needs to replay this cluster's final pass: initial LDS parameters and MNIW prior
        out[f"m{m}_Gamma0"], out[f"m{m}_A0"], out[f"m{m}_C0"] = npy(g.Gamma[0]), npy(g.A[0]), npy(g.C[0])
        out[f"m{m}_Gamma_last"], out[f"m{m}_A_last"] = npy(g.Gamma[-1]), npy(g.A[-1])
        out[f"m{m}_f_star_sm_last"] = npy(g.f_star_sm[-1]).reshape(-1)
        out[f"m{m}_n0"] = np.array(float(g.internal_params.n0))
        out[f"m{m}_free_deg"] = np.array(float(g.free_deg_MNIV))
    out["q"] = np.stack(qs, axis=1)
    np.savez_compressed(os.path.join(OUT, f"offline_{tag}.npz"), **out)
    # forward / backward messages and pair responsibilities of the switching variable on the run's final
    # variational observations q (GPI_HDP.py:3546-3700), full recursion (no cached prefix)
    rec = {}
    of, ob, oc = sw.forward, sw.backward, sw.coupled_state_coef

    def f_(pi=None, trans_A=None, q=None):
        out_ = of(pi, trans_A, q)
        rec["f"] = (pi, q, out_)
        return out_

    def b_(trans_A=None, q=None, margprob=None):
        out_ = ob(trans_A, q, margprob)
        rec["b"] = out_
        return out_

    def c_(alpha=None, beta=None, trans_A=None, q=None, margprobs=None):
        out_ = oc(alpha, beta, trans_A, q, margprobs)
        rec["c"] = out_
        return out_

    sw.forward, sw.backward, sw.coupled_state_coef = f_, b_, c_
    keep = sw.fmsg, sw.margPrObs
    sw.fmsg = None
    sw.variational_local_terms(sw.q[-1])        # the reference's own call sequence (GPI_HDP.py:586-628)
    sw.fmsg, sw.margPrObs = keep
    sw.forward, sw.backward, sw.coupled_state_coef = of, ob, oc
    pi_in, q_in, (fmsg, marg) = rec["f"]
    K = q_in.shape[1]
    hm = {"q": npy(q_in), "log_pi": npy(sw.compute_trans_pi(K, pi_in)), "log_trans": npy(sw.compute_trans_A(K)),
          "fmsg": npy(fmsg), "margPrObs": npy(marg), "bmsg": npy(rec["b"]), "log_respPair": npy(rec["c"])}
    np.savez_compressed(os.path.join(OUT, f"hmm_{tag}.npz"), **hm)
    print(f"hmm_{tag}: q{hm['q'].shape} log_trans{hm['log_trans'].shape}")
    print(f"offline_{tag}: N={N} T={T} M={len(models)} counts={[len(g.indexes) for g in models]}")



# ------------------------------------- drop-in surface: reload_model_from_labels + cluster_new_batch (record 102)
def gen_reload(tag, rec, n=None, leads=(0,)):
    """What hdpgpc/tests/test_offline_multi_output_load.py:74-85 does, on lead 0 with theta injected: rebuild the model from
    the record's annotation labels (one full_pass_weighted per class), then classify the same batch with the frozen
    models (cluster_new_batch, learning=False: M x N log_sq_error(i=-1) calls -> LogLik -> forward / backward ->
    one-hot arg-max)."""
    data = np.load(os.path.join(REF, "data", "mitbih", f"{rec}.npy"))[:, :, list(leads)]
    labels = np.load(os.path.join(REF, "data", "mitbih", f"{rec}_labels.npy"))
    D = len(leads)                # D = 2 is the driver as written (both leads; SNR-weighted combination of the leads)
    if n is not None:
        data, labels = data[:n], labels[:n]
    data = np.ascontiguousarray(data)
    N, T, _ = data.shape
    labels = labels[:N]
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(data)
    sigma, gamma = std * 1.0, std * 1.1
    noise_warp = std * 0.1
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                     bound_lengthscale=(1.0, 20.0), ini_gamma=gamma, ini_sigma=sigma, ini_outputscale=300.0,
                     noise_warp=noise_warp, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                     bound_noise_warp=(noise_warp * 0.1, noise_warp * 0.2), warp_updating=False, method_compute_warp="greedy",
                     verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                     inducing_points=False, reestimate_initial_params=True, n_explore_steps=20, free_deg_MNIV=5)
    labels_trans = {'N': 1, 'V': 2, 'R': 3, '!': 4, 'F': 5, 'L': 6, 'A': 7, '/': 8, 'Q': 9, 'f': 10, 'E': 11, 'J': 12, 'j': 13,
                    'e': 14, 'a': 15, 'S': 16}
    labels_num = [labels_trans[l] - 1 for l in labels]
    vals = np.unique(labels_num)
    M = vals.shape[0]
    lab = np.array([np.where(vals == l)[0] for l in labels_num]).squeeze()
    sw.reload_model_from_labels(x_trains, data, lab, M)
    new_labels = sw.cluster_new_batch(x_trains, data)
    first = (lambda a: a[..., 0]) if D == 1 else (lambda a: a)      # the one-lead fixture keeps its round-2 layout
    ref_sens = None
    if D > 1:
        # how sharply are the REFERENCE's numbers defined?  Its own run on inputs perturbed by 1e-15 relative (below one ulp):
        # the per-(lead, class) change of its scores is the yardstick the parity test uses for the ill-conditioned lead
        sw2 = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                          bound_lengthscale=(1.0, 20.0), ini_gamma=gamma, ini_sigma=sigma, ini_outputscale=300.0,
                          noise_warp=noise_warp, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                          bound_noise_warp=(noise_warp * 0.1, noise_warp * 0.2), warp_updating=False, method_compute_warp="greedy",
                          verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                          inducing_points=False, reestimate_initial_params=True, n_explore_steps=20, free_deg_MNIV=5)
        data_p = data * (1.0 + 1e-15 * np.random.default_rng(0).standard_normal(data.shape))
        sw2.reload_model_from_labels(x_trains, data_p, lab, M)
        qa, qb = npy(sw.q_last), npy(sw2.q_last)
        la, lb = npy(sw.q_lat_last), npy(sw2.q_lat_last)
        with np.errstate(invalid="ignore", divide="ignore"):
            ref_sens = np.maximum(np.max(np.abs(qb - qa) / np.abs(qa), axis=0),
                                  np.nanmax(np.where(la != 0, np.abs(lb - la) / np.abs(la), 0.0), axis=0))    # [M, D]
        print("reference sensitivity to a 1e-15 input perturbation [class, lead]:\n", ref_sens)
    out = {"y": first(data), "x_basis": xb[:, 0], "labels": lab.astype(np.int64), "M": np.array(M),
           "estimators": np.array([std, std_dif, bound_sigma[0], bound_sigma[1], bound_gamma[0], bound_gamma[1]]),
           "sigma": np.array(sigma), "gamma": np.array(gamma), "theta_inject": np.array(THETA_INJECT),
           "new_labels": npy(new_labels).astype(np.int64), "transTheta": npy(sw.transTheta), "startTheta": npy(sw.startTheta),
           "rho": npy(sw.rho), "omega": npy(sw.omega), "q_last": first(npy(sw.q_last)), "q_lat_last": first(npy(sw.q_lat_last)),
           "resp_assigned": npy(sw.resp_assigned[-1]).astype(np.int64)}
    # the q matrix cluster_new_batch scored (frozen last states, i = -1) for diagnostics of the arg-max margin
    xt, yt = torch.from_numpy(x_trains), torch.from_numpy(data)
    qn = np.zeros((N, M, D))
    for ld in range(D):
        for m in range(M):
            g = sw.gpmodels[ld][m]
            qn[:, m, ld] = [float(g.log_sq_error(xt[i], yt[i][:, [ld]], i=-1)) for i in range(N)]
            if ld == 0:
                out[f"m{m}_theta"] = kernel_theta(g.gp.kernel)
                out[f"m{m}_n_members"] = np.array(len(g.indexes))
    out["q_new"] = first(qn)
    if ref_sens is not None:
        out["ref_sens"] = ref_sens
    np.savez_compressed(os.path.join(OUT, f"reload_{tag}.npz"), **out)
    print(f"reload_{tag}: N={N} M={M} counts={[len(g.indexes) for g in sw.gpmodels[0]]} "
          f"changed labels={int(np.sum(out['new_labels'] != lab))}")


# ------------------------------------------------ online-side producer pieces on a real state (GPI_model.py:561-593,726-745)
def gen_producer_extra():
    """posterior_weighted / smoother_weighted (what GPI_HDP.estimate_new calls, GPI_HDP.py:2830-2841) on the state of the
    t45 fixture: shared grid and irregular grid (the K_cov path of GPI.posterior, GPI.py:124-133,144-146), h = 1 and h < 1;
    then reinit_LDS / reinit_GP and a second pass over other members."""
    rng = np.random.default_rng(31)
    data = load_beats("102", 24, 2)
    members = [0, 1, 2, 3, 4, 7, 8, 11, 15, 16, 20]
    gm, x_trains, y_trains, q, q_lat = build_model(data, members)
    n, T, _ = data.shape
    x_irr = np.arange(float(T))[:, None] + rng.uniform(-0.3, 0.3, (T, 1))
    out = {"x_irr": x_irr[:, 0], "y_new": data[21, :, 0]}
    for tag, xx in (("shared", npy(x_trains[21])), ("irr", x_irr)):
        for h in (1.0, 0.6):
            f, c = gm.posterior_weighted(torch.from_numpy(xx), y_trains[21], h)
            out[f"pw_{tag}_h{h}_f"], out[f"pw_{tag}_h{h}_cov"] = npy(f)[:, 0], npy(c)
        f, c = gm.posterior_weighted(torch.from_numpy(xx), y_trains[21], 1.0, t=3)
        out[f"pw_{tag}_t3_f"], out[f"pw_{tag}_t3_cov"] = npy(f)[:, 0], npy(c)
    means, covs, C, Sigma = gm.smoother_weighted(x_trains[21], y_trains[21], 1.0)
    out["sw_len"] = np.array([len(means), len(covs), len(C), len(Sigma)])
    out["sw_last_f"], out["sw_last_cov"] = npy(means[-1])[:, 0], npy(covs[-1])
    # estimate_new's score: log_sq_error with the smoothed candidate as params, first=True (GPI_HDP.py:2835-2841)
    out["lse_candidate"] = np.array(float(gm.log_sq_error(x_trains[21], y_trains[21], mean=means[-1], cov=covs[-1], C=C[-1],
                                                          Sigma=Sigma[-1], i=0, first=True)))
    # re-initialise and run another member set through the SAME (fitted) model
    gm.reinit_LDS(save_last=False)
    gm.reinit_GP(save_last=False)
    out["re_N"], out["re_fitted"] = np.array(gm.N), np.array(int(gm.fitted))
    resp = torch.zeros(n)
    resp[[5, 6, 9, 10, 12]] = 1.0
    q2, ql2 = gm.full_pass_weighted(x_trains, y_trains, resp)
    out["re_q"], out["re_q_lat"] = npy(q2), npy(ql2)
    out["re_Sigma_last"], out["re_f_sm_last"] = npy(gm.Sigma[-1]), npy(gm.f_star_sm[-1])[:, 0]
    np.savez_compressed(os.path.join(OUT, "producer_extra.npz"), **out)
    print("producer_extra: done")


# ------------------------------------------------------------- 8f-4: batched monotone time-warp fit (WARP:548-735)
def gen_warp_batch():
    """Warping_system.compute_warp_batch: B independent warps fitted by Adam (torch autograd in the reference) - inputs, the
    warps, the warped observations, the prior scores and the per-iteration mean losses."""
    rng = np.random.default_rng(41)
    out = {}
    i = 0
    for (T, B, D, iters, theta, recursive) in [(90, 7, 1, 50, 1.2, False), (90, 5, 1, 250, (0.8, 1.5), False),
                                               (45, 4, 2, 60, None, True), (128, 3, 1, 40, 1.2, False)]:
        x = np.arange(float(T)) if T != 45 else np.arange(float(T)) * 2.0
        t = x / x[-1]
        base = np.stack([80 * np.exp(-0.5 * ((t - 0.45) / 0.05) ** 2) - 30 * np.exp(-0.5 * ((t - 0.6) / 0.08) ** 2) + 5 * d
                         for d in range(D)], axis=1)                                    # (T, D) cluster mean
        Yt = np.zeros((B, T, D))
        for b in range(B):
            shift = rng.uniform(-0.06, 0.06)
            tw = np.clip(t + shift * np.sin(np.pi * t), 0, 1)
            for d in range(D):
                Yt[b, :, d] = np.interp(tw, t, base[:, d]) + rng.normal(0, 1.0, T)
        noise = rng.uniform(1.0, 3.0, T)
        wgt = None if i != 2 else rng.uniform(0.2, 1.0, B)
        ws = Warping_system(x[:, None], noise_warp=0.5, bound_noise_warp=(0.05, 5.0), recursive=recursive, bayesian=True,
                            cuda=False, mode="rough")
        reps = 2 if recursive else 1                       # second call starts from the first call's mean control vector
        for rep in range(reps):
            xw, yw, lik, tr = ws.compute_warp_batch(torch.from_numpy(x), torch.from_numpy(Yt), torch.from_numpy(base), theta=theta,
                                                    noise=torch.from_numpy(noise), weights=None if wgt is None else torch.from_numpy(wgt),
                                                    train_iter=iters)
            out[f"c{i}_r{rep}_xw"], out[f"c{i}_r{rep}_yw"], out[f"c{i}_r{rep}_lik"] = npy(xw)[:, :, 0], npy(yw), npy(lik)
            out[f"c{i}_r{rep}_loss"] = np.array(tr["loss"])
        out[f"c{i}_x"], out[f"c{i}_Yt"], out[f"c{i}_Ym"], out[f"c{i}_noise"] = x, Yt, base, noise
        out[f"c{i}_theta"] = np.array([np.nan, np.nan]) if theta is None else np.atleast_1d(np.asarray(theta, dtype=np.float64))
        out[f"c{i}_meta"] = np.array([iters, int(recursive), reps, ws.n_ctrl, ws.lr, ws.lambda_smooth_base, ws.lambda_amp_base, 0.5, 0.05, 5.0])
        if wgt is not None:
            out[f"c{i}_w"] = wgt
        i += 1
    out["n_cases"] = np.array(i)
    np.savez_compressed(os.path.join(OUT, "warp_batch.npz"), **out)
    print(f"warp_batch: {i} cases")


# --------------------------------------------- configs[4]: the online path's calls at T = 256 (beats resampled)
def gen_online_t256():
    """BASELINE configs[4] runs the online path on beats resampled to T = 256.  What one online step asks of a cluster
    (GPI_HDP.py:1970-2197): compute_q_lat_all, log_sq_error(i=-1), return_LDS_param_likelihood, the candidate posterior
    (posterior_weighted / smoother_weighted) - on a state the reference builds itself from 6 members.  Only inputs and
    final outputs are stored (the mirror rebuilds the state from the beats)."""
    rng = np.random.default_rng(51)
    raw = load_beats("102", 10, 1)[..., 0]                                   # (10, 90)
    T = 256
    tt = np.linspace(0, raw.shape[1] - 1, T)
    data = np.stack([np.interp(tt, np.arange(raw.shape[1]), r) for r in raw])[:, :, None]
    members = [0, 1, 2, 4, 5, 7]
    gm, x_trains, y_trains, q, q_lat = build_model(np.ascontiguousarray(data), members)
    n = data.shape[0]
    x_irr = np.arange(float(T))[None, :, None] + rng.uniform(-0.3, 0.3, (n, T, 1))
    out = {"y": data[..., 0], "members": np.array(members), "theta": kernel_theta(gm.gp.kernel),
           "sigma0": npy(gm.Sigma[0])[0, 0], "gamma0": npy(gm.Gamma[0])[0, 0], "x_irr": x_irr[..., 0],
           "q_shared": npy(q), "q_lat": npy(q_lat), "lds_lik": np.array(float(gm.return_LDS_param_likelihood())),
           "lse_last_shared": np.array([float(gm.log_sq_error(x_trains[j], y_trains[j], i=-1)) for j in range(n)]),
           "lse_last_irr": np.array([float(gm.log_sq_error(torch.from_numpy(x_irr[j]), y_trains[j], i=-1)) for j in (8, 9)]),
           "Sigma_last_diag": np.diag(npy(gm.Sigma[-1])), "Sigma_last_row7": npy(gm.Sigma[-1])[7],
           "f_star_sm_last": npy(gm.f_star_sm[-1])[:, 0], "n0": np.array(float(gm.internal_params.n0))}
    f, c = gm.posterior_weighted(x_trains[8], y_trains[8], 1.0)
    out["pw_f"], out["pw_cov_diag"], out["pw_cov_row100"] = npy(f)[:, 0], np.diag(npy(c)), npy(c)[100]
    means, covs, C, Sigma = gm.smoother_weighted(x_trains[8], y_trains[8], 1.0)
    out["lse_candidate"] = np.array(float(gm.log_sq_error(x_trains[8], y_trains[8], mean=means[-1], cov=covs[-1], C=C[-1],
                                                          Sigma=Sigma[-1], i=0, first=True)))
    np.savez_compressed(os.path.join(OUT, "online_t256.npz"), **out)
    print("online_t256: done", out["q_shared"][:3])


def _trace_loop(sw, run):
    """Run `run()` with GPI_HDP.compute_q_elbo / estimate_q_all / variational_local_terms_batch and GPI_model.full_pass_weighted
    wrapped; returns (order, elbo, qall, fpw, em, wall seconds, exception or None)."""
    import time
    order = []                       # event kinds in call order: 0 elbo, 1 estimate_q_all, 2 full_pass_weighted, 3 EM iteration
    elbo, qall, fpw, em = [], [], [], []
    o_elbo, o_qall, o_vltb = sw.compute_q_elbo, sw.estimate_q_all, sw.variational_local_terms_batch
    o_fpw = GM.GPI_model.full_pass_weighted
    lab = lambda r: npy(torch.argmax(r, dim=1)).astype(np.int16)   # noqa: E731

    def w_elbo(resp, respPair, q, q_lat, gpmodels, M, *a, **k):
        out_ = o_elbo(resp, respPair, q, q_lat, gpmodels, M, *a, **k)
        order.append(0)
        elbo.append((npy(torch.sum(resp, dim=0)), float(out_[0]), float(out_[1]), float(bool(k.get("post", False)))))
        return out_

    def w_qall(M, **k):
        out_ = o_qall(M, **k)
        order.append(1)
        qall.append(lab(out_[0]))
        return out_

    def w_fpw(self, x_trains_, y_trains_, resp, q=None, q_lat=None, snr=None):
        out_ = o_fpw(self, x_trains_, y_trains_, resp, q=q, q_lat=q_lat, snr=snr)
        order.append(2)
        mem = npy(torch.nonzero(resp > 0.99).reshape(-1))
        fpw.append((float(len(mem)), float(mem[0]) if len(mem) else -1.0, float(mem[-1]) if len(mem) else -1.0,
                    float(torch.sum(out_[0])) if out_[0] is not None else 0.0,
                    float(torch.sum(out_[1])) if out_[1] is not None else 0.0))
        return out_

    def w_vltb(*a, **k):
        out_ = o_vltb(*a, **k)
        order.append(3)
        em.append((lab(out_[0]), npy(out_[2]).copy(), npy(out_[3]).copy(), bool(out_[6])))
        return out_

    sw.compute_q_elbo, sw.estimate_q_all, sw.variational_local_terms_batch = w_elbo, w_qall, w_vltb
    GM.GPI_model.full_pass_weighted = w_fpw
    t0 = time.time()
    err = None
    try:
        run()
    except NameError as e:           # GPI_HDP.py:3139 reads an undefined name at the loop's stop condition (cluster_new_batch)
        err = e
    finally:
        GM.GPI_model.full_pass_weighted = o_fpw
        sw.compute_q_elbo, sw.estimate_q_all, sw.variational_local_terms_batch = o_elbo, o_qall, o_vltb
    return order, elbo, qall, fpw, em, time.time() - t0, err


def _pack_trace(out, N, order, elbo, qall, fpw, em):
    Mmax = max(len(e[0]) for e in elbo)
    counts = np.full((len(elbo), Mmax), -1.0)
    for i, e in enumerate(elbo):
        counts[i, :len(e[0])] = e[0]
    out.update({"order": np.array(order, dtype=np.int8), "elbo_counts": counts, "elbo_vals": np.array([e[1:] for e in elbo]),
                "qall_labels": np.stack(qall) if qall else np.zeros((0, N), np.int16), "fpw": np.array(fpw), "n_em": np.array(len(em))})
    for i, (l_, q_, ql_, re_) in enumerate(em):
        out[f"em{i}_labels"], out[f"em{i}_q"], out[f"em{i}_q_lat"], out[f"em{i}_reallocate"] = l_, q_, ql_, np.array(re_)


# ------------------------------------- SURVEY 8b Face 1: the offline variational loop, GPI_HDP.include_batch
def gen_include_batch(tag, rec, n=None, lead=0, n_explore=5, leads=None, warp=False):
    """Run the reference's include_batch exactly as hdpgpc/tests/test_offline.py:32-79 drives it (kernel fit replaced by the
    theta injection above) and record a TRACE of what the loop decided and computed: every ELBO evaluation
    (GPI_HDP.compute_q_elbo), every assignment returned by estimate_q_all, every full_pass_weighted, and per EM
    iteration (variational_local_terms_batch) the assignments and the q / q_lat matrices.  Data only."""
    leads = [lead] if leads is None else list(leads)       # several leads: hdpgpc/tests/test_offline_multi_output.py
    data = np.ascontiguousarray(np.load(os.path.join(REF, "data", "mitbih", f"{rec}.npy"))[:n, :, leads])
    N, T, D = data.shape
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic",
                     ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std,
                     ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                     bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False, method_compute_warp="greedy",
                     verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                     inducing_points=False, reestimate_initial_params=True, n_explore_steps=n_explore, free_deg_MNIV=5)
    order, elbo, qall, fpw, em, wall, _ = _trace_loop(sw, lambda: sw.include_batch(x_trains, data, warp=warp))
    out = {"y": data[..., 0] if D == 1 else data, "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]),
           "theta_inject": np.array(THETA_INJECT), "n_explore": np.array(n_explore), "wall_s": np.array(wall), "warp": np.array(warp),
           "M_final": np.array(sw.M), "train_elbo": np.array([float(e) for e in sw.train_elbo]),
           "resp_assigned": np.stack([npy(r).astype(np.int16) for r in sw.resp_assigned]),
           "f_ind_old": npy(sw.f_ind_old).astype(np.int64), "transTheta": npy(sw.transTheta), "startTheta": npy(sw.startTheta),
           "rho": npy(sw.rho), "omega": npy(sw.omega), "sigma_def": np.array(float(sw.ini_sigma_def)),
           "gamma_def": np.array(float(sw.ini_gamma_def)),
           "counts_final": np.array([len(g.indexes) for g in sw.gpmodels[0]], dtype=np.int64)}
    _pack_trace(out, N, order, elbo, qall, fpw, em)
    if D > 1:
        # the reference's own sensitivity (lead 1 of record 102 is ill-conditioned): the same run on inputs perturbed by 1e-15
        data_p = data * (1.0 + 1e-15 * np.random.default_rng(0).standard_normal(data.shape))
        sw2 = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic",
                          ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std,
                          ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                          bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False, method_compute_warp="greedy",
                          verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                          inducing_points=False, reestimate_initial_params=True, n_explore_steps=n_explore, free_deg_MNIV=5)
        o2, e2, qa2, f2, em2, _, _ = _trace_loop(sw2, lambda: sw2.include_batch(x_trains, data_p, warp=False))
        rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(np.asarray(b)))), 1e-300))  # noqa: E731
        same = o2 == order and all(np.array_equal(a, b) for a, b in zip(qa2, qall))
        out["ref_pert_same_decisions"] = np.array(same)
        if same:
            out["ref_sens"] = np.array(max([rel(a[1:3], b[1:3]) for a, b in zip(e2, elbo)] + [rel(a[3:], b[3:]) for a, b in zip(f2, fpw)] +
                                           [max(rel(a[1], b[1]), rel(a[2], b[2])) for a, b in zip(em2, em)]))
            print("reference sensitivity of the traced numbers to a 1e-15 input perturbation:", float(out["ref_sens"]))
    if n is None or n > 500:          # the full record's beats are their own fixture (mitbih<rec>_lead0.npz)
        del out["y"]
        beats = os.path.join(OUT, f"mitbih{rec}_lead{lead}.npz")
        if D == 1 and not os.path.exists(beats):
            np.savez_compressed(beats, y=data[..., 0], labels=np.load(os.path.join(REF, "data", "mitbih", f"{rec}_labels.npy")))
    np.savez_compressed(os.path.join(OUT, f"include_batch_{tag}.npz"), **out)
    print(f"include_batch_{tag}: N={N} wall={wall:.1f}s EM iterations={len(em)} M={sw.M} counts={out['counts_final']} "
          f"events={len(order)} elbo={out['train_elbo']}")



# ------------------------------------- SURVEY 8b Face 1 / configs[4]: the online step, GPI_HDP.include_sample
def gen_include_sample(tag, rec, n, T_res=None, lead=0, with_warp=False, off_grid=None):
    """Run the reference's online loop as hdpgpc/tests/test_online.py:41-83 drives it (n_f = 30, free_deg_MNIV = 20, warp
    off, theta injected) on the first n beats of a record - optionally resampled to T_res points by linear interpolation
    (BASELINE configs[4] names T = 256) - and record after every beat what the step decided and scored.
    off_grid = (beat indices, shift): those beats are handed over on the grid x_basis + shift (key x_shift[n]: the per-beat
    shift), so they leave the shared-grid short cut of pred_dist (GPI.py:467-468); such a trace also records the reference's
    own sensitivity (ref_sens, ref_sens_row[n]: the same run on inputs perturbed by 1e-15 relative)."""
    import time
    if isinstance(rec, (list, tuple)):     # BASELINE configs[4] "concatenated MIT-BIH records": n beats of each record, one after the other
        raw = np.concatenate([np.load(os.path.join(REF, "data", "mitbih", f"{r}.npy"))[:n, :, [lead]] for r in rec])
        n = raw.shape[0]
    else:
        raw = np.load(os.path.join(REF, "data", "mitbih", f"{rec}.npy"))[:, :, [lead]]
    if T_res is not None:
        tt = np.linspace(0, raw.shape[1] - 1, T_res)
        raw = np.stack([np.interp(tt, np.arange(raw.shape[1]), r[:, 0]) for r in raw[:max(n, 32)]])[:, :, None]
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(raw, 30)
    data = np.ascontiguousarray(raw[:n])
    T = data.shape[1]
    xb = np.arange(float(T))[:, None]
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                     bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                     bound_sigma=bound_sigma, bound_gamma=bound_gamma, bound_noise_warp=(std * 0.01, std * 0.02),
                     warp_updating=bool(with_warp), method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100,
                     mode_warp="rough", bayesian_params=True, inducing_points=False, estimation_limit=None, free_deg_MNIV=20)
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]),
           "theta_inject": np.array(THETA_INJECT), "with_warp": np.array(bool(with_warp))}
    x_shift = np.zeros(n)
    if off_grid is not None:
        x_shift[sorted(off_grid[0])] = float(off_grid[1])
        out["x_shift"] = x_shift
    states, Ms, secs = [], [], []
    for i in range(n):
        t0 = time.time()
        sw.include_sample(xb + x_shift[i], data[i], with_warp=bool(with_warp))   # hdpgpc/tests/test_online_warp.py:82 passes True
        secs.append(time.time() - t0)
        if with_warp:   # what compute_warp_y returned for this beat: liks [M + 1], the warps and the warped beat per cluster
            out[f"b{i}_liks"] = np.asarray(npy(sw.liks[-1]) if torch.is_tensor(sw.liks[-1]) else sw.liks[-1], dtype=np.float64)
            out[f"b{i}_xw"] = np.stack([npy(v).reshape(-1) for v in sw.x_w[-1]])
            out[f"b{i}_yw"] = np.stack([npy(v).reshape(-1) for v in sw.y_w[-1]])
        states.append(sw.actual_state)
        Ms.append(sw.M)
        out[f"b{i}_labels"] = npy(sw.resp_assigned[-1]).astype(np.int16)
        out[f"b{i}_q"] = npy(sw.q[-1]).copy()
        out[f"b{i}_counts"] = np.array([len(g.indexes) for g in sw.gpmodels[0]], dtype=np.int64)
    out["state"], out["M"], out["secs"] = np.array(states), np.array(Ms), np.array(secs)
    out["transTheta"], out["startTheta"], out["rho"], out["omega"] = npy(sw.transTheta), npy(sw.startTheta), npy(sw.rho), npy(sw.omega)
    if off_grid is not None:
        # how sharply are the REFERENCE's scores defined?  Its own run on inputs perturbed by 1e-15 relative (below one ulp)
        data_p = data * (1.0 + 1e-15 * np.random.default_rng(0).standard_normal(data.shape))
        sw2 = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                          bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                          bound_sigma=bound_sigma, bound_gamma=bound_gamma, bound_noise_warp=(std * 0.01, std * 0.02),
                          warp_updating=False, method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100,
                          mode_warp="rough", bayesian_params=True, inducing_points=False, estimation_limit=None, free_deg_MNIV=20)
        same, row = True, np.zeros(n)
        for i in range(n):
            sw2.include_sample(xb + x_shift[i], data_p[i], with_warp=False)
            q0, q1 = out[f"b{i}_q"], npy(sw2.q[-1])
            same = same and sw2.actual_state == states[i] and sw2.M == Ms[i] and q1.shape == q0.shape and \
                np.array_equal(npy(sw2.resp_assigned[-1]).astype(np.int16), out[f"b{i}_labels"])
            if not same:
                break
            fin = np.isfinite(q0)
            d = np.where(fin, np.abs(q1 - np.where(fin, q0, 0.0)) / np.maximum(np.abs(np.where(fin, q0, 1.0)), 1e-300), 0.0)
            row[:i + 1] = np.maximum(row[:i + 1], d.reshape(i + 1, -1).max(axis=1))
        out["ref_pert_same_decisions"] = np.array(same)
        if same:
            out["ref_sens"], out["ref_sens_row"] = np.array(row.max()), row
            print("reference sensitivity of the score matrices to a 1e-15 input perturbation:", row.max(), "per row:", row)
    np.savez_compressed(os.path.join(OUT, f"include_sample_{tag}.npz"), **out)
    print(f"include_sample_{tag}: n={n} T={T} states={states} M={Ms[-1]} total {sum(secs):.1f}s last beat {secs[-1]:.2f}s")


# ------------------------------------- cluster_new_batch(learning=True): the EM loop re-entered with new segments
def gen_cluster_learning(tag, rec, n0, n1, leads=(0, 1), n_explore=5):
    """As hdpgpc/tests/test_offline_multi_output_load.py:81-85 (both leads): rebuild the cluster models of the first n0 beats
    from the annotation labels, then cluster_new_batch(the next n1 beats, learning=True).  The reference's loop ends in a
    NameError (GPI_HDP.py:3139, `warp_computed`) after its last assignment; the state at that point is what is recorded."""
    data = np.load(os.path.join(REF, "data", "mitbih", f"{rec}.npy"))[:n0 + n1, :, list(leads)]
    labels = np.load(os.path.join(REF, "data", "mitbih", f"{rec}_labels.npy"))[:n0]
    N, T, D = data.shape
    std, std_dif, bound_sigma, bound_gamma = compute_estimators_LDS(data, n_f=50)
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                     bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                     bound_sigma=bound_sigma, bound_gamma=bound_gamma, bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                     method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100, mode_warp="rough",
                     bayesian_params=True, inducing_points=False, reestimate_initial_params=True, n_explore_steps=n_explore,
                     free_deg_MNIV=5)
    sw.warp = False                      # include_batch sets it; cluster_new_batch reads it through the proposals
    vals = np.unique(labels)
    lab = np.array([int(np.where(vals == l_)[0][0]) for l_ in labels])
    sw.reload_model_from_labels(x_trains[:n0], data[:n0], lab, len(vals))
    order, elbo, qall, fpw, em, wall, err = _trace_loop(
        sw, lambda: sw.cluster_new_batch(x_trains[n0:], data[n0:], learning=True))
    out = {"y": data, "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]), "labels": lab,
           "n0": np.array(n0), "M0": np.array(len(vals)), "theta_inject": np.array(THETA_INJECT), "n_explore": np.array(n_explore),
           "wall_s": np.array(wall), "ended_in_nameerror": np.array(err is not None), "M_final": np.array(sw.M),
           "train_elbo": np.array([float(e) for e in sw.train_elbo]),
           "resp_last": npy(torch.argmax(sw.resp_assigned[-1].reshape(N, -1), dim=1) if sw.resp_assigned[-1].dim() > 1
                            else sw.resp_assigned[-1]).astype(np.int16),
           "counts_final": np.array([[len(g.indexes) for g in sw.gpmodels[ld]] for ld in range(D)], dtype=np.int64),
           "q_last": npy(sw.q_last), "q_lat_last": npy(sw.q_lat_last)}
    _pack_trace(out, N, order, elbo, qall, fpw, em)
    # the reference's own sensitivity: the same run on inputs perturbed by 1e-15 relative (below one ulp)
    data_p = data * (1.0 + 1e-15 * np.random.default_rng(0).standard_normal(data.shape))
    sw2 = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                      bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                      bound_sigma=bound_sigma, bound_gamma=bound_gamma, bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                      method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100, mode_warp="rough",
                      bayesian_params=True, inducing_points=False, reestimate_initial_params=True, n_explore_steps=n_explore,
                      free_deg_MNIV=5)
    sw2.warp = False
    sw2.reload_model_from_labels(x_trains[:n0], data_p[:n0], lab, len(vals))
    o2, e2, qa2, f2, em2, _, _ = _trace_loop(sw2, lambda: sw2.cluster_new_batch(x_trains[n0:], data_p[n0:], learning=True))
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(float(np.max(np.abs(np.asarray(b)))), 1e-300))  # noqa: E731
    same = o2 == order and all(np.array_equal(a, b) for a, b in zip(qa2, qall))
    out["ref_pert_same_decisions"] = np.array(same)
    if same:
        sens = max([rel(a[1:3], b[1:3]) for a, b in zip(e2, elbo)] + [rel(a[3:], b[3:]) for a, b in zip(f2, fpw)] +
                   [max(rel(a[1], b[1]), rel(a[2], b[2])) for a, b in zip(em2, em)])
        out["ref_sens"] = np.array(sens)
        print("reference sensitivity of the traced numbers to a 1e-15 input perturbation:", sens)
    np.savez_compressed(os.path.join(OUT, f"cluster_learning_{tag}.npz"), **out)
    print(f"cluster_learning_{tag}: N={N} D={D} wall={wall:.1f}s EM iterations={len(em)} M={sw.M} counts={out['counts_final'].tolist()} "
          f"events={len(order)} err={err}")


# ------------------------------------- the gpytorch fit - the only numbers the reference HOLDS for it
def gen_kernel_fit_notebook():
    """gpytorch is absent here, so the fit cannot be run; but hdpgpc/tests/test_step.ipynb stores the printed output of four
    fits of the reference's own run (loss every 500 iterations to 3 decimals, the four raw gpytorch parameters after the 4000th
    step to 8+ digits).  This copies those NUMBERS (and which beat each fit saw) into a fixture: data, not code."""
    import json
    import re
    nb = json.load(open(os.path.join(REF, "tests", "test_step.ipynb")))
    fits = []
    for i, c in enumerate(nb["cells"]):
        if c["cell_type"] != "code":
            continue
        txt = "".join("".join(o.get("text") or o.get("data", {}).get("text/plain") or []) for o in c.get("outputs", []))
        for m in re.finditer(r"(?:Sample: (\d+) /[^\n]*\n(?:[^\n]*\n){0,3})?\s*Fitting_GP:(.*?)raw_lengthscale\s+value = \[\[([-\d.e]+)\]\]", txt, re.S):
            blk = m.group(2)
            losses = re.findall(r"Iter (\d+)/4000 - Loss: ([\d.]+)", blk)
            vals = re.findall(r"value = \[?([-\d.e]+)", blk)
            fits.append((i, m.group(1), [int(a) for a, _ in losses], [float(b) for _, b in losses], [float(v) for v in vals] + [float(m.group(3))]))
    assert [f[0] for f in fits] == [22, 26, 33, 36], fits
    fits = fits[:3]
    # cell 4: data = record 100 [1700:1950]; cells 22 / 26 / 33 fit data_[0], data_[5], data_[206] (lead 0) with the white-kernel
    # bounds (std 0.1, std 0.2), std = compute_estimators_LDS(data, n_f = 50) (cell 8 prints 11.558797835735662).  Cell 36 (the
    # first fit inside include_batch with reestimate_initial_params) is left out: no beat of the record reproduces its first loss
    # (472.718) under the bounds today's redefine_default would set - the notebook ran an older revision of that re-estimation
    data = np.load(os.path.join(REF, "data", "mitbih", "100.npy"))
    # (the number the NOTEBOOK printed in cell 8: today's compute_estimators_LDS returns another estimate for the same beats)
    cell8 = "".join("".join(o.get("text") or []) for o in nb["cells"][8].get("outputs", []))
    std = float(re.search(r"Sigma estimated: ([\d.]+)", cell8).group(1))
    out = {"beats": np.array([1700, 1705, 1906]), "iters": np.array(fits[0][2]),
           "losses": np.array([f[3] for f in fits]), "raw_final": np.array([f[4] for f in fits]),   # raw noise, mean, raw outputscale, raw lengthscale
           "std_cell8": np.array(float(std)), "y": np.stack([data[b, :, 0] for b in (1700, 1705, 1906)])}
    np.savez_compressed(os.path.join(OUT, "kernel_fit_notebook.npz"), **out)
    print("kernel_fit_notebook:", out["losses"][:, [0, -1]], out["raw_final"], float(std))


if __name__ == "__main__":
    which = sys.argv[1:] or ["gram", "score", "pred", "ill", "state", "lml", "warp", "offline"]
    if "gram" in which:
        gen_gram()
    if "score" in which:
        gen_score_shared()
    if "pred" in which:
        gen_pred_dist()
    if "ill" in which:
        gen_pairs_ill()
    if "state" in which:
        gen_state("t30", "100", 14, 3, [2, 5, 6, 9, 12], 11)
        gen_state("t45", "102", 24, 2, [0, 1, 2, 3, 4, 7, 8, 11, 15, 16, 20], 12)
        gen_state("t90", "100", 8, 1, [0, 1, 3, 6], 13)
    if "state_l3" in which or "state" in which:
        gen_state("t45l3", "102", 24, 2, [0, 1, 2, 3, 4, 7, 8, 11, 15, 16, 20], 12, theta=(341.0, 3.0, 4.66))
    if "lml" in which:
        gen_lml()
    if "warp" in which:
        gen_warp_prior()
    if "offline" in which:
        gen_offline("r102_t45", "102", 60, 2)
    if "online256" in which:
        gen_online_t256()
    if "warpbatch" in which:
        gen_warp_batch()
    if "extra" in which:
        gen_producer_extra()
    if "ib80" in which:
        gen_include_batch("r100_n80", "100", 80)
    if "ibw" in which:
        gen_include_batch("r100_n80_warp", "100", 80, warp=True)
    if "ib2" in which:
        gen_include_batch("r102_2leads_n100", "102", 100, leads=(0, 1), n_explore=5)
    if "ib100" in which:
        gen_include_batch("r100", "100", None)
    if "ib102" in which:              # BASELINE configs[2]: the whole of record 102 (hdpgpc/tests/test_offline.py:32-79)
        gen_include_batch("r102", "102", None)
    if "learn" in which:
        gen_cluster_learning("r102_2leads", "102", 300, 20)
    if "online90" in which:
        gen_include_sample("r102_n40", "102", 40)
    if "onlinew" in which:
        gen_include_sample("r102_n25_warp", "102", 25, with_warp=True)
    if "online256" in which and "trace" in which:
        gen_include_sample("r102_t256_n24", "102", 24, T_res=256)
    if "online256x2" in which:         # configs[4]: two records concatenated (16 beats of record 100, then 16 of record 102), T = 256
        gen_include_sample("r100_r102_t256_n32", ["100", "102"], 16, T_res=256)
    if "onlinemix" in which:           # beats on and off the basis grid in one run: the per-pair scores and the one-by-one commit
        gen_include_sample("r102_n37_mixedgrid", "102", 37, off_grid=({5, 19, 20, 21, 29, 30, 31, 34}, 0.3))
    if "fitnb" in which:
        gen_kernel_fit_notebook()
    if "reload" in which:
        gen_reload("r102", "102")
    if "reload2" in which:
        gen_reload("r102_2leads", "102", n=700, leads=(0, 1))
    print("done")
