"""Shared by the CPU and GPU tests of ``estimation_limit``: the mirror set up from the fixtures of
tests/golden/make_golden_estlimit.py - their `estimation_limit` key included - and driven as online_trace.py / offline_trace.py
drive it; the comparisons are those helpers' own."""
import numpy as np

from offline_trace import traced
from online_trace import _beat


def online_mirror(g):
    import hdpgpc.GPI_HDP as hdpgp

    std, std_dif, bs0, bs1, bg0, bg1 = (float(v) for v in g["estimators"])
    data = np.asarray(g["y"], dtype=np.float64)[:, :, None]
    xb = np.arange(float(data.shape[1]))[:, None]
    sw = hdpgp.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                       bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                       bound_sigma=(bs0, bs1), bound_gamma=(bg0, bg1), bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                       method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100, mode_warp="rough",
                       bayesian_params=True, inducing_points=False, estimation_limit=int(g["estimation_limit"]), free_deg_MNIV=20)
    sw.fixed_theta = tuple(float(v) for v in g["theta_inject"])
    return sw, xb, data


def run_online(g, n=None, each=None):
    """The first n beats of the trace g; each(sw, i) (optional) is called after every beat."""
    sw, xb, data = online_mirror(g)
    tr = []
    for i in range(data.shape[0] if n is None else n):
        sw.include_sample(xb, data[i], with_warp=False)
        tr.append(_beat(sw))
        if each is not None:
            each(sw, i)
    return sw, tr


def offline_mirror(g):
    import hdpgpc.GPI_HDP as hdpgp

    std, std_dif, bs0, bs1, bg0, bg1 = (float(v) for v in g["estimators"])
    data = np.asarray(g["y"], dtype=np.float64)[:, :, None]
    N, T, D = data.shape
    xb = np.arange(float(T))[:, None]
    sw = hdpgp.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                       bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                       bound_sigma=(bs0, bs1), bound_gamma=(bg0, bg1), bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                       method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100, mode_warp="rough",
                       bayesian_params=True, inducing_points=False, estimation_limit=int(g["estimation_limit"]),
                       reestimate_initial_params=bool(g["reestimate_initial_params"]), n_explore_steps=int(g["n_explore"]),
                       free_deg_MNIV=5)
    sw.fixed_theta = tuple(float(v) for v in g["theta_inject"])
    return sw, np.array([xb] * N), data


def run_offline(g):
    sw, x_trains, data = offline_mirror(g)
    return sw, traced(sw, lambda: sw.include_batch(x_trains, data, with_warp=False))


def list_lengths_ok(sw):
    """Every cluster: state lists one longer than its members, parameter lists min(that, E)."""
    for lead in sw.gpmodels:
        for m in lead:
            n = len(m.f_star)
            if len(m.indexes) and not (n == len(m.f_star_sm) == len(m.cov_f) == len(m.cov_f_sm) == len(m.indexes) + 1):
                return False
            if not (len(m.A) == len(m.Gamma) == len(m.C) == len(m.Sigma) == min(n, m.estimation_limit)):
                return False
    return True
