"""Shared by the CPU and GPU tests of ``model_type='static'``: the mirror set up from the fixtures of
tests/golden/make_golden_static.py and driven as offline_trace.py drives it; the comparisons are that helper's own
(compare_trace: every event of the trace, the same gates)."""
import numpy as np
import torch

from offline_trace import traced


def driver(g, D, model_type, M=None):
    import hdpgpc.GPI_HDP as hdpgp

    std, std_dif, bs0, bs1, bg0, bg1 = (float(v) for v in g["estimators"])
    T = len(g["x_basis"])
    xb = np.arange(float(T))[:, None]
    sw = hdpgp.GPI_HDP(xb, M=M, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type=model_type, ini_lengthscale=3.0,
                       bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                       bound_sigma=(bs0, bs1), bound_gamma=(bg0, bg1), bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False,
                       method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100, mode_warp="rough",
                       bayesian_params=True, inducing_points=False, reestimate_initial_params=True,
                       n_explore_steps=int(g["n_explore"]), free_deg_MNIV=5)
    sw.fixed_theta = tuple(float(v) for v in g["theta_inject"])
    return sw, xb


def run_offline(g):
    """include_batch on the fixture's beats with model_type='static', traced."""
    data = np.asarray(g["y"], dtype=np.float64)[:, :, None]
    sw, xb = driver(g, 1, "static")
    x_trains = np.array([xb] * data.shape[0])
    return sw, traced(sw, lambda: sw.include_batch(x_trains, data, with_warp=False))


def static_lists_ok(sw):
    """Every cluster static: parameter lists of length 1, Gamma zero, state lists one longer than the members, and the smoothed
    lists equal to the filtered ones (a static model has no smoother)."""
    for lead in sw.gpmodels:
        for m in lead:
            if not (len(m.A) == len(m.Gamma) == len(m.C) == len(m.Sigma) == 1) or bool(torch.any(m.Gamma[-1] != 0)):
                return False
            n = len(m.f_star)
            if not (n == len(m.f_star_sm) == len(m.cov_f) == len(m.cov_f_sm)) or (len(m.indexes) and n != len(m.indexes) + 1):
                return False
            if not (torch.equal(m.f_star.stack(), m.f_star_sm.stack()) and torch.equal(m.cov_f.stack(), m.cov_f_sm.stack())):
                return False
    return True
