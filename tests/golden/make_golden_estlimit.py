#!/usr/bin/env python3
"""Golden traces and vectors for ``estimation_limit`` (a cluster stops re-estimating its LDS parameters once it has that many
members, GPI_model.py:974,1092), written by RUNNING THE REFERENCE.

Build-container only, like make_golden.py, whose reference import, stand-ins and trace helpers it reuses; the constructor
calls are its own (they pass the limit).  Every generator asserts that its run really freezes something.

Usage (from the repo root):   python tests/golden/make_golden_estlimit.py [online] [offline] [step]
Writes, data only:
  include_sample_r102_n40_el4.npz   the online step on the first 40 beats of record 102 with estimation_limit = 4, in the format
                                    of make_golden.gen_include_sample.  Unscaled, this record spawns a cluster at almost every
                                    beat (27 clusters of at most 3 members, with or without a limit): the four estimators are
                                    multiplied by 100, and the SCALED values are what `estimators` holds.
  include_batch_r102_n100_el6.npz   include_batch on the first 100 beats with estimation_limit = 6 and
                                    reestimate_initial_params = False (the reference's redefine_default reads np.PINF, which
                                    numpy 2 no longer has), in the format of make_golden.gen_include_batch.
  chain_step_estlimit_t30.npz       one frozen member step at N' = E and at N' = E + 1 on the t30 configuration: per step sN_
                                    (N = N') the eight lists of the model before (sN_pre_<list>) and after (sN_post_<list>)
                                    include_weighted_sample + backwards_pair + bayesian_new_params, both distributions
                                    before and after (sN_pre_dD_<field>, sN_post_dD_<field>) and the observation sN_y.
"""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

HDP, npy = mg.HDP, mg.npy


def _online(xb, est, limit):
    std, std_dif, bs0, bs1, bg0, bg1 = est
    return HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, kernels=None, model_type="dynamic", ini_lengthscale=3.0,
                       bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1,
                       bound_sigma=(bs0, bs1), bound_gamma=(bg0, bg1), bound_noise_warp=(std * 0.01, std * 0.02),
                       warp_updating=False, method_compute_warp="greedy", verbose=False, hmm_switch=True, max_models=100,
                       mode_warp="rough", bayesian_params=True, inducing_points=False, estimation_limit=limit, free_deg_MNIV=20)


def gen_online(rec="102", n=40, E=4, scale=100.0):
    raw = np.load(os.path.join(mg.REF, "data", "mitbih", f"{rec}.npy"))[:, :, [0]]
    std, std_dif, bound_sigma, bound_gamma = mg.compute_estimators_LDS(raw, 30)
    est = np.array([std, std_dif, *bound_sigma, *bound_gamma], dtype=np.float64) * scale
    data = np.ascontiguousarray(raw[:n])
    xb = np.arange(float(data.shape[1]))[:, None]
    runs = {}
    for limit in (E, None):
        sw = _online(xb, est, limit)
        beats, secs = [], []
        for i in range(n):
            t0 = time.time()
            sw.include_sample(xb, data[i], with_warp=False)
            secs.append(time.time() - t0)
            beats.append((sw.actual_state, sw.M, npy(sw.resp_assigned[-1]).astype(np.int16), npy(sw.q[-1]).copy(),
                          np.array([len(g.indexes) for g in sw.gpmodels[0]], dtype=np.int64)))
        runs[limit] = (sw, beats, secs)
    sw, beats, secs = runs[E]
    counts = beats[-1][4]
    assert int(np.sum(counts > E)) >= 2, f"fewer than two clusters end above the limit: {counts}"
    first_full = next(i for i, b in enumerate(beats) if b[4].max() >= E)
    births = sum(1 for i in range(first_full + 1, n) if beats[i][1] > beats[i - 1][1])
    assert births >= 3, f"only {births} births after the first cluster reached the limit"
    for g in sw.gpmodels[0]:
        assert len(g.A) == min(len(g.f_star), E) and len(g.f_star) == len(g.indexes) + 1, (len(g.A), len(g.f_star))
    free = runs[None][1]
    differ = [i for i in range(n) if beats[i][0] != free[i][0] or beats[i][1] != free[i][1] or not np.array_equal(beats[i][2], free[i][2])]
    assert differ, "the decisions are those of the run without a limit: the limit is not exercised"
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "estimators": est, "theta_inject": np.array(mg.THETA_INJECT),
           "with_warp": np.array(False), "estimation_limit": np.array(E), "first_differs": np.array(differ[0])}
    for i, (state, M, labels, q, cnt) in enumerate(beats):
        out[f"b{i}_labels"], out[f"b{i}_q"], out[f"b{i}_counts"] = labels, q, cnt
    out["state"], out["M"], out["secs"] = np.array([b[0] for b in beats]), np.array([b[1] for b in beats]), np.array(secs)
    out["transTheta"], out["startTheta"], out["rho"], out["omega"] = npy(sw.transTheta), npy(sw.startTheta), npy(sw.rho), npy(sw.omega)
    path = os.path.join(mg.OUT, f"include_sample_r{rec}_n{n}_el{E}.npz")
    np.savez_compressed(path, **out)
    print(f"include_sample_r{rec}_n{n}_el{E}: M={beats[-1][1]} sizes={counts} births after the limit={births} "
          f"decisions differ from the unlimited run first at beat {differ[0]}; {sum(secs):.1f}s, {os.path.getsize(path)} bytes")


def gen_offline(rec="102", n=100, E=6, n_explore=5):
    data = np.ascontiguousarray(np.load(os.path.join(mg.REF, "data", "mitbih", f"{rec}.npy"))[:n, :, [0]])
    N, T, D = data.shape
    std, std_dif, bound_sigma, bound_gamma = mg.compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = HDP.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type="dynamic",
                     ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std,
                     ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                     bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False, method_compute_warp="greedy",
                     verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                     inducing_points=False, estimation_limit=E, reestimate_initial_params=False, n_explore_steps=n_explore,
                     free_deg_MNIV=5)
    order, elbo, qall, fpw, em, wall, err = mg._trace_loop(sw, lambda: sw.include_batch(x_trains, data, warp=False))
    assert err is None, err
    counts = np.array([len(g.indexes) for g in sw.gpmodels[0]], dtype=np.int64)
    assert np.any(counts > E) and np.any((counts > 0) & (counts < E)), f"both modes must occur in one run: sizes {counts}"
    for g in sw.gpmodels[0]:
        assert len(g.A) == min(len(g.f_star), E), (len(g.A), len(g.f_star))
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]),
           "theta_inject": np.array(mg.THETA_INJECT), "n_explore": np.array(n_explore), "wall_s": np.array(wall), "warp": np.array(False),
           "estimation_limit": np.array(E), "reestimate_initial_params": np.array(False),
           "M_final": np.array(sw.M), "train_elbo": np.array([float(e) for e in sw.train_elbo]),
           "resp_assigned": np.stack([npy(r).astype(np.int16) for r in sw.resp_assigned]),
           "f_ind_old": npy(sw.f_ind_old).astype(np.int64), "transTheta": npy(sw.transTheta), "startTheta": npy(sw.startTheta),
           "rho": npy(sw.rho), "omega": npy(sw.omega), "sigma_def": np.array(float(sw.ini_sigma_def)),
           "gamma_def": np.array(float(sw.ini_gamma_def)), "counts_final": counts}
    mg._pack_trace(out, N, order, elbo, qall, fpw, em)
    path = os.path.join(mg.OUT, f"include_batch_r{rec}_n{n}_el{E}.npz")
    np.savez_compressed(path, **out)
    print(f"include_batch_r{rec}_n{n}_el{E}: M={sw.M} sizes={counts} EM iterations={len(em)} events={len(order)} wall={wall:.1f}s "
          f"{os.path.getsize(path)} bytes")


LISTS = ("A", "Gamma", "C", "Sigma", "f_star", "f_star_sm", "cov_f", "cov_f_sm")
DIST = ("m_mean", "m_r_cov", "n0", "scale")


def gen_step(E=3, members=(2, 5, 6, 9, 12)):
    data = mg.load_beats("100", 14, 3)
    N, T, _ = data.shape
    std, std_dif, bound_sigma, bound_gamma = mg.compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    kern = mg.ConstantKernel(300.0, (300.0, 1500.0)) * mg.RBF(3.0, (1.0, 20.0)) + mg.WhiteKernel(bound_sigma[0], bound_sigma)
    gm = mg.GM.GPI_model(kern, xb, annealing=True, bayesian=True, estimation_limit=E, free_deg_MNIV=5, verbose=False)
    cond = gm.GPR_dynamic(std_dif, std)
    gm.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    x_t, y_t = torch.from_numpy(xb), torch.from_numpy(data)
    out = {"estimation_limit": np.array(E), "x_basis": xb[:, 0]}

    def snap(p):
        for name in LISTS:
            out[p + name] = np.stack([npy(v).astype(np.float64).reshape(T, -1) for v in getattr(gm, name)])
        for d, dist in enumerate((gm.internal_params, gm.observation_params)):
            for k in DIST:
                v = getattr(dist, k)
                out[f"{p}d{d}_{k}"] = np.eye(T) if v is None else np.asarray(npy(v), dtype=np.float64)

    stored = []
    for idx in members:
        Np = gm.N + 1
        keep = Np in (E, E + 1)
        if keep:
            snap(f"s{Np}_pre_")
            out[f"s{Np}_y"] = data[idx, :, 0].copy()
        gm.include_weighted_sample(idx, x_t, x_t, y_t[idx], 1.0)
        gm.backwards_pair(1.0)
        gm.bayesian_new_params(1.0)
        if keep:
            snap(f"s{Np}_post_")
            stored.append(Np)
            assert out[f"s{Np}_post_A"].shape[0] == out[f"s{Np}_pre_A"].shape[0] == E, "the parameter lists grew"
            assert out[f"s{Np}_post_f_star"].shape[0] == out[f"s{Np}_pre_f_star"].shape[0] + 1 == Np + 1
            for d in range(2):
                for k in DIST:
                    assert np.array_equal(out[f"s{Np}_pre_d{d}_{k}"], out[f"s{Np}_post_d{d}_{k}"]), "a distribution changed"
    assert stored == [E, E + 1], stored
    path = os.path.join(mg.OUT, "chain_step_estlimit_t30.npz")
    np.savez_compressed(path, **out)
    print(f"chain_step_estlimit_t30: T={T} E={E} steps {stored} stored, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["online", "offline", "step"]
    if "step" in which:
        gen_step()
    if "offline" in which:
        gen_offline()
    if "online" in which:
        gen_online()
