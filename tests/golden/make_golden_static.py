#!/usr/bin/env python3
"""Golden vectors and traces for STATIC cluster models (model_type='static': Gamma = 0, the template does not evolve), written by
RUNNING THE REFERENCE.

Build-container only, like make_golden.py, whose reference import, stand-ins, theta injection and trace helpers it reuses; the
constructor calls are its own (they pass the model type).

Usage (from the repo root):   python tests/golden/make_golden_static.py [chain] [offline] [reload]
Writes, data only:
  chain_static_t30.npz                  a static GPI_model (built as make_golden.build_model builds one, with GPR_static) after the
                                        reference's full_pass_weighted over 12 beats of record 102 at T = 30: the inputs, theta,
                                        A / C / Sigma[0], every row of f_star, cov_f, f_star_sm, cov_f_sm, the returned q and q_lat.
  include_batch_r102_n60_static.npz     the make_golden._trace_loop trace of include_batch on the first 60 beats of record 102,
                                        lead 0, model_type='static', otherwise the arguments of make_golden.gen_include_batch.
  reload_r102_n100_static_mixed.npz     reload_model_from_labels on the first 70 of the 100 beats 40 .. 139 (the first window of
                                        the record whose annotations hold three classes: paced 52, normal 12, fusion 6; the
                                        labels are the annotations, renumbered), then cluster_new_batch(learning=False) and
                                        cluster_new_batch(learning=True) on the other 30, with model_type alternating
                                        'static', 'dynamic', ... over the label classes: the labels, the q matrix of the reload, the
                                        labels the frozen models give and the trace of the learning call in the format of
                                        make_golden.gen_cluster_learning (the reference's loop ends in its NameError at
                                        GPI_HDP.py:3139 after the last assignment; the state at that point is recorded).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

HDP, npy = mg.HDP, mg.npy


def gen_chain(rec="102", n=12, stride=3):
    data = mg.load_beats(rec, n, stride)
    N, T, _ = data.shape
    std, std_dif, bound_sigma, bound_gamma = mg.compute_estimators_LDS(data)
    xb = np.arange(float(T))[:, None]
    kern = mg.ConstantKernel(300.0, (300.0, 1500.0)) * mg.RBF(3.0, (1.0, 20.0)) + mg.WhiteKernel(bound_sigma[0], bound_sigma)
    gm = mg.GM.GPI_model(kern, xb, annealing=True, bayesian=True, free_deg_MNIV=5, verbose=False)
    cond = gm.GPR_static(std)
    gm.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    x_trains, y_trains = torch.from_numpy(np.array([xb] * N)), torch.from_numpy(data)
    resp = torch.ones(N)
    q, q_lat = gm.full_pass_weighted(x_trains, y_trains, resp)
    assert len(gm.A) == len(gm.Gamma) == len(gm.C) == len(gm.Sigma) == 1 and len(gm.f_star) == N + 1
    assert float(torch.sum(torch.abs(q_lat))) == 0.0
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "sigma": np.array(float(std)), "noise_bounds": np.array(bound_sigma, dtype=np.float64),
           "theta": mg.kernel_theta(gm.gp.kernel), "theta_inject": np.array(mg.THETA_INJECT),
           "A0": npy(gm.A[0]), "C0": npy(gm.C[0]), "Sigma0": npy(gm.Sigma[0]), "Gamma0": npy(gm.Gamma[0]),
           "q": npy(q), "q_lat": npy(q_lat), "indexes": np.array(gm.indexes, dtype=np.int64)}
    for name in ("f_star", "f_star_sm"):
        out[name] = np.stack([npy(f).reshape(-1) for f in getattr(gm, name)])
    for name in ("cov_f", "cov_f_sm"):
        out[name] = np.stack([npy(m) for m in getattr(gm, name)])
    path = os.path.join(mg.OUT, "chain_static_t30.npz")
    np.savez_compressed(path, **out)
    print(f"chain_static_t30: T={T} members={N} sum q={float(torch.sum(q)):.6f} {os.path.getsize(path)} bytes")


def _driver(xb, D, est, model_type, n_explore, M=None):
    std, std_dif, bound_sigma, bound_gamma = est
    return HDP.GPI_HDP(xb, M=M, x_basis_warp=xb[::2], n_outputs=D, kernels=None, model_type=model_type,
                       ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif, ini_sigma=std,
                       ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=bound_sigma, bound_gamma=bound_gamma,
                       bound_noise_warp=(std * 0.01, std * 0.02), warp_updating=False, method_compute_warp="greedy",
                       verbose=False, hmm_switch=True, max_models=100, mode_warp="rough", bayesian_params=True,
                       inducing_points=False, reestimate_initial_params=True, n_explore_steps=n_explore, free_deg_MNIV=5)


def gen_offline(rec="102", n=60, n_explore=5):
    data = np.ascontiguousarray(np.load(os.path.join(mg.REF, "data", "mitbih", f"{rec}.npy"))[:n, :, [0]])
    N, T, D = data.shape
    est = mg.compute_estimators_LDS(data)
    std, std_dif, bound_sigma, bound_gamma = est
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    sw = _driver(xb, D, est, "static", n_explore)
    order, elbo, qall, fpw, em, wall, err = mg._trace_loop(sw, lambda: sw.include_batch(x_trains, data, warp=False))
    assert err is None, err
    counts = np.array([len(g.indexes) for g in sw.gpmodels[0]], dtype=np.int64)
    for g in sw.gpmodels[0]:
        assert len(g.A) == len(g.Gamma) == len(g.C) == len(g.Sigma) == 1 and not bool(torch.any(g.Gamma[-1] != 0))
    assert all(float(np.sum(np.abs(e[2]))) == 0.0 for e in em), "a static model has no latent score"
    out = {"y": data[..., 0], "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]),
           "theta_inject": np.array(mg.THETA_INJECT), "n_explore": np.array(n_explore), "wall_s": np.array(wall), "warp": np.array(False),
           "M_final": np.array(sw.M), "train_elbo": np.array([float(e) for e in sw.train_elbo]),
           "resp_assigned": np.stack([npy(r).astype(np.int16) for r in sw.resp_assigned]),
           "f_ind_old": npy(sw.f_ind_old).astype(np.int64), "transTheta": npy(sw.transTheta), "startTheta": npy(sw.startTheta),
           "rho": npy(sw.rho), "omega": npy(sw.omega), "sigma_def": np.array(float(sw.ini_sigma_def)),
           "gamma_def": np.array(float(sw.ini_gamma_def)), "counts_final": counts}
    mg._pack_trace(out, N, order, elbo, qall, fpw, em)
    path = os.path.join(mg.OUT, f"include_batch_r{rec}_n{n}_static.npz")
    np.savez_compressed(path, **out)
    print(f"include_batch_r{rec}_n{n}_static: M={sw.M} sizes={counts} EM iterations={len(em)} events={len(order)} wall={wall:.1f}s "
          f"Elbo_LDS last={elbo[-1][2]:.2f} {os.path.getsize(path)} bytes")


def gen_reload(rec="102", n=100, n0=70, start=40, n_explore=5):
    data = np.ascontiguousarray(np.load(os.path.join(mg.REF, "data", "mitbih", f"{rec}.npy"))[start:start + n, :, [0]])
    ann = np.load(os.path.join(mg.REF, "data", "mitbih", f"{rec}_labels.npy"))[start:start + n]
    classes, labels = np.unique(ann[:n0], return_inverse=True)
    M0 = len(classes)
    assert M0 >= 3, f"the label classes must alternate over both types: {classes}"
    N, T, D = data.shape
    est = mg.compute_estimators_LDS(data)
    std, std_dif, bound_sigma, bound_gamma = est
    xb = np.arange(float(T))[:, None]
    x_trains = np.array([xb] * N)
    types = [("static", "dynamic")[m % 2] for m in range(M0)]
    sw = _driver(xb, D, est, types, n_explore, M=M0)
    sw.warp = False                      # include_batch sets it; cluster_new_batch reads it through the proposals
    sw.reload_model_from_labels(x_trains[:n0], data[:n0], torch.from_numpy(labels.astype(np.int64)), M0)
    q_reload = npy(sw.q[-1]).copy()
    gamma_zero = np.array([not bool(torch.any(g.Gamma[-1] != 0)) for g in sw.gpmodels[0]])
    frozen = npy(sw.cluster_new_batch(x_trains[n0:], data[n0:], learning=False)).astype(np.int64)
    order, elbo, qall, fpw, em, wall, err = mg._trace_loop(sw, lambda: sw.cluster_new_batch(x_trains[n0:], data[n0:], learning=True))
    out = {"y": data, "x_basis": xb[:, 0], "estimators": np.array([std, std_dif, *bound_sigma, *bound_gamma]),
           "theta_inject": np.array(mg.THETA_INJECT), "n_explore": np.array(n_explore), "n0": np.array(n0), "M0": np.array(M0), "start": np.array(start),
           "labels": labels.astype(np.int64), "model_type": np.array(types), "gamma_zero_after_reload": gamma_zero,
           "q_reload": q_reload, "labels_frozen": frozen, "wall_s": np.array(wall), "ended_in_nameerror": np.array(err is not None),
           "M_final": np.array(sw.M), "train_elbo": np.array([float(e) for e in sw.train_elbo]),
           "counts_final": np.array([[len(g.indexes) for g in lead] for lead in sw.gpmodels], dtype=np.int64),
           "resp_last": npy(torch.argmax(sw.resp_assigned[-1].reshape(N, -1), dim=1) if sw.resp_assigned[-1].dim() > 1
                            else sw.resp_assigned[-1]).astype(np.int16),
           "q_last": npy(sw.q_last), "q_lat_last": npy(sw.q_lat_last)}
    mg._pack_trace(out, N, order, elbo, qall, fpw, em)
    path = os.path.join(mg.OUT, f"reload_r{rec}_n{n}_static_mixed.npz")
    np.savez_compressed(path, **out)
    print(f"reload_r{rec}_n{n}_static_mixed: M0={M0} types={types} gamma zero after reload={gamma_zero} frozen labels={np.bincount(frozen)} "
          f"M={sw.M} events={len(order)} wall={wall:.1f}s {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    which = sys.argv[1:] or ["chain", "offline", "reload"]
    if "chain" in which:
        gen_chain()
    if "offline" in which:
        gen_offline()
    if "reload" in which:
        gen_reload()
