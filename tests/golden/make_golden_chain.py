#!/usr/bin/env python3
"""Golden vectors of the element-wise tail of one member step, written by RUNNING THE REFERENCE: the inputs and outputs of
matrix_normal_inv_wishart.posterior (GPI_model.py:1300-1344) and the rows GPI_model.bayesian_new_params appends
(GPI_model.py:1076-1106), recorded while the reference's own full_pass_weighted runs on the t30 configuration.

Build-container only, like make_golden.py, whose reference import, stand-ins and model builder it reuses.

Usage (from the repo root):   python tests/golden/make_golden_chain.py
Writes tests/golden/chain_step_t30.npz - data only.

Steps N = 2 (right covariances still the identity) and N = 3 (dense right covariances) are stored.  Per step sN_ and
distribution d (0 = internal, 1 = observation):
  sN_dD_old_m_mean / old_m_r_cov / old_n0 / old_scale   the distribution posterior() was called on
  sN_dD_y1 / y2                                          its samples
  sN_dD_S__ / part_mean / jitter                         intermediates, recomputed in the wrapper with the calls of
                                                         GPI_model.py:1313-1330; main() asserts that the recomputed part_mean
                                                         gives the returned mean bit for bit
  sN_dD_new_m_mean / new_m_r_cov / new_n0 / new_scale    what posterior() returned
  sN_N, sN_Gamma0, sN_Sigma0, sN_A_last, sN_Gamma_last, sN_C_last, sN_Sigma_last    after bayesian_new_params.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

STEPS = (2, 3)
MEMBERS = [2, 5, 6, 9, 12]


def intermediates(dist, y1, y2, cov_, cov_cross):
    """S__, part_mean and the jitter of posterior() with sse_matrix = None (the shared grid), call for call."""
    T = dist.scale.shape[0]
    eye = torch.eye(T, device=dist.scale.device, dtype=dist.scale.dtype)
    R = 0.5 * (dist.m_r_cov + dist.m_r_cov.T)
    jitter = 1e-2 * torch.mean(torch.diag(dist.scale).abs()).clamp_min(torch.finfo(dist.scale.dtype).eps)
    R_inv = torch.cholesky_solve(eye, torch.linalg.cholesky(R + jitter * eye))
    y2p, y1p = eye @ y2, eye @ y1
    S__ = (y2p @ y2p.T + eye @ cov_ @ eye.T) + R_inv
    S_ = (y1p @ y2p.T + eye @ cov_cross @ eye.T) + dist.m_mean @ R_inv
    L = torch.linalg.cholesky(0.5 * (S__ + S__.T) + 1e-8 * eye)
    return S__, torch.cholesky_solve(S_.T, L).T, jitter


def main():
    MNIW, Model = mg.GM.matrix_normal_inv_wishart, mg.GM.GPI_model
    o_post, o_bnp = MNIW.posterior, Model.bayesian_new_params
    calls, steps = [], []

    def w_post(self, n_k, y1, y2, cov, cov_, cov_cross, sse_matrix=None, annealing=False):
        assert n_k == 1 and sse_matrix is None
        rec = {"old_m_mean": self.m_mean.clone(), "old_m_r_cov": self.m_r_cov.clone(), "old_n0": float(self.n0),
               "old_scale": self.scale.clone(), "y1": y1.clone(), "y2": y2.clone()}
        rec["S__"], rec["part_mean"], rec["jitter"] = intermediates(self, y1, y2, cov_, cov_cross)
        new = o_post(self, n_k, y1, y2, cov, cov_, cov_cross, sse_matrix=sse_matrix, annealing=annealing)
        n0 = rec["old_n0"]
        assert torch.equal(((n0 - 2) * rec["old_m_mean"] + rec["part_mean"]) / (n0 - 1), new.m_mean)
        assert torch.equal(rec["S__"], new.m_r_cov)
        rec.update(new_m_mean=new.m_mean, new_m_r_cov=new.m_r_cov, new_n0=float(new.n0), new_scale=new.scale)
        calls.append(rec)
        return new

    def w_bnp(self, h, *a, **k):
        first = len(calls)
        r = o_bnp(self, h, *a, **k)
        steps.append({"N": float(self.N), "posterior": calls[first:], "Gamma0": self.Gamma[0], "Sigma0": self.Sigma[0],
                      "A_last": self.A[-1], "Gamma_last": self.Gamma[-1], "C_last": self.C[-1], "Sigma_last": self.Sigma[-1]})
        return r

    MNIW.posterior, Model.bayesian_new_params = w_post, w_bnp
    try:
        mg.build_model(mg.load_beats("100", 14, 3), MEMBERS)
    finally:
        MNIW.posterior, Model.bayesian_new_params = o_post, o_bnp
    assert len(calls) == 8 and [s["N"] for s in steps] == [1.0, 2.0, 3.0, 4.0, 5.0], (len(calls), [s["N"] for s in steps])
    out = {}
    for st in steps:
        if int(st["N"]) not in STEPS:
            continue
        p = f"s{int(st['N'])}_"
        assert len(st["posterior"]) == 2
        for d, rec in enumerate(st["posterior"]):
            for k, v in rec.items():
                out[f"{p}d{d}_{k}"] = mg.npy(v).astype(np.float64)
        for k in ("N", "Gamma0", "Sigma0", "A_last", "Gamma_last", "C_last", "Sigma_last"):
            out[p + k] = mg.npy(st[k]).astype(np.float64)
    T = out["s2_Gamma0"].shape[0]
    assert np.array_equal(out["s2_d0_old_m_r_cov"], np.eye(T)) and np.array_equal(out["s2_d1_old_m_r_cov"], np.eye(T))
    assert np.count_nonzero(out["s3_d0_old_m_r_cov"]) == T * T
    path = os.path.join(mg.OUT, "chain_step_t30.npz")
    np.savez_compressed(path, **out)
    print(f"chain_step_t30: T={T}, {len(calls)} posterior calls, steps {STEPS} stored, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
