#!/usr/bin/env python3
"""Golden vectors of the symmetric-KL distance between cluster states, written by RUNNING THE REFERENCE
(GPI_model.KL_divergence, GPI_model.py:899-931, and the double loop of util_plots.plot_MDS, util_plots.py:600-616).

Build-container only, like make_golden.py, whose reference import, stand-ins and model builder it reuses.

Usage (from the repo root):   python tests/golden/make_golden_kl.py
Writes tests/golden/kl_states.npz - data only.

Three clusters built by the reference's own full_pass_weighted on MIT-BIH beats:
  L_  record 102, every second sample (T = 45), a long cluster of 62 members of which only the LAST 8 states are stored (the
      tail of every stack; state t of the stored model is state L_offset + t of the cluster): its late consecutive states are
      nearly identical - the trace term of a consecutive pair is within 1 % of 2T, which main() asserts;
  S_  the same beats, a short second cluster of the same lead (the partner of L_ in the plot_MDS matrix);
  H_  record 100 at full resolution (T = 90), a few members (pairs within the cluster only: another grid).
Member counts are what a committed file of under 1 MiB holds with four [S,T,T] stacks per cluster.  A is not stored and Gamma
only as its last row (KL_divergence reads Gamma[-1] alone, to tell a static from a dynamic model).  Pairs across clusters exist
at equal T only (L x S); there is no L x H block.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_golden as mg  # noqa: E402
import kl_ref  # noqa: E402

import copy  # noqa: E402

N45, STRIDE45 = 64, 2
S_MEMBERS = [3, 60]
L_MEMBERS = [i for i in range(N45) if i not in S_MEMBERS]
L_TAIL = 8                                      # states of the long cluster that are stored
NEAR = 1e-2                                     # largest |trace term / 2T - 1| of a consecutive pair of stored L states
N90, H_MEMBERS = 8, [0, 3]


def tail_view(gm, k):
    """The reference's model restricted to its last k states: every per-step list cut to its tail, so that state t of the view is
    state len(indexes) - k + t of the model and the reference's own KL_divergence runs on it unchanged."""
    v = copy.copy(gm)
    v.indexes = list(gm.indexes[-k:])
    for name in ("f_star", "f_star_sm", "cov_f", "cov_f_sm", "C", "Sigma", "A", "Gamma"):
        setattr(v, name, list(getattr(gm, name)[-(k + 1):]))
    return v


def dump(gm, prefix, out):
    out[prefix + "theta"] = mg.kernel_theta(gm.gp.kernel)
    out[prefix + "x_basis"] = mg.npy(gm.x_basis)[:, 0]
    out[prefix + "indexes"] = np.array(gm.indexes, dtype=np.int64)
    for name in ("f_star", "f_star_sm"):
        out[prefix + name] = np.stack([mg.npy(f).reshape(-1) for f in getattr(gm, name)])
    for name in ("cov_f", "cov_f_sm", "C", "Sigma"):
        out[prefix + name] = np.stack([mg.npy(m) for m in getattr(gm, name)])
    out[prefix + "Gamma_last"] = mg.npy(gm.Gamma[-1])


def moments(gm, t, smoothed, x_bas=None):
    """The Gaussian the reference hands to IterativeGaussianProcess.KL_divergence for state t (GPI_model.py:902-930)."""
    f, P = (gm.f_star_sm, gm.cov_f_sm) if smoothed else (gm.f_star, gm.cov_f)
    f, P = f[t + 1], P[t + 1]
    tc = -1 if gm.estimation_limit <= t else t
    if x_bas is not None and not torch.equal(x_bas, gm.x_basis):
        m, c = gm.observe(x_bas, tc, params=[f, P, gm.C[tc], gm.Sigma[tc]])
    else:
        m = torch.matmul(gm.C[tc], f)
        c = torch.linalg.multi_dot([gm.C[tc], P, gm.C[tc].T]) + gm.Sigma[tc]
    return mg.npy(m).reshape(-1), mg.npy(c)


def block(g1, g2, smoothed, x_bas=None, ts1=None, ts2=None, sens=None):
    ts1 = range(len(g1.indexes)) if ts1 is None else ts1
    ts2 = range(len(g2.indexes)) if ts2 is None else ts2
    out = np.zeros((len(ts1), len(ts2)))
    for a, t in enumerate(ts1):
        for b, u in enumerate(ts2):
            v = g1.KL_divergence(t, g2, u, smoothed=smoothed, x_bas=x_bas)
            out[a, b] = v
            if sens is not None:
                w = kl_ref.kl_pair(*moments(g1, t, smoothed, x_bas), *moments(g2, u, smoothed, x_bas), order="chol")
                sens.append(abs(v - w) / max(abs(v), 1.0))
    return out


def main():
    out, sens = {}, []
    d45 = mg.load_beats("102", N45, STRIDE45)
    gL_full = mg.build_model(d45, L_MEMBERS)[0]
    gL = tail_view(gL_full, L_TAIL)
    out["L_offset"] = np.array(len(gL_full.indexes) - L_TAIL)
    for t in range(L_TAIL):          # the view reads what the full model reads
        assert gL.KL_divergence(t, gL, 0, smoothed=False) == gL_full.KL_divergence(int(out["L_offset"]) + t, gL_full,
                                                                                      int(out["L_offset"]), smoothed=False)
    exc = []
    for sm in (False, True):
        for t in range(L_TAIL - 1):
            (m1, c1), (m2, c2) = moments(gL, t, sm), moments(gL, t + 1, sm)
            exc.append(np.trace(np.linalg.inv(c2) @ c1 + np.linalg.inv(c1) @ c2) / (2 * len(m1)) - 1.0)
    out["L_trace_excess"] = np.array(exc)
    assert 0.0 < max(exc) < NEAR, exc
    gS = mg.build_model(d45, S_MEMBERS)[0]
    gH = mg.build_model(mg.load_beats("100", N90, 1), H_MEMBERS)[0]
    for g, p in ((gL, "L_"), (gS, "S_"), (gH, "H_")):
        assert len(g.Gamma) > 0 and not bool(torch.all(g.Gamma[-1] == 0))
        dump(g, p, out)
    for sm, tag in ((False, "f"), (True, "s")):
        out["kl_LL_" + tag] = block(gL, gL, sm, sens=sens)
        out["kl_LS_" + tag] = block(gL, gS, sm, sens=sens)
        out["kl_SL_" + tag] = block(gS, gL, sm, sens=sens)
        out["kl_SS_" + tag] = block(gS, gS, sm, sens=sens)
        out["kl_HH_" + tag] = block(gH, gH, sm, sens=sens)
    # another grid: half-sample spacing (the grid util_plots.py:755-758 draws on)
    xb = torch.from_numpy(np.arange(0.0, d45.shape[1] - 1 + 1e-9, 0.5)[:, None])
    out["xbas"] = mg.npy(xb)[:, 0]
    out["xbas_tL"] = np.array([0, 3, len(gL.indexes) - 2, len(gL.indexes) - 1], dtype=np.int64)
    out["xbas_tS"] = np.array([0, len(gS.indexes) - 1], dtype=np.int64)
    out["kl_LS_xbas_f"] = block(gL, gS, False, xb, list(out["xbas_tL"]), list(out["xbas_tS"]), sens=sens)
    out["kl_LL_xbas_f"] = block(gL, gL, False, xb, list(out["xbas_tL"]), list(out["xbas_tL"]), sens=sens)
    # the loop of util_plots.plot_MDS (util_plots.py:600-616) over the lead's two clusters
    n_seg = d45.shape[0]
    x_bas = gL.x_basis
    KL = np.zeros((n_seg, n_seg))
    for gp1 in (gL, gS):
        for i, ind1 in enumerate(gp1.indexes):
            for gp2 in (gL, gS):
                for j, ind2 in enumerate(gp2.indexes):
                    if ind1 < ind2:
                        KL[ind1, ind2] = gp1.KL_divergence(i, gp2, j, smoothed=False, x_bas=x_bas)
    for i in range(n_seg):
        for j in range(i, n_seg):
            KL[j, i] = KL[i, j]
    out["plot_mds"] = KL
    out["n_seg"] = np.array(n_seg)
    out["ref_sens"] = np.array(max(sens))
    path = os.path.join(mg.OUT, "kl_states.npz")
    np.savez_compressed(path, **out)
    print(f"late L trace excess {min(exc):.2e} .. {max(exc):.2e}")
    print(f"kl_states: L {len(gL.indexes)} S {len(gS.indexes)} H {len(gH.indexes)} members, ref_sens {max(sens):.3e}, "
          f"{os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
