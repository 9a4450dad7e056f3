#!/usr/bin/env python3
"""Golden vectors of the projection onto the basis grid, written by RUNNING THE REFERENCE
(IterativeGaussianProcess.project_y, GPI.py:194-238).

Build-container only, like make_golden.py, whose reference import and stand-ins it reuses.

Usage (from the repo root):   python tests/golden/make_golden_project.py
Writes tests/golden/project_y.npz - data only, a few KB.

Cases (c = 300, two leads, length-scales 1.2 and 3.0 each):
  T = 90 with L = 60 / 75 points over the same span, L = 90 shifted by 0.3, and L = 90 on the basis itself (the torch.equal
  short-circuit); T = 30 with L = 45 (more points than the basis) - that one also with a C that is not the identity.
The values are smooth beat-like curves (two Gaussian bumps on a slow sine), not white noise: what the operator is for.
Also printed: how far tests/project_ref.py's NumPy restatement sits from the reference's own numbers.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import make_golden as mg  # noqa: E402
import project_ref  # noqa: E402

C_OUT = 300.0
ELLS = (1.2, 3.0)
CASES = [(90, 60, 0.0), (90, 75, 0.0), (90, 90, 0.3), (90, 90, 0.0), (30, 45, 0.0)]    # T, L, shift


def curves(x, T):
    """[L, 2]: beat-like values on the grid x of a segment that spans [0, T - 1]."""
    u = np.asarray(x, dtype=np.float64) / (T - 1.0)
    a = 180.0 * np.exp(-0.5 * ((u - 0.45) / 0.03) ** 2) - 40.0 * np.exp(-0.5 * ((u - 0.52) / 0.02) ** 2) + 25.0 * np.sin(2 * np.pi * u)
    b = -90.0 * np.exp(-0.5 * ((u - 0.40) / 0.05) ** 2) + 30.0 * np.exp(-0.5 * ((u - 0.70) / 0.08) ** 2) + 10.0 * np.cos(3 * np.pi * u)
    return np.stack([a, b], axis=1)


def grid(T, L, shift):
    return np.arange(T, dtype=np.float64) + shift if L == T else np.linspace(0.0, T - 1.0, L)


def main():
    out, worst = {}, 0.0
    k = 0
    for ell in ELLS:
        for T, L, shift in CASES:
            xb = np.arange(T, dtype=np.float64)[:, None]
            x = grid(T, L, shift)[:, None]
            y = curves(x[:, 0], T)
            gp = mg.GPI.IterativeGaussianProcess(mg.make_kernel(C_OUT, ell, 1.0), torch.from_numpy(xb), cuda=False, verbose=False)
            Cs = [np.eye(T)]
            if T == 30:
                Cs.append(np.eye(T) + 0.05 * np.diag(np.ones(T - 1), 1) - 0.02 * np.diag(np.ones(T - 2), -2))
            for C in Cs:
                Sigma = 2.0 * np.eye(T)
                y_p, S_p = gp.project_y(torch.from_numpy(x), torch.from_numpy(y), None, torch.from_numpy(C), torch.from_numpy(Sigma),
                                        x_basis=torch.from_numpy(xb))
                y_p = mg.npy(y_p)
                assert np.array_equal(mg.npy(S_p), Sigma)
                mine, _ = project_ref.project_y_ref(x[:, 0], y, C, Sigma, xb[:, 0], C_OUT, ell)
                worst = max(worst, project_ref.rel_err(mine, y_p))
                p = f"c{k}_"
                out[p + "theta"] = np.array([C_OUT, ell])
                out[p + "xb"], out[p + "x"], out[p + "y"], out[p + "yp"] = xb[:, 0], x[:, 0], y, y_p
                if not np.array_equal(C, np.eye(T)):
                    out[p + "C"] = C
                k += 1
    out["n_cases"] = np.array(k)
    out["restatement_err"] = np.array(worst)
    path = os.path.join(mg.OUT, "project_y.npz")
    np.savez_compressed(path, **out)
    print(f"project_y: {k} cases, restatement within {worst:.3e} of the reference, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
