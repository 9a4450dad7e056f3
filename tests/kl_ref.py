"""NumPy restatement of the symmetric Kullback-Leibler distance between Gaussians (reference: GPI.py:1058-1094),

    KL(i, j) = 1/4 (tr(cov_j^-1 cov_i) + tr(cov_i^-1 cov_j) - 2T) + 1/4 d^T (cov_i^-1 + cov_j^-1) d,   d = m_i - m_j,

in two evaluation orders, so that a test can take its tolerance from the formula's own sensitivity to the order of the
operations rather than from the code under test:

  order="inv":  the reference's order - np.linalg.inv (LU), the matrix products, their trace;
  order="chol": inverses through the Cholesky factor, the traces as Frobenius inner products <cov_j^-1, cov_i>.

A test helper (like kernel_fit_ref.py), not part of the product.
"""
import numpy as np


def kl_pair(m1, c1, m2, c2, order="inv"):
    """One pair, exactly the reference's sequence of operations for order="inv"."""
    m1, m2 = np.asarray(m1, np.float64).reshape(-1), np.asarray(m2, np.float64).reshape(-1)
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    T = c1.shape[0]
    if order == "inv":
        i1, i2 = np.linalg.inv(c1), np.linalg.inv(c2)
        tr = (np.trace(i2 @ c1 + i1 @ c2) - 2 * T) / 4
    else:
        i1, i2 = chol_inv(c1), chol_inv(c2)
        tr = ((np.sum(i2 * c1) + np.sum(i1 * c2)) - 2 * T) / 4
    d = m1 - m2
    return float(np.sum(((i1 + i2) @ d) * d) / 4 + tr)


def chol_inv(c):
    """c^-1 = Z^T Z, Z = chol(c)^-1 (batched over leading axes)."""
    L = np.linalg.cholesky(c)
    Z = np.linalg.solve(L, np.broadcast_to(np.eye(c.shape[-1]), c.shape))
    return np.swapaxes(Z, -1, -2) @ Z


def kl_matrix(mA, cA, mB=None, cB=None, order="chol"):
    """All pairs [nA, nB] (B omitted: A against itself).  The traces are taken as inner products over the flat T^2 axis in
    both orders (the matrix products of 90 000 pairs are out of reach on the host); what differs is the inversion."""
    mA, cA = np.asarray(mA, np.float64), np.asarray(cA, np.float64)
    nA, T = cA.shape[0], cA.shape[-1]
    mA = mA.reshape(nA, T)
    if cB is None:
        mB, cB = mA, cA
    mB, cB = np.asarray(mB, np.float64).reshape(-1, T), np.asarray(cB, np.float64)
    nB = cB.shape[0]
    inv = np.linalg.inv if order == "inv" else chol_inv
    pA, pB = inv(cA), inv(cB)
    if order == "inv":   # the reference multiplies inv(cov_j) cov_i: entry (a, a) of the product pairs row a with column a
        pAf, pBf = np.swapaxes(pA, 1, 2).reshape(nA, -1), np.swapaxes(pB, 1, 2).reshape(nB, -1)
    else:
        pAf, pBf = pA.reshape(nA, -1), pB.reshape(nB, -1)
    tr = cA.reshape(nA, -1) @ pBf.T + pAf @ cB.reshape(nB, -1).T
    out = (tr - 2 * T) / 4
    for i in range(nA):
        D = mA[i][None, :] - mB                                   # [nB, T]
        out[i] += (np.einsum("jt,jt->j", D @ pA[i], D) + np.einsum("jt,jt->j", (D[:, None, :] @ pB)[:, 0, :], D)) / 4
    return out


def state_moments(st, t, smoothed, x_bas=None, estimation_limit=np.inf):
    """The Gaussian GPI_model.KL_divergence compares for state t of a dynamic model (GPI_model.py:902-930) from the stacks
    `st` (a mapping with f_star, f_star_sm, cov_f, cov_f_sm, C, Sigma, x_basis, theta): f[t+1], P[t+1] with C[t], Sigma[t];
    on another grid the reference goes through observe(x_bas, t, params=...), i.e. pred_dist of (C f, Sigma)."""
    f = (st["f_star_sm"] if smoothed else st["f_star"])[t + 1]
    P = (st["cov_f_sm"] if smoothed else st["cov_f"])[t + 1]
    tc = -1 if estimation_limit <= t else t
    C, S = st["C"][tc], st["Sigma"][tc]
    if x_bas is not None and not np.array_equal(np.asarray(x_bas).reshape(-1), st["x_basis"].reshape(-1)):
        from oracle import hdpgpc_oracle as orc
        m, c = orc.pred_dist(x_bas, st["x_basis"], C @ f, S, tuple(st["theta"]))
        return m.reshape(-1), c
    return C @ f, C @ P @ C.T + S


def cluster(z, prefix):
    """One cluster's stacks of tests/golden/kl_states.npz."""
    names = ("theta", "x_basis", "indexes", "f_star", "f_star_sm", "cov_f", "cov_f_sm", "C", "Sigma", "Gamma_last")
    return {n: z[prefix + n] for n in names}


def golden_blocks(z):
    """(name, cluster prefix 1, cluster prefix 2, smoothed, x_bas, states 1, states 2) of every recorded block."""
    out = []
    for tag, sm in (("f", False), ("s", True)):
        for a, b in (("L", "L"), ("L", "S"), ("S", "L"), ("S", "S"), ("H", "H")):
            out.append((f"kl_{a}{b}_{tag}", a + "_", b + "_", sm, None, None, None))
    out.append(("kl_LS_xbas_f", "L_", "S_", False, z["xbas"], list(z["xbas_tL"]), list(z["xbas_tS"])))
    out.append(("kl_LL_xbas_f", "L_", "L_", False, z["xbas"], list(z["xbas_tL"]), list(z["xbas_tL"])))
    return out
