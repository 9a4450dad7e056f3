"""The pair score (oracle.pred_dist / log_sq_error_state / chol_spd) and the plan's operators at 40 significant digits.

Pure Python on mpmath, no GPU imports.  Inputs are float64 arrays and are converted exactly; every constant of the formulas
(1e-4, 1e-6, 1e-8) is the double the float64 codes use.  What is evaluated is the mathematical expression, not an operation
order: K~ = K(xb, xb) + jitter I is inverted explicitly, which costs about log10 kappa(K~) <= 9 of the 40 digits.  The results
are the truth that tests/golden/mp_pairs_t*.npz record (tests/golden/make_golden_mp_pairs.py) and that
tests/test_gpu_pairs_truth.py and tests/test_mp_ref_host.py measure the kernels, the oracle and a NumPy restatement against."""
import mpmath as mp
import numpy as np

DPS = 40
EPS = 2.0 ** -52


def _mat(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix(a.reshape(a.shape[0], -1).tolist())


def _eye(n, s):
    return mp.diag([s] * n)


def gram(x, y, c, ell):
    """c exp(-((a - b) / ell)^2 / 2): exactly c on the diagonal of gram(x, x)."""
    c, ell = mp.mpf(float(c)), mp.mpf(float(ell))
    xs, ys = [mp.mpf(float(a)) for a in x], [mp.mpf(float(b)) for b in y]
    return mp.matrix([[c * mp.exp(-(((a - b) / ell) ** 2) / 2) for b in ys] for a in xs])


def _norm_inf(A):
    return max(mp.fsum(abs(A[i, j]) for j in range(A.cols)) for i in range(A.rows))


def _mean_abs_diag(A):
    return mp.fsum(abs(A[i, i]) for i in range(A.rows)) / A.rows


def cluster_ops(xb, mean, Sigma, theta, want_M=True, dps=DPS):
    """Per cluster: K~^-1, ||K~^-1||_inf, kappa_inf(K~), bound = eps (c ||K~^-1||_inf)^2, jitter, a' = c K~^-1 mean and
    M' = c^2 (K~^-1 Sigma_s K~^-1 - K~^-1), Sigma_s = (Sigma + Sigma^T) / 2.  Matrices stay mpmath; the scalars too."""
    with mp.workdps(dps):
        c, ell, noise = (float(t) for t in theta)
        T = len(xb)
        Sg = _mat(Sigma)
        dS = np.diag(np.asarray(Sigma, dtype=np.float64))
        mS = float(np.mean(dS))
        iso = bool(np.all(np.abs(dS - mS) <= 1e-8 + 1e-5 * abs(mS)))        # torch.isclose defaults: the iso branch
        jitter = mp.mpf(1e-4) * max(_mean_abs_diag(Sg), mp.mpf(EPS))
        Kt = gram(xb, xb, c, ell) + _eye(T, jitter)
        Kinv = mp.inverse(Kt)
        Kinv = (Kinv + Kinv.T) / 2
        nrm = _norm_inf(Kinv)
        Ss = (Sg + Sg.T) / 2
        out = dict(theta=(c, ell, noise), iso=iso, mS=mp.fsum(Sg[i, i] for i in range(T)) / T, jitter=jitter, Kinv=Kinv, Ss=Ss, norm=nrm, kappa=nrm * _norm_inf(Kt), bound=mp.mpf(EPS) * (mp.mpf(c) * nrm) ** 2,
                   ap=mp.mpf(c) * (Kinv * _mat(mean)), Mp=None)
        if want_M:
            out["Mp"] = mp.mpf(c) ** 2 * (Kinv * Ss * Kinv - Kinv)
        return out


def pair(x, y, xb, ops, first_noises=(0.0,), dps=DPS):
    """[(quad, logdet) for each first_noise] of segment (x, y) against the cluster of `ops`, as mpmath numbers."""
    with mp.workdps(dps):
        c, ell, noise = ops["theta"]
        m = len(x)
        Ks = gram(xb, x, c, ell)                                 # K*  [T, m]
        S = ops["Kinv"] * Ks                                      # K~^-1 K*
        f = Ks.T * (ops["ap"] / mp.mpf(c))                        # K*^T K~^-1 mean
        if ops["iso"]:
            cov_f = _eye(m, ops["mS"])
        else:
            Kss = gram(x, x, c, ell) + _eye(m, mp.mpf(noise))
            cov_f = Kss + S.T * (ops["Ss"] * S - Ks)              # K** - K*^T K~^-1 K* + K*^T K~^-1 Sigma K~^-1 K*
            cov_f = (cov_f + cov_f.T) / 2 + _eye(m, mp.mpf(1e-6))
        d = _mat(y) - f
        out = []
        for fn in first_noises:
            cov = cov_f + _eye(m, mp.mpf(float(fn))) if fn != 0.0 else cov_f
            cov = (cov + cov.T) / 2
            cov = cov + _eye(m, mp.mpf(1e-8) * max(_mean_abs_diag(cov), mp.mpf(EPS)))
            L = mp.cholesky(cov)
            z = _forward(L, d)
            out.append((mp.fsum(v * v for v in z), 2 * mp.fsum(mp.log(L[i, i]) for i in range(m))))
        return out


def _forward(L, d):
    z = []
    for i in range(L.rows):
        z.append((d[i] - mp.fsum(L[i, j] * z[j] for j in range(i))) / L[i, i])
    return z


def to_f64(A):
    """mpmath matrix (or list of mpmath numbers) -> float64 array, each entry rounded to nearest."""
    if isinstance(A, mp.matrix):
        return np.array([[float(A[i, j]) for j in range(A.cols)] for i in range(A.rows)])
    return np.array([float(v) for v in A])


def rel(a, b):
    """|a - b| / |b| as a float, computed at the working precision."""
    return float(abs(mp.mpf(a) - mp.mpf(b)) / abs(mp.mpf(b)))
