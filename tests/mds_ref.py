"""NumPy restatement of metric SMACOF as sklearn/manifold/_mds.py::_smacof_single (1.7.2) runs it - the reference the device
kernel (hgp_smacof_steps_f64) is compared with.  Two deliberate differences from scikit-learn's code, none in the mathematics:
distances are formed by direct differences, sqrt(sum_c (x_ic - x_jc)^2), not by the expanded |x|^2 + |y|^2 - 2 x.y of
sklearn.metrics.euclidean_distances (which loses digits where embedded points nearly coincide), and nothing else is supported
(metric case, raw stress).  The update is B @ X / n as scikit-learn writes it."""
import numpy as np


def distances(X):
    """[n,n] Euclidean distances of the rows of X by direct differences; the diagonal is exactly zero."""
    diff = X[:, None, :] - X[None, :, :]
    return np.sqrt((diff ** 2).sum(axis=2))


def stress_norm(X, delta):
    """(sum_ij (d_ij - delta_ij)^2 / 2, sum_ij d_ij^2 / 2) of the configuration X."""
    d = distances(X)
    return ((d.ravel() - delta.ravel()) ** 2).sum() / 2, (d.ravel() ** 2).sum() / 2


def guttman(X, delta):
    """One Guttman transform: X_{k+1} = B X / n, B = -delta / d off the diagonal (d == 0 -> 1e-5), B_ii += sum_j ratio_ij."""
    n = X.shape[0]
    d = distances(X)
    d[d == 0] = 1e-5
    ratio = delta / d
    B = -ratio
    B[np.arange(n), np.arange(n)] += ratio.sum(axis=1)
    return 1.0 / n * np.dot(B, X)


def smacof_single(delta, X0, max_iter=300, eps=1e-6, trace=None):
    """(X, stress, n_iter) as _smacof_single(metric=True, normalized_stress=False, init=X0).  `trace` (a list) receives the stop
    criterion (old_stress - stress) / norm of every iteration that evaluates it, in order."""
    delta = np.asarray(delta, dtype=np.float64)
    X = np.array(X0, dtype=np.float64)
    old_stress = None
    it = -1
    stress = None
    for it in range(max_iter):
        X = guttman(X, delta)
        stress, norm = stress_norm(X, delta)
        if old_stress is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                crit = (old_stress - stress) / norm
            if trace is not None:
                trace.append(float(crit))
            if crit < eps:
                break
        old_stress = stress
    return X, stress, it + 1


def smacof(delta, starts, max_iter=300, eps=1e-6):
    """Best of the starts [B,n,p] as sklearn.manifold.smacof keeps it (`stress < best_stress`: the first of equals wins):
    (X, stress, n_iter, index of the best start, [(X, stress, n_iter) of every start])."""
    runs = [smacof_single(delta, X0, max_iter=max_iter, eps=eps) for X0 in starts]
    best = 0
    for b in range(1, len(runs)):
        if runs[b][1] < runs[best][1]:
            best = b
    return runs[best][0], runs[best][1], runs[best][2], best, runs


def drifting_groups(n, seed, dim=6, groups=3, sep=5.0, step=0.5):
    """n points in `dim` dimensions: `groups` separated groups (centres `sep` times a standard normal), each a slow drift (a
    random walk of steps `step` times a standard normal) that the points visit in turn - the shape of consecutive states of a
    few clusters, without near-coincident points.  Returns (points, their Euclidean distance matrix D)."""
    rng = np.random.default_rng(seed)
    cur = sep * rng.standard_normal((groups, dim))
    pts = np.empty((n, dim))
    for i in range(n):
        g = i % groups
        cur[g] += step * rng.standard_normal(dim)
        pts[i] = cur[g]
    D = distances(pts)
    return pts, 0.5 * (D + D.T)
