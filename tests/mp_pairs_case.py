"""Seeded inputs of the 40-digit pair fixtures (tests/golden/mp_pairs_t*.npz): clusters on both sides of the accuracy threshold.

Shared by tests/golden/make_golden_mp_pairs.py, tests/test_mp_ref_host.py and tests/test_gpu_pairs_truth.py.  As in
plan_ops_case.py every random input is an integer from a frozen RandomState stream scaled by a power of two, and what is derived
from them uses single correctly rounded operations only, so the arrays are the same doubles on every machine and are not stored;
the fixtures carry their SHA-256.

Clusters (K = 4 per size), Sigma from plan_ops_case.make_sigma (SPD plus a small non-symmetric part):
  (a) c = 1,   ell = 1.2                 bound ~ 1e-11: explicit operator, far below the threshold
  (b) c = 1.5, ell = ELL_BELOW[T]        truth bound in [0.25, 0.5] x 1e-9: explicit operator, just below the threshold
  (c) c = 1,   ell = ELL_ABOVE[T]        truth bound in [2, 4] x 1e-9: solve-based, just above it
  (d) c = 1,   ell = 3.0, Sigma = s I    the iso branch on an ill-conditioned kernel: solve-based
ELL_BELOW / ELL_ABOVE were bisected in float64 for these Sigma and c (make_golden_mp_pairs.py --bisect: targets 0.35e-9 and
2.8e-9, rounded to four decimals); the generator asserts the windows on the 40-digit bound.

Segments (N = 4 per size): two of length T - the basis grid jittered by up to 0.25 steps (the static band pattern) and a jittered
grid reversed and shifted by +3.7 (fall-back list, generic kernel) - and two of length ceil(0.7 T) on a jittered grid of step
45/32 (T* != T)."""
import hashlib

import numpy as np

import plan_ops_case as pc

SIZES = (20, 50, 90, 128, 150)      # padded 32, 64, 96, 128, 192
K = 4
N_FULL, N_SHORT = 2, 2
EXPLICIT = (0, 1)                   # clusters whose M' the fixtures hold
WIN_BELOW = (0.25e-9, 0.5e-9)
WIN_ABOVE = (2e-9, 4e-9)
C_BELOW = 1.5
ELL_BELOW = {20: 1.374, 50: 1.3558, 90: 1.3555, 128: 1.3556, 150: 1.3555}
ELL_ABOVE = {20: 1.4651, 50: 1.4397, 90: 1.4392, 128: 1.4392, 150: 1.4392}


def short_len(T):
    return (7 * T + 9) // 10


def make_case(T, ell_below=None, ell_above=None):
    rs = np.random.RandomState(2000 + T)
    theta = np.array([[1.0, 1.2, 0.125],
                      [C_BELOW, ELL_BELOW[T] if ell_below is None else ell_below, 0.125],
                      [1.0, ELL_ABOVE[T] if ell_above is None else ell_above, 0.125],
                      [1.0, 3.0, 0.125]])
    xb = np.arange(T, dtype=np.float64)
    mean = rs.randint(-256, 256, size=(K, T)) / 256.0
    m = short_len(T)
    jit = lambda n, t: rs.randint(-16, 17, size=(n, t)) / 64.0  # noqa: E731
    x_full = xb[None, :] + jit(N_FULL, T)
    x_full[1] = x_full[1, ::-1] + 3.7
    x_short = (np.arange(m, dtype=np.float64) * 1.40625)[None, :] + jit(N_SHORT, m)
    y_full = rs.randint(-512, 512, size=(N_FULL, T)) / 256.0
    y_short = rs.randint(-512, 512, size=(N_SHORT, m)) / 256.0
    # first_noise on a scattered third of the pairs: 2^-6 ... 2^-3
    n_all = N_FULL + N_SHORT
    first = np.where(np.add.outer(np.arange(n_all), np.arange(K)) % 3 == 0, rs.randint(1, 9, size=(n_all, K)) / 64.0, 0.0)
    return dict(T=T, K=K, theta=theta, xb=xb, mean=mean, Sigma=pc.make_sigma(T, K, 3000 + T, iso=3),
                sets=((x_full, y_full), (x_short, y_short)), first=first)


def set_rows(s):
    """Rows of the fixtures' [N, K] arrays that segment set s (0: length T, 1: length ceil(0.7 T)) fills."""
    return slice(0, N_FULL) if s == 0 else slice(N_FULL, N_FULL + N_SHORT)


def digest(case):
    h = hashlib.sha256()
    for a in (case["theta"], case["xb"], case["mean"], case["Sigma"], case["sets"][0][0], case["sets"][0][1], case["sets"][1][0],
              case["sets"][1][1], case["first"]):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8)


# ---- the gates of tests/test_gpu_pairs_truth.py, stated once: the host tier (tests/test_mp_ref_host.py) holds a NumPy restatement
# of both paths to the same ones.  err / err_ref are relative errors against truth of the evaluation under test and of the
# float64 oracle for the same pairs; every function returns observed / allowed, so a gate holds when the value is <= 1.
EPS = float(np.finfo(np.float64).eps)
RT_PAIR = 1e-8


def rel_each(got, truth):
    return np.abs(np.asarray(got, dtype=np.float64) - truth) / np.abs(truth)


def oracle_errors(case, gold, first):
    """err_ref [N, K] of quad and of logdet: the oracle against truth, for both segment sets."""
    from oracle import hdpgpc_oracle as orc

    q, ld = np.zeros_like(gold["quad"]), np.zeros_like(gold["quad"])
    for s, (xs, ys) in enumerate(case["sets"]):
        r = set_rows(s)
        _, q[r], ld[r] = orc.loglik_pairs(xs, ys, case["xb"], case["theta"], case["mean"], case["Sigma"],
                                          first_noise=case["first"][r] if first else None)
    sfx = "_first" if first else ""
    return rel_each(q, gold["quad" + sfx]), rel_each(ld, gold["logdet" + sfx])


def gate_promise(err):
    return float(err.max()) / RT_PAIR


def gate_bound(err_k, err_ref_k, bound_k):
    """Explicit-operator clusters: err <= truth bound + 4 max(err_ref of the cluster's pairs, eps)."""
    return float(err_k.max()) / (bound_k + 4.0 * max(float(err_ref_k.max()), EPS))


def gate_solve(err_k, err_ref_k):
    """Solve-based clusters: err <= 8 max(err_ref of the cluster's pairs, 64 eps)."""
    return float(err_k.max()) / (8.0 * max(float(err_ref_k.max()), 64.0 * EPS))


def gate_inverse(T, kappa_k):
    """8 T eps kappa_inf: first-order forward bound of an inverse taken through a Cholesky factor."""
    return 8.0 * T * EPS * kappa_k


def triu_to_full(T, tri):
    M = np.zeros((T, T))
    M[np.triu_indices(T)] = tri
    return M + np.triu(M, 1).T
