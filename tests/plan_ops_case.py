"""Seeded inputs of the plan-update fixtures (tests/golden/plan_ops_t*.npz) and the map of the plan's device buffer.

Shared by tests/golden/make_golden_plan_ops.py (run once against the build whose operators are the yardstick) and
tests/test_gpu_plan_ops.py.  Every input is an integer from a frozen RandomState stream scaled by a power of two, so the
arrays are the same doubles on every machine (no libm call, no summation-order dependence)."""
import numpy as np

WAVE_T = (20, 50, 90, 128)     # padded 32, 64, 96, 128: every one-wave size, each with T < TP padding
COOP_T = 150                   # padded 192: the cooperative family
PAIRS_FB_CAP = 65536
N_SEG = 8


def n_clusters(T):
    return 2 if T > 128 else 3


def tp_for(T):
    if T <= 128:
        nb = (T + 15) // 16
        nb = max(2, (nb + 1) & ~1)
        return 16 * nb
    return 192 if T <= 192 else 256


def make_sigma(T, K, seed, iso=0):
    """[K,T,T]: cluster `iso` is s I, the others 0.05 B B^T / T + 0.125 I plus a small non-symmetric part."""
    rs = np.random.RandomState(seed)
    Sigma = np.zeros((K, T, T))
    for k in range(K):
        B = rs.randint(-512, 512, size=(T, T)) / 256.0
        R = rs.randint(-64, 64, size=(T, T)) / 65536.0
        Sigma[k] = 0.05 * ((B @ B.T) / T) + 0.125 * np.eye(T) + R
    if iso is not None:
        Sigma[iso] = 0.25 * np.eye(T)
    return Sigma


def make_case(T, seed=None):
    """Inputs of one shape: cluster 0 has Sigma = s I (iso flag), cluster 1 is ordinary (ell = 1.2), the last cluster has
    ell = 3.0 (its accuracy bound exceeds the default tolerance: solve-based).  With two clusters: iso + ell = 3.0."""
    K = n_clusters(T)
    seed = 1000 + T if seed is None else seed
    rs = np.random.RandomState(seed)
    theta = np.array([[1.0, 1.2, 0.125]] * K)
    theta[K - 1, 1] = 3.0
    theta[0, 0] = 1.5
    xb = np.arange(T, dtype=np.float64)
    mean = rs.randint(-256, 256, size=(K, T)) / 256.0
    x = xb[None, :] + rs.randint(-16, 16, size=(N_SEG, T)) / 64.0
    y = rs.randint(-512, 512, size=(N_SEG, T)) / 256.0
    return dict(T=T, K=K, theta=theta, xb=xb, mean=mean, Sigma=make_sigma(T, K, seed + 1), x=x, y=y,
                Sigma_other=make_sigma(T, K, seed + 2, iso=None))


def _r256(n):
    return (n + 255) & ~255


def plan_areas(T, K, total_bytes):
    """name -> (byte offset, byte length) of the areas the fixtures record, from the area order of plan_layout (hgp_plan.hip):
    theta, scal, six [K,TP,TP] matrices, M', a' from the front; the solve-based areas, acc_list and fb from the back (the
    cooperative overflow areas lie between and are not needed).  Every area is rounded up to 256 bytes."""
    TP = tp_for(T)
    NB = TP // 16
    mat = K * TP * TP * 8
    o = _r256(K * 3 * 8) + _r256(K * 8 * 8) + 6 * _r256(mat)
    areas = {"Mp": (o, mat)}
    o += _r256(mat)
    areas["ap"] = (o, K * TP * 8)
    ntl = NB * (NB - 1) // 2
    grid = 256 if NB > 8 else 512
    back = [("fb", (PAIRS_FB_CAP + 2) * 4), ("acc_list", (K + 1) * 4), ("sscr", grid * NB * NB * 256 * 8), ("mu", K * TP * 8),
            ("Sop", K * NB * NB * 256 * 8), ("Dop", K * 4 * NB * 256 * 8), ("LTop", K * ntl * 256 * 8), ("Lop", K * ntl * 256 * 8)]
    end = total_bytes
    for name, n in back:
        end -= _r256(n)
        areas[name] = (end, n)
    return areas


def read_area(plan, areas, name, dtype):
    off, n = areas[name]
    return plan._buf[off:off + n].view(dtype).cpu().numpy().copy()


PACKED = ("Lop", "LTop", "Dop", "Sop", "mu")


def record(plan, case):
    """The operators of the plan after update(): M', a', scal, acc_list and, for the flagged clusters, the packed operands."""
    import torch

    T, K = case["T"], case["K"]
    TP = tp_for(T)
    areas = plan_areas(T, K, plan._buf.numel())
    torch.cuda.synchronize()
    out = {"Mp": read_area(plan, areas, "Mp", torch.float64).reshape(K, TP, TP),
           "ap": read_area(plan, areas, "ap", torch.float64).reshape(K, TP),
           "scal": plan.scalars().cpu().numpy().copy(),
           "acc_list": read_area(plan, areas, "acc_list", torch.int32)}
    n = int(out["acc_list"][0])
    out["acc_list"][1 + n:] = 0   # entries behind the count are never written
    flagged = out["scal"][:, 7] != 0.0
    for name in PACKED:
        a = read_area(plan, areas, name, torch.float64).reshape(K, -1)
        out[name] = a[flagged]    # the areas of unflagged clusters are never written
    return out
