"""The MDS embedding of a distance matrix - sklearn.manifold.MDS(dissimilarity='precomputed') / sklearn.manifold.smacof, metric
case (sklearn/manifold/_mds.py), what plot_MDS / plot_MDS_plotly run on the state-distance matrix (util_plots.py:619-620) - with
every start side by side on the device (hgp_smacof_steps_f64, include/hdpgpc_hip_mds.h): nothing returns to the host but one
status vector per chunk of iterations.  The start configurations are drawn on the host, in scikit-learn's order."""
import numbers

import numpy as np
import torch


def _random_state(seed):
    """sklearn.utils.check_random_state."""
    if seed is None or seed is np.random:
        return np.random.mtrand._rand
    if isinstance(seed, numbers.Integral):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError(f"{seed!r} cannot be used to seed a numpy.random.RandomState instance")


def initial_configurations(n, p, n_init, random_state=None):
    """The n_init start configurations [n_init, n, p] that smacof(n_init=...) / MDS draw one after the other from ONE
    RandomState (an int seed, a RandomState, or None for numpy's global one): uniform(size=n * p).reshape(n, p) each."""
    rs = _random_state(random_state)
    return np.stack([rs.uniform(size=n * p).reshape(n, p) for _ in range(int(n_init))]) if n_init > 0 else np.zeros((0, n, p))


def smacof(delta, n_components=2, init=None, n_init=4, max_iter=300, eps=1e-6, random_state=None, chunk=50):
    """Metric SMACOF on the symmetric distance matrix delta [n,n] (a host array or an fp64 device tensor, which is used where it
    lies), parameters as sklearn.manifold.smacof(metric=True, normalized_stress=False): n_init random starts (or `init` [n,p] /
    [B,n,p], which replaces them), each at most max_iter iterations, stopped when the relative decrease of the stress falls
    below eps.  All starts advance side by side; the host reads one status vector per `chunk` iterations.
    Returns (X [n,p], stress, n_iter) of the start with the smallest stress (the first of equals), as host values, and a dict
    with every start's `X` [B,n,p], `stress`, `n_iter`, `status` [B] (1: stop rule, 2: max_iter) and `best`.
    ValueError: delta not square or not symmetric (numpy.allclose with atol 1e-10, sklearn's check_symmetric);
    FloatingPointError: a start met a non-finite stress (non-finite delta or init)."""
    from . import ops                            # the library: initial_configurations needs none

    f64 = torch.float64
    if torch.is_tensor(delta):
        D = delta if delta.is_cuda else delta.to("cuda")
        D = D.to(f64)
    else:
        D = torch.as_tensor(np.ascontiguousarray(delta, dtype=np.float64), device="cuda")
    if D.dim() != 2 or D.shape[0] != D.shape[1] or D.shape[0] < 1:
        raise ValueError(f"smacof: delta must be a square matrix, got {tuple(D.shape)}")
    if D.stride(1) != 1 and D.shape[0] > 1:
        D = D.contiguous()
    if not bool(torch.allclose(D, D.T, atol=1e-10)):
        raise ValueError("smacof: delta must be symmetric")
    n, dev = D.shape[0], D.device
    if init is not None:
        X0 = np.array(init.detach().cpu().numpy() if torch.is_tensor(init) else init, dtype=np.float64)
        if X0.ndim == 2:
            X0 = X0[None]
        if X0.ndim != 3 or X0.shape[1] != n or X0.shape[0] < 1:
            raise ValueError(f"smacof: init must be [{n}, p] or [B, {n}, p]")
    else:
        if n_init < 1:
            raise ValueError("smacof: n_init < 1")
        X0 = initial_configurations(n, int(n_components), n_init, random_state)
    if not 1 <= X0.shape[2] <= 3:
        raise ValueError("smacof: n_components must be 1, 2 or 3")
    if max_iter < 1 or chunk < 1:
        raise ValueError("smacof: max_iter and chunk must be at least 1")
    B = X0.shape[0]
    X = torch.as_tensor(np.ascontiguousarray(X0), device=dev)
    state = torch.zeros((B, ops._ffi.MDS_STATE_DOUBLES), dtype=f64, device=dev)
    status, n_it = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    stress = torch.zeros(B, dtype=f64, device=dev)
    left = int(max_iter) + 1                     # the end at max_iter takes one pass more (the stress of the last iterate)
    while left > 0:
        steps = min(int(chunk), left)
        ops.smacof_steps(D, X, state, status, stress, n_it, steps, eps=eps, max_iter=max_iter)
        left -= steps
        st = status.cpu().numpy()
        if np.all(st != 0):
            break
    if np.any(st < 0):
        raise FloatingPointError(f"smacof: non-finite stress in start(s) {np.nonzero(st < 0)[0].tolist()} (non-finite delta or init)")
    assert np.all(st != 0), "a start is still running after max_iter + 1 passes"
    Xh, sh, nh = X.cpu().numpy(), stress.cpu().numpy(), n_it.cpu().numpy().astype(np.int64)
    best = 0
    for b in range(1, B):                        # sklearn.manifold.smacof: `stress < best_stress`, the first of equals stays
        if sh[b] < sh[best]:
            best = b
    return Xh[best].copy(), float(sh[best]), int(nh[best]), {"X": Xh, "stress": sh, "n_iter": nh, "status": st.astype(np.int64), "best": best}
