"""NumPy restatement of the glue of one member step of the LDS recursion, written from the contract in include/hdpgpc_hip.h
(hgp_lds_chain_gather2_batched_f64, hgp_lds_chain_finish2_batched_f64, hgp_copy_list_f64) and not from the kernels.

tests/test_chain_glue_ref.py pins it to the reference's own matrix_normal_inv_wishart.posterior / bayesian_new_params
(tests/golden/chain_step_t30.npz); tests/test_gpu_chain_glue.py compares the kernels with it bit for bit.

A chain's state is a dict:
    the eight stacks "A", "G", "C", "S", "Psm", "P" ([L,T,T]) and "F", "Fsm" ([L,T])       (order of hgp_chain_gather_desc.st)
    "W" [3,2,T,T] = means, right covariances, scales of the two MNIW distributions (0 = internal, 1 = observation)
    "n0", "Nf" floats, "pos" int, "bad_count" int32 [2].
Every function returns new arrays; its arguments are left as they are.  All arithmetic of finish_ref is float64, one correctly
rounded operation per operator, in the order the header writes it (NumPy does not contract a product and a sum).
"""
import copy

import numpy as np

STACKS = ("A", "G", "C", "S", "Psm", "P", "F", "Fsm")
EPS = float(np.finfo(np.float64).eps)
# bits of hgp_chain_finish_desc.annealing
ANNEAL, DRY, KEEP_PREV = 1, 2, 4


def jitter_ref(scale):
    """1e-2 max(mean |diag scale|, eps) (GPI_model.py:1314), the mean taken in np.longdouble; returns a longdouble."""
    d = np.abs(np.diag(scale)).astype(np.longdouble)
    return np.longdouble(1e-2) * max(d.sum() / np.longdouble(d.size), np.longdouble(EPS))


def gather_ref(stacks, pos, W, Y, y_row0):
    """(out[6 T T + 2 T], y_out[T] or None, Rp[2,T,T] in longdouble, jitter[2] in longdouble).
    out = row pos of the eight stacks in STACKS order; y_out = Y[pos - y_row0] (row 0 when y_row0 < 0; None when Y is None);
    Rp = W[1] + jitter I with jitter[m] = jitter_ref(W[2, m])."""
    T = W.shape[-1]
    out = np.concatenate([np.asarray(stacks[k][pos], dtype=np.float64).reshape(-1) for k in STACKS])
    assert out.size == 6 * T * T + 2 * T
    y_out = None if Y is None else np.array(Y[0 if y_row0 < 0 else pos - y_row0], dtype=np.float64)
    jit = np.array([jitter_ref(W[2, m]) for m in range(2)], dtype=np.longdouble)
    Rp = W[1].astype(np.longdouble)
    for m in range(2):
        Rp[m][np.diag_indices(T)] += jit[m]
    return out, y_out, Rp, jit


def finish_ref(state, inputs, info1, info2, flags):
    """The state after hgp_lds_chain_finish2_batched_f64.  inputs: dict of f_post, f_sm_prev, y [T], c_post, P_sm_prev [T,T],
    part, Snew [2,T,T]; info1 [4], info2 [2]; flags = the descriptor's `annealing` field."""
    s = copy.deepcopy(state)
    W = s["W"]
    n0, Nf1, pos = float(s["n0"]), float(s["Nf"]) + 1.0, int(s["pos"])
    f_post, f_sm_prev, y = (np.asarray(inputs[k], dtype=np.float64).reshape(-1) for k in ("f_post", "f_sm_prev", "y"))
    bad = bool(info1[2] != 0 or info1[3] != 0 or info2[0] != 0 or info2[1] != 0)
    dry, keep_prev = bool(flags & DRY), bool(flags & KEEP_PREV)
    if bad:                                          # the previous distributions are kept (GPI_model.py:1068-1071)
        means, R, scales, n0n = W[0].copy(), W[1].copy(), W[2].copy(), n0
    else:
        e = (f_post - f_sm_prev, y - f_post)         # y1 - y2 of the internal and of the observation update
        ee = np.stack([np.outer(e[0], e[0]), np.outer(e[1], e[1])])
        means = ((n0 - 2.0) * W[0] + inputs["part"]) / (n0 - 1.0)
        R = np.array(inputs["Snew"], dtype=np.float64)
        scales = ((n0 - 2.0) * W[2] + ee) / (n0 - 1.0)
        n0n = n0 + 1.0
    scl = n0n / (n0n - 2.0)
    ann = 1.0 / (Nf1 * Nf1) if flags & ANNEAL else 0.0
    nxt = pos + 1
    s["A"][nxt], s["C"][nxt] = means[0], means[1]
    s["G"][nxt] = scales[0] * scl + s["G"][0] * ann
    s["S"][nxt] = scales[1] * scl + s["S"][0] * ann
    s["P"][nxt] = s["Psm"][nxt] = inputs["c_post"]
    s["F"][nxt] = s["Fsm"][nxt] = f_post
    if not keep_prev:                                # the re-smoothed previous state (backwards_pair, GPI_model.py:705-716)
        s["Psm"][pos] = inputs["P_sm_prev"]
        s["Fsm"][pos] = f_sm_prev
    if not dry:                                      # a candidate step writes rows only
        s["W"] = np.stack([means, R, scales])
        s["n0"], s["Nf"], s["pos"] = n0n, Nf1, nxt
    s["bad_count"][0] += int(bad)
    if s["bad_count"][1] == 0 and (info1[0] != 0 or info1[1] != 0):
        s["bad_count"][1] = nxt
    return s


def copy_ref(items):
    """hgp_copy_list_f64: items = [(src, dst, n)], arrays; dst[:n] = src[:n] in list order, in place."""
    for src, dst, n in items:
        dst[:n] = src[:n]
