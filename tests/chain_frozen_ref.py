"""NumPy restatement of hgp_lds_chain_finish2_batched_f64 with bit 3 of its flag word set (parameters frozen: a cluster at its
estimation limit), written from the contract in include/hdpgpc_hip.h and not from the kernel; without the bit it is
chain_glue_ref.finish_ref.

tests/test_chain_frozen_ref.py pins it to the reference's own include_weighted_sample + backwards_pair + bayesian_new_params
at and behind the limit (tests/golden/chain_step_estlimit_t30.npz); tests/test_gpu_chain_frozen.py compares the kernel with it
bit for bit.  State, inputs and conventions: chain_glue_ref.
"""
import copy

import numpy as np

import chain_glue_ref as cg

FROZEN = 8              # bit 3 of hgp_chain_finish_desc.annealing
PARAMS = cg.STACKS[:4]


def finish_ref(state, inputs, info1, info2, flags):
    """The state after the finish kernel.  With FROZEN: the state rows as without it (DRY, KEEP_PREV hold), the parameter rows
    copied forward, W / n0 / bad_count[0] untouched; part, Snew, info1[2..3] and info2 have no influence."""
    if not flags & FROZEN:
        return cg.finish_ref(state, inputs, info1, info2, flags)
    s = copy.deepcopy(state)
    pos = int(s["pos"])
    nxt = pos + 1
    f_post = np.asarray(inputs["f_post"], dtype=np.float64).reshape(-1)
    for k in PARAMS:
        s[k][nxt] = s[k][pos]
    s["P"][nxt] = s["Psm"][nxt] = inputs["c_post"]
    s["F"][nxt] = s["Fsm"][nxt] = f_post
    if not flags & cg.KEEP_PREV:
        s["Psm"][pos] = inputs["P_sm_prev"]
        s["Fsm"][pos] = np.asarray(inputs["f_sm_prev"], dtype=np.float64).reshape(-1)
    if not flags & cg.DRY:
        s["Nf"], s["pos"] = float(s["Nf"]) + 1.0, nxt
    if s["bad_count"][1] == 0 and (info1[0] != 0 or info1[1] != 0):
        s["bad_count"][1] = nxt
    return s
