"""The offline member step (filter, pair smoother and MNIW update, one member per step) of one chain or of many independent
chains side by side ("the sequential LDS recursion does not shard over segments: parallel over independent
chains - clusters x leads x birth proposals").

One chain = GPI_model.full_pass_weighted of one model over its members (GPI_model.py:377-406): strictly sequential, ~14
dependent launches per member, each a few microseconds of work on a few compute units - the chip is >90 % idle.  The
variational loop, however, asks for many chains that do not depend on each other (the clusters a proposal changes, the leads,
the proposals of one exploration round, the classes of reload_model_from_labels).  ``run(jobs)`` advances chains of the same
basis length T <= 128 in lock-step with the SAME number of launches per member step as one chain:

* every dependency level of the step is one ``hgp_gemm_list_f64`` launch over the concatenated item lists of all chains,
* the two inversions of the step are one ``hgp_chol_inverse_rhs_batched_f64`` launch each over [4 * chains] / [2 * chains]
  matrices, gather and finish are the descriptor-array launches ``hgp_lds_chain_*2_batched_f64`` (blockIdx.y = chain),
* chains are sorted by length; when the shortest live chain ends the launches simply shrink to a prefix (every buffer and list
  is laid out chain-major), each phase captured once as a hipGraph and replayed,
* the backward (RTS) recursions then run concurrently, one stream per chain.

Every other chain runs the same step as a group of one (n_chains = 1): a chain without a partner of its length, and every chain
with 128 < T <= 256, whose inversions are the cooperative inverse-only kernels with Z rhs one more list level behind each (the
batch size picks the inversion kernel, so these chains are not batched).  GPI_model.full_pass_weighted is ``run`` over one job.
Results are bit-identical to running the chains one after the other.  Chains the graphed step does not cover (static models,
soft members, irregular grids, T > 256, fewer than 4 members, an estimation limit) take GPI_model._full_pass_eager.
"""
import ctypes

import numpy as np
import torch

from . import _ffi, ops

f64 = torch.float64
UNROLL = 8                                   # member steps per captured hipGraph
_STACKS = ("A", "G", "C", "S", "Psm", "P", "F", "Fsm")          # order of hgp_chain_gather_desc.st
_SH4 = ("X4", "RH4", "Z4", "Y4", "i4")       # step buffers of the first inversion: four matrices per chain, the others two


class Job:
    """One chain: model `gp` absorbs the segments with resp > 0.99; `prev` = (q, q_lat) handed back when there are none."""

    def __init__(self, gp, x_trains, y_trains, resp, prev=(None, None)):
        self.gp, self.x, self.y, self.resp, self.prev = gp, x_trains, y_trains, torch.as_tensor(resp), prev
        self.active = torch.nonzero(self.resp > 0.99, as_tuple=False).reshape(-1).tolist()
        self.out = None


def _graphable(job):
    """The graphed member step covers: dynamic model, h = 1 for every active member, at least 4 members, no estimation limit,
    the members on the basis grid, T <= 256."""
    gp = job.gp
    a = job.active
    if len(a) < 4 or gp.x_basis.shape[0] > 256 or gp.estimation_limit != np.inf:
        return False
    if not bool(torch.any(gp.Gamma[-1] != 0)) or not bool(torch.all(job.resp[a] == 1.0)):
        return False
    X2 = job.x[..., 0] if job.x.ndim == 3 else job.x
    return bool(torch.equal(X2[a], gp.x_basis.reshape(1, -1).expand(len(a), -1)))


def _descs(structs, dev):
    arr = (type(structs[0]) * len(structs))(*structs)
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(dev)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def gather_desc(ch, T, Y, y_row0):
    """hgp_chain_gather_desc of a chain (GPI_model._chain_alloc + _chain_lists); the step reads observation row pos - y_row0 of Y
    (y_row0 < 0: Y is the observation itself)."""
    b = ch["bufs"]
    g = _ffi.ChainGatherDesc()
    for i, k in enumerate(_STACKS):
        g.st[i] = ch[k].data_ptr()
    g.pos, g.out, g.Y, g.y_out, g.W, g.Rp = _p(ch["pos"]), _p(ch["ws"]), _p(Y), _p(b["y"]), _p(ch["W"]), _p(b["X4"][2:4])
    g.y_row0, g.T = y_row0, T
    return g


def finish_desc(ch, T, flags, bad):
    """hgp_chain_finish_desc of a chain; flags = its `annealing` field (include/hdpgpc_hip.h), bad = the status words it updates."""
    b = ch["bufs"]
    f = _ffi.ChainFinishDesc()
    f.f_post, f.c_post, f.f_sm_prev, f.P_sm_prev, f.y = _p(b["f_post"]), _p(b["c_post"]), _p(b["f_sm_prev"]), _p(b["P_sm_prev"]), _p(b["y"])
    f.part, f.Snew, f.info1, f.info2 = _p(b["part"]), _p(b["S__"]), _p(ch["i4"]), _p(ch["i2"])
    f.W, f.n0, f.Nf, f.bad_count = _p(ch["W"]), _p(ch["n0"]), _p(ch["Nf"]), _p(bad)
    f.stA, f.stG, f.stC, f.stS = _p(ch["A"]), _p(ch["G"]), _p(ch["C"]), _p(ch["S"])
    f.stF, f.stFsm, f.stP, f.stPsm = _p(ch["F"]), _p(ch["Fsm"]), _p(ch["P"]), _p(ch["Psm"])
    f.pos, f.sync, f.T, f.annealing = _p(ch["pos"]), _p(ch["sync"]), T, flags
    return f


def run(jobs):
    """Execute the jobs; returns [(q, q_lat)] in job order (scores of every segment under the finished model, as
    full_pass_weighted returns them)."""
    for j in jobs:
        j.x, j.y = j.gp.cond_to_torch(j.x), j.gp.cond_to_torch(j.y)
    by_T = {}                                          # chains advance in lock-step only with chains of their own basis length
    for j in jobs:
        if not len(j.active):
            j.out = j.prev
        elif _graphable(j):
            by_T.setdefault(int(j.gp.x_basis.shape[0]), []).append(j)
        else:
            j.out = j.gp._full_pass_eager(j.x, j.y, j.resp, j.active)
    for T, g in by_T.items():
        for group in ([g] if T <= 128 and len(g) >= 2 else [[j] for j in g]):
            _run_group(group)
    return [j.out for j in jobs]


def _run_group(jobs):
    """The graphed member step over the members of every job (all of one basis length), then commit, RTS pass and scores."""
    dev = jobs[0].gp.device
    T = int(jobs[0].gp.x_basis.shape[0])
    assert all(j.gp.x_basis.shape[0] == T for j in jobs)
    # the first member of a fresh model takes the eager path (kernel fit, prior-predictive first step)
    for j in jobs:
        gp = j.gp
        head = 1 if gp.N == 0 else 0
        for index in j.active[:head]:
            gp.include_weighted_sample(index, j.x[index], j.x[index], j.y[index], 1.0)
            gp.backwards_pair(1.0)
            gp.bayesian_new_params(1.0)
        j.rest = j.active[head:]
        gp._check_pending()
    jobs = sorted(jobs, key=lambda j: -len(j.rest))    # longest first: the live set is always a prefix
    nc = len(jobs)
    new = lambda *shape: torch.zeros(shape, dtype=f64, device=dev)      # noqa: E731
    sh = {"X4": new(nc * 4, T, T), "RH4": new(nc * 4, T, T), "Z4": new(nc * 4, T, T), "Y4": new(nc * 4, T, T),
          "S__": new(nc * 2, T, T), "S_": new(nc * 2, T, T), "Zs": new(nc * 2, T, T), "Y3": new(nc * 2, T, T),
          "i4": torch.zeros(nc * 4, dtype=torch.int32, device=dev), "i2": torch.zeros(nc * 2, dtype=torch.int32, device=dev)}
    rhs_on = torch.tensor([1, 1, 0, 0] * nc, dtype=torch.int32, device=dev)
    per_chain = lambda k: 4 if k in _SH4 else 2          # noqa: E731
    chs = []
    for c, j in enumerate(jobs):
        ch = j.gp._chain_alloc(len(j.rest))
        # observations of the run; the step reads row (pos - y_row0) inside its gather kernel
        ch["Y"] = (j.y[j.rest][..., 0] if j.y.ndim == 3 else j.y[j.rest]).reshape(len(j.rest), -1).contiguous()
        ch["y_row0"] = int(ch["pos"][0])
        j.gp._chain_lists(ch, views={k: v[per_chain(k) * c:per_chain(k) * (c + 1)] for k, v in sh.items()})
        chs.append(ch)
    gdev = _descs([gather_desc(ch, T, ch["Y"], ch["y_row0"]) for ch in chs], dev)
    fdev = _descs([finish_desc(ch, T, int(bool(j.gp.annealing)), ch["bad"]) for j, ch in zip(jobs, chs)], dev)
    # level lists, chain-major: items [0, n_l * k) of level l belong to the first k chains
    n_lv = len(chs[0]["lv"])
    per = [len(chs[0]["lv"][l]._items) for l in range(n_lv)]
    merged = [ops.GemmList.concat([ch["lv"][l] for ch in chs]).finalize() for l in range(n_lv)]
    level = lambda l, k: merged[l].run_range(0, per[l] * k)          # noqa: E731
    riding = chs[0]["riding"]
    stream = ops._stream

    def step(k):                                           # one member of the first k chains
        _ffi.check(_ffi.lib.hgp_lds_chain_gather2_batched_f64(_p(gdev), k, T, stream()), "chain_gather2_batched")
        for l in range(4):
            level(l, k)
        if riding:
            ops.chol_inverse_rhs(sh["X4"][:4 * k], sh["Z4"], sh["RH4"], sh["Y4"], sh["i4"], rhs_on=rhs_on)
        else:
            ops.chol_inverse(sh["X4"][:4 * k], out=sh["Z4"][:4 * k], info=sh["i4"][:4 * k])
            level(10, k)
        for l in range(4, 9):
            level(l, k)
        if riding:
            ops.chol_inverse_rhs(sh["S__"][:2 * k], sh["Zs"], sh["S_"], sh["Y3"], sh["i2"], rhs_trans=True, add_diag=1e-8)
        else:
            ops.chol_inverse(sh["S__"][:2 * k], 0.0, 1e-8, out=sh["Zs"][:2 * k], info=sh["i2"][:2 * k])
            level(11, k)
        level(9, k)
        _ffi.check(_ffi.lib.hgp_lds_chain_finish2_batched_f64(_p(fdev), k, T, stream()), "chain_finish2_batched")

    lengths = [len(j.rest) for j in jobs]
    graphs = []
    done = 0
    for k in range(nc, 0, -1):                             # phase: the first k chains are alive for lengths[k-1] - done steps
        n_it = lengths[k - 1] - done
        if n_it > 0:
            graphs.append(_replay([j.gp for j in jobs[:k]], lambda: step(k), n_it, 1 if nc == 1 else 2 * UNROLL))
            done += n_it
    bads = [ch["bad"].tolist() for ch in chs]             # the first read-back waits for every replay: the graphs may go
    del graphs
    main = torch.cuda.current_stream()
    side = [None] if nc == 1 else [torch.cuda.Stream() for _ in jobs]
    for j, ch, s, bad in zip(jobs, chs, side, bads):       # commit + backward recursion (lock-step: one stream per chain)
        gp = j.gp
        gp._chain_commit(ch, j.rest, j.x, j.y)
        if bad[1] != 0:      # torch.linalg.solve / inv of the reference would have raised at that member
            raise torch.linalg.LinAlgError(f"posterior / backwards_pair: the input is not positive-definite (LDS step {bad[1]})")
        if bad[0] != 0 and gp.verbose:
            print("Alg error matrix ill conditioned.")     # GPI_model.py:1069
        if s is None:
            gp._backwards_graphed()
            continue
        s.wait_stream(main)
        with torch.cuda.stream(s):
            gp._backwards_graphed()
    for s in side:
        if s is not None:
            main.wait_stream(s)
    for j in jobs:
        gp = j.gp
        gp._check_pending()
        gp._stk = {}
        j.out = (gp.compute_sq_err_all(j.x, j.y), gp.compute_q_lat_all(j.x))


def _replay(gps, fn, n_iter, min_left):
    """fn() n_iter times: once eagerly on a side stream (warm-up = first iteration); then, if at least `min_left` (>= 1) iterations
    remain, UNROLL of them captured as ONE hipGraph and replayed (a replay costs ~8 us of launch gap, amortised over the unrolled
    iterations); the remainder eagerly.  The replays count in graph_replays of every model of `gps`.  Returns the graph (None
    without one), which must outlive its replays: nothing here waits for them.  A failed capture raises: silently re-running
    eagerly would both hide a 30x slow-down and, after a partial replay, apply steps twice."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    n_iter -= 1
    graph = None
    if n_iter >= min_left:
        unroll = min(UNROLL, n_iter)
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):
                for _ in range(unroll):
                    fn()
        except RuntimeError as e:
            raise RuntimeError(f"hipGraph capture of the LDS step failed: {e}") from e
        for _ in range(n_iter // unroll):
            graph.replay()
        for gp in gps:
            gp.graph_replays = getattr(gp, "graph_replays", 0) + n_iter // unroll
        n_iter %= unroll
    for _ in range(n_iter):
        fn()
    return graph
