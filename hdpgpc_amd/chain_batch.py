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
Results are bit-identical to running the chains one after the other.  A STATIC model (Gamma = 0) has no pair smoother and no
parameter update: its chain is the filter alone, and every such chain with h = 1 members on the basis grid and T <= 128 - of any
length - goes into ONE hgp_static_chain_steps_f64 launch per basis length (_run_static; one workgroup per chain walks its members).
Chains neither step covers (soft members, irregular grids, T > 256, dynamic chains of fewer than 4 members, static ones with
T > 128) take GPI_model._full_pass_eager.  A chain with an estimation
limit runs the full step up to the limit and the frozen step (finish flag 8: no MNIW update, the parameters copied forward)
behind it, as two consecutive runs (_run_group).

The step itself - a chain's device state, its level lists, the descriptors, the launch order - is member_step.py, which the
online pool (online_chain.py) runs too; here is the offline orchestration around it.
"""
import numpy as np
import torch

from . import _ffi, ops
from .member_step import Chain, bind_static, finish_desc, gather_desc, member_step, shared_buffers, upload_descs, ws_size

f64 = torch.float64
UNROLL = 8                                   # member steps per captured hipGraph


class Job:
    """One chain: model `gp` absorbs the segments with resp > 0.99; `prev` = (q, q_lat) handed back when there are none."""

    def __init__(self, gp, x_trains, y_trains, resp, prev=(None, None)):
        self.gp, self.x, self.y, self.resp, self.prev = gp, x_trains, y_trains, torch.as_tensor(resp), prev
        self.active = torch.nonzero(self.resp > 0.99, as_tuple=False).reshape(-1).tolist()
        self.out = None


def _graphable(job):
    """The graphed member step covers: dynamic model, h = 1 for every active member, at least 4 members, the members on the
    basis grid, T <= 256."""
    gp = job.gp
    a = job.active
    if len(a) < 4 or gp.x_basis.shape[0] > _ffi.MAX_T_COOP:
        return False
    if not bool(torch.any(gp.Gamma[-1] != 0)) or not bool(torch.all(job.resp[a] == 1.0)):
        return False
    X2 = job.x[..., 0] if job.x.ndim == 3 else job.x
    return bool(torch.equal(X2[a], gp.x_basis.reshape(1, -1).expand(len(a), -1)))


def _on_basis_h1(job):
    """Every active member has h = 1 and sits on the basis grid."""
    gp, a = job.gp, job.active
    if not bool(torch.all(job.resp[a] == 1.0)):
        return False
    X2 = job.x[..., 0] if job.x.ndim == 3 else job.x
    return bool(torch.equal(X2[a], gp.x_basis.reshape(1, -1).expand(len(a), -1)))


def _static_fused(job):
    """The fused static filter chain covers: static model, h = 1 for every active member, the members on the basis grid,
    T <= 128; any number of members."""
    gp = job.gp
    if gp.x_basis.shape[0] > _ffi.MAX_T_WAVE or gp._is_dynamic():
        return False
    return _on_basis_h1(job)


class _MergedLevels:
    """The level lists of chains that advance together, merged chain-major: level l has per[l] items per chain."""

    def __init__(self, chs):
        self.per = [len(l_._items) for l_ in chs[0].lv]
        self.merged = [ops.GemmList.concat([ch.lv[l] for ch in chs]).finalize() for l in range(len(self.per))]

    def run(self, l, lo, hi):
        self.merged[l].run_range(self.per[l] * lo, self.per[l] * (hi - lo))


def run(jobs):
    """Execute the jobs; returns [(q, q_lat)] in job order (scores of every segment under the finished model, as
    full_pass_weighted returns them)."""
    for j in jobs:
        j.x, j.y = j.gp.cond_to_torch(j.x), j.gp.cond_to_torch(j.y)
    by_T = {}                                          # chains advance in lock-step only with chains of their own basis length
    static_by_T = {}                                   # static chains: one launch per basis length
    for j in jobs:
        if not len(j.active):
            j.out = j.prev
        elif _graphable(j):
            by_T.setdefault(int(j.gp.x_basis.shape[0]), []).append(j)
        elif _static_fused(j):
            static_by_T.setdefault(int(j.gp.x_basis.shape[0]), []).append(j)
        else:
            j.out = j.gp._full_pass_eager(j.x, j.y, j.resp, j.active)
    for T, g in by_T.items():
        for group in ([g] if T <= _ffi.MAX_T_WAVE and len(g) >= 2 else [[j] for j in g]):
            _run_group(group)
    for T, g in static_by_T.items():
        _run_static(g, T)
    return [j.out for j in jobs]


def _run_group(jobs):
    """The graphed member step over the members of every job (all of one basis length), then commit, RTS pass and scores.
    A chain with an estimation limit E re-estimates its parameters while N' < E (N' = members after the inclusion) and keeps
    them from then on (GPI_model.py:974,1092): two consecutive runs over the same Chain, the full step for the first members and
    the frozen step (member_step.py: shorter lists, finish flag 8) for the rest, each in lock-step with the other chains' runs
    of its kind.  Without a limit the second run is empty."""
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
        j.bad = [0, 0]                                     # status words of the chain's runs (_advance); none without a step
        gp._check_pending()
        # member i of rest makes N' = N + i + 1: estimated while N' < E
        j.n_full = len(j.rest) if gp.estimation_limit == np.inf else int(min(max(gp.estimation_limit - gp.N - 1, 0), len(j.rest)))
        ch = j.ch = Chain.from_model(gp, len(gp.f_star) + len(j.rest))
        ch.ws = torch.empty(ws_size(T), dtype=f64, device=dev)            # gathered previous state
        ch.bad = torch.zeros(2, dtype=torch.int32, device=dev)            # [MNIW updates skipped, first step whose filter failed]
        ch.sync = torch.zeros(1, dtype=torch.int32, device=dev)           # inter-block counter of the finish kernel
        # observations of the run; the step reads row (pos - y_row0) inside its gather kernel
        ch.Y = (j.y[j.rest][..., 0] if j.y.ndim == 3 else j.y[j.rest]).reshape(len(j.rest), -1).contiguous()
        ch.y_row0 = int(ch.pos[0])
    for frozen in (False, True):
        part = [(j, len(j.rest) - j.n_full if frozen else j.n_full) for j in jobs]
        part = sorted([p for p in part if p[1] > 0], key=lambda p: -p[1])      # longest first: the live set is always a prefix
        if part:
            _advance([j for j, _ in part], [n for _, n in part], T, frozen)
    bads = [j.bad for j in jobs]
    nc = len(jobs)
    main = torch.cuda.current_stream()
    side = [None] if nc == 1 else [torch.cuda.Stream() for _ in jobs]
    for j, s, bad in zip(jobs, side, bads):                # commit + backward recursion (lock-step: one stream per chain)
        gp, ch = j.gp, j.ch
        L = int(ch.pos[0]) + 1
        ch.bind_model(gp, L, float(ch.n0), Lp=int(min(L, gp.estimation_limit)))
        for idx in j.rest:
            gp.indexes.append(int(idx))
            gp.x_train.append(j.x[idx])
            gp.y_train.append(j.y[idx].reshape(-1, 1))
        gp.N += len(j.rest)
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
        j.out = (gp.compute_sq_err_all(j.x, j.y), gp.compute_q_lat_all(j.x))
        del j.ch


def _run_static(jobs, T):
    """The filter chains of static models (all of basis length T <= 128), every member of every chain, in ONE launch
    (hgp_static_chain_steps_f64), then commit and scores.  What GPI_model._full_pass_eager does for a static model, member by
    member: include_weighted_sample(h = 1) - the kernel fit before the first member of a model that has none, then the Kalman
    update from the last smoothed state (for a static model: the last filtered one) - and nothing else."""
    dev = jobs[0].gp.device
    descs, keep = [], []
    for j in jobs:
        gp = j.gp
        gp._check_pending()
        idx0 = j.active[0]
        if gp.N == 0 and not gp.fitted:                    # include_weighted_sample, GPI_model.py:361-363
            gp.fit_kernel_params(j.x[idx0].reshape(-1, 1), j.y[idx0], gp.Sigma[-1], gp.Gamma[-1], valid=True)
        # GPI.py:136-139: a prior covariance that is the kernel Gram itself takes the first-step branch (only a model's first member can)
        k = gp.gp.kernel
        first = gp.N == 0 and bool(torch.equal(gp.cov_f_sm[-1], k(gp.x_basis, gp.x_basis)))
        L, n = len(gp.f_star_sm), len(j.active)
        Fsm = torch.empty((L + n, T, 1), dtype=f64, device=dev)
        Psm = torch.empty((L + n, T, T), dtype=f64, device=dev)
        Fsm[:L] = gp.f_star_sm.stack().reshape(L, T, 1)
        Psm[:L] = gp.cov_f_sm.stack()
        j.st = (Fsm, Psm, L, torch.zeros(1, dtype=torch.int32, device=dev))
        Y = (j.y[..., 0] if j.y.ndim == 3 else j.y).reshape(j.y.shape[0], -1).contiguous()
        ops_in = (gp.A[-1].contiguous(), gp.C[-1].contiguous(), gp.Sigma[-1].contiguous(), Y,
                  torch.tensor([L - 1], dtype=torch.int64, device=dev), ops.to_dev(np.asarray(j.active, dtype=np.int64), torch.int64, dev))
        keep.append(ops_in)
        A, C, Sigma, Y, pos, y_idx = ops_in
        descs.append(ops.static_chain_desc(A, C, Sigma, Fsm, Psm, pos, Y, y_idx, j.st[3], n, L - 1, first=first,
                                           white=(k.constant_value + k.noise_level) - k.constant_value))
    n_max = max(len(j.active) for j in jobs)
    ddev = upload_descs(descs, dev)
    ops.static_chain_steps(ddev, len(jobs), T, n_max)
    infos = torch.cat([j.st[3] for j in jobs]).tolist()    # waits for the launch: the descriptors and what they point to may go
    del keep, ddev
    for j, info in zip(jobs, infos):
        gp = j.gp
        Fsm, Psm, L, _ = j.st
        bind_static(gp, Fsm, Psm, L)
        for idx in j.active:
            gp.indexes.append(int(idx))
            gp.x_train.append(j.x[idx].reshape(-1, 1))
            gp.y_train.append(j.y[idx].reshape(-1, 1))
        gp.N += len(j.active)
        gp.static_chain_calls = getattr(gp, "static_chain_calls", 0) + 1
        del j.st
        if info != 0:        # torch.linalg of the reference would have raised at that member
            raise torch.linalg.LinAlgError("posterior: the input is not positive-definite")
        j.out = (gp.compute_sq_err_all(j.x, j.y), gp.compute_q_lat_all(j.x))


def _advance(jobs, lengths, T, frozen):
    """lengths[c] member steps of the chain of jobs[c] (lengths descending), side by side; frozen: the step of a chain at its
    estimation limit.  Waits for the steps and leaves every chain's status words in its job (job.bad)."""
    dev = jobs[0].gp.device
    nc = len(jobs)
    sh = shared_buffers(nc, T, dev)
    chs = [j.ch for j in jobs]
    for c, ch in enumerate(chs):
        ch.build_lists(sh, c, frozen=frozen)
    gdev = upload_descs([gather_desc(ch) for ch in chs], dev)
    fdev = upload_descs([finish_desc(ch, int(bool(j.gp.annealing)) | (8 if frozen else 0), ch.bad) for j, ch in zip(jobs, chs)], dev)
    levels = _MergedLevels(chs)
    step = lambda k: member_step(levels, sh, gdev, fdev, 0, k, T, frozen=frozen)      # noqa: E731  (one member of the first k chains)

    graphs = []
    done = 0
    for k in range(nc, 0, -1):                             # phase: the first k chains are alive for lengths[k-1] - done steps
        n_it = lengths[k - 1] - done
        if n_it > 0:
            graphs.append(_replay([j.gp for j in jobs[:k]], lambda: step(k), n_it, 1 if nc == 1 else 2 * UNROLL))
            done += n_it
    for j, ch in zip(jobs, chs):                       # the first read-back waits for every replay: the graphs may go
        j.bad = ch.bad.tolist()                        # (the words accumulate over a chain's runs: its last run's are final)
    del graphs


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
