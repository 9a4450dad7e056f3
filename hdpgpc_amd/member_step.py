"""The forward member step (Kalman update, pair smoother, two MNIW updates) of a chain on the device: the chain's state, its
level lists, the descriptors of its gather / finish kernels, and ``member_step`` - the one place the launch order is written.

The eager methods of GPI_model issue ~90 launches and one host sync per member: launch-bound.  For a dynamic model on a shared
grid with h = 1 the step is restated on pre-allocated stacks with device-side indices / counters and no host synchronisation,
one launch per dependency level.  Same arithmetic, same order.  The reference has no counterpart: device plumbing, kept out of
GPI_model.  chain_batch.py runs it offline under hipGraphs, online_chain.py on clusters kept as chains that are never torn down.
"""
import ctypes

import numpy as np
import torch

from . import _ffi, ops
from .GPI_model import matrix_normal_inv_wishart
from .steplist import StepList

f64 = torch.float64
_p = ops._ptr
_STACKS = ("A", "G", "C", "S", "Psm", "P", "F", "Fsm")          # order of hgp_chain_gather_desc.st
_PARAMS = _STACKS[:4]                                            # the parameter stacks (an estimation limit freezes them)
_LISTS = {"A": "A", "G": "Gamma", "C": "C", "S": "Sigma", "Psm": "cov_f_sm", "P": "cov_f", "F": "f_star", "Fsm": "f_star_sm"}
# a chain's gathered previous state `ws` (written by the gather kernel): six T x T matrices, then two T-vectors
_WS = ("A", "G", "C", "S", "Psm", "c0", "m0", "Fsm")
_WS_MATS = 6


def ws_size(T):
    return _WS_MATS * T * T + (len(_WS) - _WS_MATS) * T


def ws_offset(name, T):
    """Where `name` of _WS starts in a chain's ws (doubles)."""
    i = _WS.index(name)
    return i * T * T if i < _WS_MATS else _WS_MATS * T * T + (i - _WS_MATS) * T


def ws_view(ws, name, T):
    o = ws_offset(name, T)
    return ws[o:o + T * T].view(T, T) if name in _WS[:_WS_MATS] else ws[o:o + T]


# T <= 128: the right-hand sides ride the inversions; 128 < T <= 256: Z rhs is one more list level behind each of them
LV_RHS4, LV_RHS2 = 10, 11


def shared_buffers(n, T, dev, work=False):
    """The step buffers n chains that run side by side share, [n, ...] each (chain c's slice: [c]), so that each inversion is one
    batched launch: four matrices per chain for the first (X4 = [P, Sk, R0', R1'], RH4 = right-hand sides, riding where rhs_on,
    Z4 = L^-1, Y4 = Z rhs, status i4), two for the second (S__, S_, Zs, Y3, i2).  work: with WK4 / WK2, with which the T > 128
    inversions factor once per matrix instead of once per block column."""
    new = lambda m: torch.zeros((n, m, T, T), dtype=f64, device=dev)            # noqa: E731
    sh = {k: new(4) for k in ("X4", "RH4", "Z4", "Y4") + (("WK4",) if work else ())}
    sh.update({k: new(2) for k in ("S__", "S_", "Zs", "Y3") + (("WK2",) if work else ())})
    sh["i4"] = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    sh["i2"] = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    sh["rhs_on"] = torch.tensor([[1, 1, 0, 0]] * n, dtype=torch.int32, device=dev)
    return sh


class Chain:
    """A model's per-step lists as stacks with head-room, and everything one member step of it reads and writes."""
    __slots__ = _STACKS + ("T", "pos", "Nf", "n0", "W",          # from_model
                           "ws", "bad", "sync", "Y", "y_row0",   # the caller's: gathered previous state, status words, observations
                           "lv", "bufs",                         # build_lists
                           "bound")                              # bind_model

    def __init__(self, **fields):
        for k, v in fields.items():
            setattr(self, k, v)

    @classmethod
    def from_model(cls, gp, rows):
        """Stacks with room for `rows` rows holding the model's lists, its position and counters, and its two MNIW distributions
        (internal, observation) as one tensor: W[0] = means, W[1] = right covariances, W[2] = scales, each [2,T,T].  The
        parameter lists of a model with an estimation limit are shorter than its state lists: the rows behind them hold the
        last parameters, as the frozen finish (flag 8, include/hdpgpc_hip.h) leaves them."""
        T = gp.x_basis.shape[0]
        L = len(gp.f_star)
        dev = gp.device
        ch = cls(T=T)
        for key in _STACKS:
            shape = (T, 1) if key in ("F", "Fsm") else (T, T)
            buf = torch.empty((rows,) + shape, dtype=f64, device=dev)
            rows_ = getattr(gp, _LISTS[key]).stack()
            n = rows_.shape[0]
            buf[:n] = rows_.reshape((n,) + shape)
            if n < L:
                buf[n:L] = buf[n - 1]
            buf[L:].zero_()
            setattr(ch, key, buf)
        ch.pos = torch.tensor([L - 1], dtype=torch.int64, device=dev)
        ch.Nf = torch.tensor([float(gp.N)], dtype=f64, device=dev)
        ch.n0 = torch.tensor([float(gp.internal_params.n0)], dtype=f64, device=dev)
        eye = torch.eye(T, dtype=f64, device=dev)
        mi, mo = gp.internal_params, gp.observation_params
        ch.W = torch.stack((torch.stack((mi.m_mean, mo.m_mean)),
                            torch.stack((eye if mi.m_r_cov is None else mi.m_r_cov, eye if mo.m_r_cov is None else mo.m_r_cov)),
                            torch.stack((mi.scale, mo.scale)))).contiguous()
        return ch

    def stack_ptrs(self):
        return [getattr(self, k).data_ptr() for k in _STACKS]

    def more_rows(self, rows):
        """The stacks moved into new ones of `rows` rows."""
        for key in _STACKS:
            old = getattr(self, key)
            buf = torch.zeros((rows,) + tuple(old.shape[1:]), dtype=f64, device=old.device)
            buf[:old.shape[0]] = old
            setattr(self, key, buf)

    def bind_model(self, gp, L, n0, Lp=None):
        """The model's lists as views of the first L rows of the stacks (the four parameter lists: of the first Lp rows, default
        L; min(L, estimation limit) for a model that has one), its MNIW distributions as views of W with count n0.
        The only binder: kernels write the stacks and W in place, and NEW lists (new stamps, steplist.py) are what tells the model
        that they did - whoever lets a step write rows a model can see binds again."""
        Lp = L if Lp is None else Lp
        views = tuple(StepList(getattr(self, key)[:Lp if key in _PARAMS else L]) for key in _STACKS)
        for key, lst in zip(_STACKS, views):
            setattr(gp, _LISTS[key], lst)
        W = self.W
        gp.internal_params = matrix_normal_inv_wishart(W[0, 0], W[1, 0], n0, W[2, 0])
        gp.observation_params = matrix_normal_inv_wishart(W[0, 1], W[1, 1], n0, W[2, 1])
        self.bound = (views, gp.internal_params, gp.observation_params)

    def bound_to(self, gp):
        """Is the model still what the last bind_model(gp, ...) left: every list the very view handed out then and still a view
        (a mutation turns a list into a real one, an assignment replaces it), both MNIW distributions the objects over W?
        Identity checks only: this runs for every cluster at every beat of the online loop."""
        views, ip, op = self.bound
        if gp.internal_params is not ip or gp.observation_params is not op:
            return False
        for key, lst in zip(_STACKS, views):
            if getattr(gp, _LISTS[key]) is not lst or lst.stacked() is None:
                return False
        return True

    def build_lists(self, shared, c, alloc=None, frozen=False):
        """The member step as ONE launch per dependency level (hgp_chain.hip): every product of the step is an item of a
        device-resident list whose pointers are fixed for the life of the chain; the two inversions (hgp_inverse.hip) carry their
        right-hand sides.  14 launches per member, no torch arithmetic, no allocation (measured: a dependent launch costs ~4.5 us
        whatever it does, so launches - not flops - were the step's time).  128 < T <= 256: the inversions are the
        cooperative inverse-only kernels and Z rhs is one more list level behind each of them (16 launches).
        shared, c: this chain is chain c of shared_buffers (one batched inversion for all of them).  alloc(*shape) (optional):
        where the step's own buffers come from (a pool hands out slices of its arena); zeroed.  Needs self.ws.
        frozen: the step of a chain at its estimation limit (finish flag 8, member_step(..., frozen=True)): the same items in
        the same order minus what only the two MNIW updates consume - SINV, MS, S__, S_, part and the LV_RHS2 level."""
        T = self.T
        riding = T <= _ffi.MAX_T_WAVE
        dev = self.ws.device
        new = alloc or (lambda *shape: torch.zeros(shape, dtype=f64, device=dev))
        A, G, C, S, Psm, c0, m0, Fsm = (ws_view(self.ws, k, T) for k in _WS)
        X4, RH4, Z4, Y4 = (shared[k][c] for k in ("X4", "RH4", "Z4", "Y4"))   # [P, Sk, R0', R1'], riding RHS, Z, Z rhs
        S__, S_, Zs, Y3 = (shared[k][c] for k in ("S__", "S_", "Zs", "Y3"))
        part = new(2, T, T)
        AP0, Pk, K_t, J, SINV, IKC, KS, MS, T1, KKt, KKtmP, c_post, CmP, X, P_sm_prev = (
            new(T, T), new(T, T), new(T, T), new(T, T), new(2, T, T), new(T, T), new(T, T), new(2, T, T), new(T, T), new(T, T),
            new(T, T), new(T, T), new(T, T), new(T, T), new(T, T))
        y, xm, innov, f_post, w, f_sm_prev = new(T), new(T), new(T), new(T), new(T), new(T)
        means = self.W[0]
        P, Sk = X4[0], X4[1]
        lv = [ops.GemmList(dev) for _ in range(10)]
        # L1-L4: predictions (GPI.py:100-139; GPI.py:283-287 for the pair smoother's P = A c0 A^T + G)
        lv[0].add(A, Psm, AP0)
        lv[0].add(A, c0, RH4[0])                                  # A c0, the smoother gain's right-hand side
        lv[0].add(A, Fsm, xm)
        lv[1].add(AP0, A, Pk, D=G, transB=True)
        lv[1].add(RH4[0], A, P, D=G, transB=True)
        lv[1].add(C, xm, innov, D=y, alpha=-1.0)                  # y - C x_m
        lv[2].add(C, Pk, RH4[1])                                  # C P_k, the Kalman gain's right-hand side
        lv[3].add(RH4[1], C, Sk, D=S, transB=True)
        # after INV1 (Z = L^-1 of P, Sk, R0', R1';  Y = Z rhs):  K = (C Pk)^T Sk^-1 = Y1^T Z1,  J = (A c0)^T P^-1 = Y0^T Z0
        lv[4].add(Y4[1], Z4[1], K_t, transA=True)
        lv[4].add(Y4[0], Z4[0], J, transA=True)
        if not frozen:
            lv[4].add(Z4[2], Z4[2], SINV[0], transA=True)
            lv[4].add(Z4[3], Z4[3], SINV[1], transA=True)
        lv[5].add(K_t, innov, f_post, D=xm)
        lv[5].add(K_t, C, IKC, alpha=-1.0, add_eye=1.0)
        lv[5].add(K_t, S, KS)
        if not frozen:
            lv[5].add(means[0], SINV[0], MS[0])
            lv[5].add(means[1], SINV[1], MS[1])
        lv[6].add(IKC, Pk, T1)
        lv[6].add(KS, K_t, KKt, transB=True)
        lv[6].add(KS, K_t, KKtmP, D=P, transB=True, beta=-1.0)
        lv[6].add(A, m0, w, D=f_post, alpha=-1.0)                 # f_post - A m0
        lv[7].add(T1, IKC, c_post, D=KKt, transB=True)            # Joseph form (GPI.py:148-150)
        lv[7].add(T1, IKC, CmP, D=KKtmP, transB=True)             # c_post - P for the smoother
        lv[7].add(J, w, f_sm_prev, D=m0)
        lv[8].add(J, CmP, X)
        if not frozen:
            lv[8].add(f_sm_prev, f_sm_prev, S__[0], D=SINV[0], transB=True)  # y2 y2^T + R'^-1 (GPI_model.py:1317-1322)
            lv[8].add(f_post, f_post, S__[1], D=SINV[1], transB=True)
            lv[8].add(f_post, f_sm_prev, S_[0], D=MS[0], transB=True)        # y1 y2^T + M R'^-1
            lv[8].add(y, f_post, S_[1], D=MS[1], transB=True)
            # after INV2 (Zs of S__ + 1e-8 I;  Y3 = Zs S_^T):  S_ S__^-1 = Y3^T Zs
            lv[9].add(Y3[0], Zs[0], part[0], transA=True)
            lv[9].add(Y3[1], Zs[1], part[1], transA=True)
        lv[9].add(X, J, P_sm_prev, D=c0, transB=True)
        if not riding:
            lvy = [ops.GemmList(dev), ops.GemmList(dev)]          # levels LV_RHS4, LV_RHS2
            lvy[0].add(Z4[0], RH4[0], Y4[0])                     # Z_P (A c0)
            lvy[0].add(Z4[1], RH4[1], Y4[1])                     # Z_S (C P_k)
            lvy[1].add(Zs[0], S_[0], Y3[0], transB=True)         # Z_s S_^T
            lvy[1].add(Zs[1], S_[1], Y3[1], transB=True)
            lv += lvy[:1] if frozen else lvy
        self.lv = lv
        self.bufs = dict(X4=X4, RH4=RH4, Z4=Z4, Y4=Y4, S__=S__, S_=S_, Zs=Zs, Y3=Y3, part=part, y=y, f_post=f_post, c_post=c_post,
                         f_sm_prev=f_sm_prev, P_sm_prev=P_sm_prev, i4=shared["i4"][c], i2=shared["i2"][c])


def _same_entries(a, b):
    """Do two per-step lists hold the very same tensors (one stack behind both, or the same objects entry by entry)?"""
    if len(a) != len(b):
        return False
    sa, sb = getattr(a, "stacked", lambda: None)(), getattr(b, "stacked", lambda: None)()
    if sa is not None or sb is not None:
        return sa is sb
    return all(x is y for x, y in zip(a, b))


def bind_static(gp, Fsm, Psm, L):
    """bind_model's sibling for a STATIC model whose filter chain (hgp_static_chain_steps_f64) appended rows L .. to the stacks
    Fsm [rows,T,1] and Psm [rows,T,T], which hold the model's smoothed lists in their first L rows.  A static model has no
    smoother: the reference appends the same tensors to the filtered and the smoothed lists (GPI_model.py:317), so the new rows
    serve both.  Where the two lists held the same entries before (always, unless somebody assigned to one of them) one stack
    serves both lists; otherwise the filtered lists keep their own first L rows.  The four parameter lists keep their length and
    the MNIW objects are not touched."""
    for filt, sm, st in (("f_star", "f_star_sm", Fsm), ("cov_f", "cov_f_sm", Psm)):
        old_f, old_sm = getattr(gp, filt), getattr(gp, sm)
        shared = _same_entries(old_f, old_sm)
        if not shared:
            own = torch.cat([torch.stack(list(old_f)).reshape((L,) + tuple(st.shape[1:])), st[L:]])
        setattr(gp, sm, StepList(st))
        setattr(gp, filt, StepList(st if shared else own))


def gather_desc(ch):
    """hgp_chain_gather_desc of a chain; the step reads observation row pos - y_row0 of its Y (y_row0 < 0: Y is the observation
    itself)."""
    b = ch.bufs
    g = _ffi.ChainGatherDesc()
    for i, ptr in enumerate(ch.stack_ptrs()):
        g.st[i] = ptr
    g.pos, g.out, g.Y, g.y_out, g.W, g.Rp = _p(ch.pos), _p(ch.ws), _p(ch.Y), _p(b["y"]), _p(ch.W), _p(b["X4"][2:4])
    g.y_row0, g.T = ch.y_row0, ch.T
    return g


def finish_desc(ch, flags, bad):
    """hgp_chain_finish_desc of a chain; flags = its `annealing` field (include/hdpgpc_hip.h), bad = the status words it updates."""
    b = ch.bufs
    f = _ffi.ChainFinishDesc()
    f.f_post, f.c_post, f.f_sm_prev, f.P_sm_prev, f.y = _p(b["f_post"]), _p(b["c_post"]), _p(b["f_sm_prev"]), _p(b["P_sm_prev"]), _p(b["y"])
    f.part, f.Snew, f.info1, f.info2 = _p(b["part"]), _p(b["S__"]), _p(b["i4"]), _p(b["i2"])
    f.W, f.n0, f.Nf, f.bad_count = _p(ch.W), _p(ch.n0), _p(ch.Nf), _p(bad)
    f.stA, f.stG, f.stC, f.stS = _p(ch.A), _p(ch.G), _p(ch.C), _p(ch.S)
    f.stF, f.stFsm, f.stP, f.stPsm = _p(ch.F), _p(ch.Fsm), _p(ch.P), _p(ch.Psm)
    f.pos, f.sync, f.T, f.annealing = _p(ch.pos), _p(ch.sync), ch.T, flags
    return f


def upload_descs(structs, dev):
    """An array of descriptor structs as device bytes."""
    arr = (type(structs[0]) * len(structs))(*structs)
    return torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).to(dev)


def gather(gdev, lo, hi, T):
    """The gather launch of chains [lo, hi) of the descriptor array gdev: each chain's last state into its ws."""
    base = ctypes.c_void_p(gdev.data_ptr() + lo * ctypes.sizeof(_ffi.ChainGatherDesc))
    _ffi.check(_ffi.lib.hgp_lds_chain_gather2_batched_f64(base, hi - lo, T, ops._stream()), "chain_gather2_batched")


def member_step(levels, shared, gdev, fdev, lo, hi, T, gather_first=True, no_smoother=(), frozen=False):
    """One member step of chains [lo, hi), chain-major in every argument:
    levels.run(l, lo, hi) launches level l of those chains; shared: their shared_buffers; gdev / fdev: upload_descs of their
    gather / finish descriptors; gather_first=False: a gather() of this member was already issued; no_smoother: the chains of a
    step without the pair smoother, whose previous smoothed mean stands where f_sm_prev would; frozen: `levels` are
    build_lists(frozen=True) and fdev carries flag 8 - no second inversion, no LV_RHS2 level."""
    sh = lambda k: shared[k][lo:hi].flatten(0, 1) if k in shared else None          # noqa: E731
    riding = T <= _ffi.MAX_T_WAVE
    if gather_first:
        gather(gdev, lo, hi, T)
    for l in range(4):
        levels.run(l, lo, hi)
    if riding:
        ops.chol_inverse_rhs(sh("X4"), sh("Z4"), sh("RH4"), sh("Y4"), sh("i4"), rhs_on=sh("rhs_on"))
    else:
        ops.chol_inverse(sh("X4"), out=sh("Z4"), info=sh("i4"), work=sh("WK4"))
        levels.run(LV_RHS4, lo, hi)
    for l in range(4, 8):
        levels.run(l, lo, hi)
    for ch in no_smoother:
        ch.bufs["f_sm_prev"].copy_(ws_view(ch.ws, "Fsm", T))
    levels.run(8, lo, hi)
    if frozen:
        pass                      # S__ / S_ were not formed: nothing to invert
    elif riding:
        ops.chol_inverse_rhs(sh("S__"), sh("Zs"), sh("S_"), sh("Y3"), sh("i2"), rhs_trans=True, add_diag=1e-8)
    else:
        ops.chol_inverse(sh("S__"), 0.0, 1e-8, out=sh("Zs"), info=sh("i2"), work=sh("WK2"))
        levels.run(LV_RHS2, lo, hi)
    levels.run(9, lo, hi)
    base = ctypes.c_void_p(fdev.data_ptr() + lo * ctypes.sizeof(_ffi.ChainFinishDesc))
    _ffi.check(_ffi.lib.hgp_lds_chain_finish2_batched_f64(base, hi - lo, T, ops._stream()), "chain_finish2_batched")
