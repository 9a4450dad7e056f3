"""Tensor-level wrappers over the C-ABI.  torch tensors are device containers only: every function
takes fp64 CUDA (ROCm) tensors, enqueues HIP kernels on the current stream and returns tensors."""
import ctypes
import math
import os

import numpy as np
import torch

from . import _ffi

LOG2PI = math.log(2.0 * math.pi)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def env_flag(name):
    return os.environ.get(name, "0") not in ("", "0")


def _stream():
    # the raw handle of torch's current stream (torch.cuda.current_stream() builds a Stream object: 9 us per call, and the
    # online step makes hundreds of calls per beat)
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


class _PinnedRing:
    """Small host arrays (index lists, descriptor tables, K x K transition logs) go to the device through a ring of pinned
    staging buffers with asynchronous copies: torch.as_tensor(array, device=...) is a BLOCKING copy that first waits for
    everything queued on the stream - the online step made ~40 of them per beat, each one a hidden synchronisation."""
    SLOTS, NBYTES = 64, 1 << 16

    def __init__(self):
        self.bufs = [torch.empty(self.NBYTES, dtype=torch.uint8).pin_memory() for _ in range(self.SLOTS)]
        self.views = [b.numpy() for b in self.bufs]
        self.events = [None] * self.SLOTS
        self.i = 0


_ring = None
_NP_OF = {torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64, torch.uint8: np.uint8, torch.bool: np.bool_}


def to_dev(a, dtype, device):
    """A host array / list / CPU tensor as a device tensor of `dtype` without a stream synchronisation."""
    global _ring
    if torch.is_tensor(a):
        if a.is_cuda:
            return a.to(dtype=dtype).contiguous()
        a = a.numpy()
    arr = np.ascontiguousarray(a, dtype=_NP_OF[dtype])
    dev = torch.device(device)
    if dev.type != "cuda" or arr.nbytes == 0 or arr.nbytes > _PinnedRing.NBYTES:
        return torch.as_tensor(arr, dtype=dtype, device=device)
    if _ring is None:
        _ring = _PinnedRing()
    r = _ring
    i = r.i
    r.i = (i + 1) % r.SLOTS
    if r.events[i] is not None:
        r.events[i].synchronize()          # the copy that last used this slot (64 uploads ago) has long finished
    nb = arr.nbytes
    r.views[i][:nb] = arr.reshape(-1).view(np.uint8)
    out = torch.empty(arr.shape, dtype=dtype, device=device)
    out.view(-1).view(torch.uint8).copy_(r.bufs[i][:nb], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    r.events[i] = ev
    return out


def _dev64(t, name):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise TypeError(f"{name} must be a contiguous fp64 tensor on the GPU")
    return t


def _dev_i32(t, n, who, name, shape):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
        raise TypeError(f"{who}: {name} must be a contiguous int32 tensor [{shape}] on the GPU")
    return t


def _ragged_lengths(who, lengths, N, ld, dev):
    """lengths= of a ragged batch as an int32 device tensor [N]: host values are checked against [1, ld] here, device values are
    the kernels' to check (no synchronisation)."""
    if not torch.is_tensor(lengths) or not lengths.is_cuda:
        len_h = np.asarray(lengths.numpy() if torch.is_tensor(lengths) else lengths)
        if len_h.shape != (N,) or (N and (len_h.min() < 1 or len_h.max() > ld)):
            raise ValueError(f"{who}: lengths must be [{N}] with entries in [1, {ld}]")
    elif tuple(lengths.shape) != (N,):
        raise ValueError(f"{who}: lengths must be [{N}]")
    return to_dev(lengths, torch.int32, dev)


def raise_on_info(info, what):
    """Mirror torch.linalg.cholesky's error behaviour from a per-item LAPACK info tensor (host sync)."""
    host = info.reshape(-1).cpu()          # one copy (torch.nonzero on the device is three launches and a sync: 0.3 ms)
    bad = torch.nonzero(host)
    if bad.numel():
        i = int(bad[0, 0])
        raise torch.linalg.LinAlgError(
            f"{what}: (Batch element {i}): The factorization could not be completed because the input is not "
            f"positive-definite (the leading minor of order {int(host[i])} is not positive-definite).")


def gram_rbf(x, y, c, ell, noise=0.0):
    """a1: (ConstantKernel(c)*RBF(ell)+WhiteKernel(noise))(x, y); y=None is the one-argument call."""
    x = _dev64(x.reshape(-1), "x")
    yv = None if y is None else _dev64(y.reshape(-1), "y")
    ny = x.numel() if yv is None else yv.numel()
    K = torch.empty((x.numel(), ny), dtype=torch.float64, device=x.device)
    _ffi.check(_ffi.lib.hgp_gram_rbf_f64(_ptr(x), x.numel(), _ptr(yv), ny, c, ell, noise, _ptr(K), _stream()), "gram_rbf")
    return K


def potrf_batched(A, jitter_rel=1e-8, add_diag=0.0, want_inv=False, want_logdet=False):
    """a3: batched GPI_model._chol_spd.  A [b,T,T] (not modified).  Returns (L, info[, Linv][, logdet])."""
    A = _dev64(A, "A")
    if A.dim() == 2:
        A = A.unsqueeze(0)
    b, T, _ = A.shape
    L = A.clone()
    info = torch.zeros(b, dtype=torch.int32, device=A.device)
    Linv = torch.empty_like(L) if want_inv else None
    logdet = torch.empty(b, dtype=torch.float64, device=A.device) if want_logdet else None
    _ffi.check(_ffi.lib.hgp_potrf_batched_f64(_ptr(L), T, b, float(jitter_rel), float(add_diag), _ptr(Linv), _ptr(logdet),
                                              _ptr(info), _stream()), "potrf_batched")
    out = [L, info]
    if want_inv:
        out.append(Linv)
    if want_logdet:
        out.append(logdet)
    return tuple(out)


def chol_inverse(A, jitter_rel=0.0, add_diag=0.0, out=None, info=None, work=None):
    """Z = chol(0.5 (A + A^T) + shift I)^{-1} for a batch [b,T,T] (T <= 256; A untouched).  Returns (Z, info); `out` / `info`
    may be caller-allocated (capture-safe, no allocation).  work [b,T,T] (optional, T > 128): large batches factor once into
    it and take L^-1 from L (hgp_chol_inverse_ws_f64) instead of one factorisation per block column."""
    A = _dev64(A, "A")
    A3 = A if A.dim() == 3 else A.unsqueeze(0)
    b, T, _ = A3.shape
    Z = torch.empty_like(A3) if out is None else out
    if info is None:
        info = torch.zeros(b, dtype=torch.int32, device=A.device)
    if work is not None:
        if work.numel() < A3.numel():
            raise ValueError("chol_inverse: workspace smaller than the batch")
        _ffi.check(_ffi.lib.hgp_chol_inverse_ws_f64(_ptr(A3), T, b, float(jitter_rel), float(add_diag), _ptr(Z), _ptr(_dev64(work, "work")),
                                                    _ptr(info), _stream()), "chol_inverse_ws")
        return Z, info
    _ffi.check(_ffi.lib.hgp_chol_inverse_batched_f64(_ptr(A3), T, b, float(jitter_rel), float(add_diag), _ptr(Z), _ptr(info),
                                                     _stream()), "chol_inverse")
    return Z, info


def copy_list(items_dev, n_items, max_n):
    """n_items copies dst[0..n) = src[0..n) described by the device-resident int64 table items_dev [n_items, 3] = (src, dst, n),
    the layout of hgp_copy_item (_ffi.CopyItem)."""
    _ffi.check(_ffi.lib.hgp_copy_list_f64(_ptr(items_dev), int(n_items), int(max_n), _stream()), "copy_list")


MAX_CHUNK = 64  # segments per work item: one factorisation is reused for up to this many right-hand sides


def build_items(mat_of_group, add_of_group, group_sizes):
    """Split groups (segments sorted by group) into work items of at most MAX_CHUNK segments."""
    item_mat, item_add, item_off, item_cnt = [], [], [], []
    off = 0
    for m, a, n in zip(mat_of_group, add_of_group, group_sizes):
        done = 0
        while done < n:
            c = min(MAX_CHUNK, n - done)
            item_mat.append(m)
            item_add.append(a)
            item_off.append(off + done)
            item_cnt.append(c)
            done += c
        off += n
    return (np.asarray(item_mat, np.int32), np.asarray(item_add, np.float64), np.asarray(item_off, np.int32),
            np.asarray(item_cnt, np.int32))


def _up(a, dtype, dev):
    return None if a is None else to_dev(a, dtype, dev)


def _score_operands(Y, mean, Sigma, strides):
    """(Y, mean, Sigma, mean stride, Sigma stride) of the a4 / a6 calls: dense stacks mean [S,T], Sigma [S,T,T], checked here, or
    strides = (mean_stride, sigma_stride) in doubles: states that sit inside larger per-cluster records, taken as they are."""
    Y = _dev64(Y, "Y")
    T = Y.shape[1]
    if strides is not None:
        return Y, mean, Sigma, int(strides[0]), int(strides[1])
    Sigma = _dev64(Sigma, "Sigma")
    if Sigma.dim() == 2:
        Sigma = Sigma.unsqueeze(0)
    if mean is not None:
        mean = _dev64(mean.reshape(-1, T), "mean")
    return Y, mean, Sigma, T, T * T


def score_groups(Y, mean, Sigma, item_mat, item_add, item_off, item_cnt, seg_ids=None, jitter_rel=1e-8,
                 want_logdet=False, want_info=True, item_mean=None, strides=None):
    """a4+a6: quad[n] = (Y[n]-mean[s])^T cov_s^{-1} (Y[n]-mean[s]) for the segments of each work item.

    Y [N,T]; mean [S,T] or None; Sigma [S,T,T]; item_* host or device int/float arrays; seg_ids [sum cnt] or None.
    """
    Y, mean, Sigma, mstride, sstride = _score_operands(Y, mean, Sigma, strides)
    dev = Y.device
    N, T = Y.shape
    im, ia = _up(item_mat, torch.int32, dev), _up(item_add, torch.float64, dev)
    io, ic = _up(item_off, torch.int32, dev), _up(item_cnt, torch.int32, dev)
    sid, imean = _up(seg_ids, torch.int32, dev), _up(item_mean, torch.int32, dev)
    quad = torch.zeros(N, dtype=torch.float64, device=dev)
    logdet = torch.zeros(N, dtype=torch.float64, device=dev) if want_logdet else None
    info = torch.zeros(N, dtype=torch.int32, device=dev) if want_info else None
    _ffi.check(_ffi.lib.hgp_score_groups_f64(_ptr(Y), T, _ptr(mean), mstride, _ptr(Sigma), sstride, T, _ptr(im), _ptr(imean),
                                             _ptr(ia), _ptr(io), _ptr(ic), im.numel(), _ptr(sid), jitter_rel, _ptr(quad),
                                             _ptr(logdet), _ptr(info), _stream()), "score_groups")
    return quad, logdet, info


def score_each(Y, mean, Sigma, seg_mat, seg_mean=None, seg_add=None, jitter_rel=1e-8, want_logdet=False, want_info=True,
               symmetric=False, strides=None):
    """a6 for member segments: segment i against its own state.  Y [n,T]; mean [S,T]; Sigma [S,T,T]; seg_* [n].
    symmetric=True promises Sigma == Sigma^T exactly (upper triangle read only)."""
    Y, mean, Sigma, mstride, sstride = _score_operands(Y, mean, Sigma, strides)
    dev = Y.device
    n, T = Y.shape
    sm, sme, sa = _up(seg_mat, torch.int32, dev), _up(seg_mean, torch.int32, dev), _up(seg_add, torch.float64, dev)
    if T > _ffi.MAX_T_WAVE:   # cooperative kernels: one work item (one workgroup) per segment
        ar = torch.arange(n, dtype=torch.int32, device=dev)
        return score_groups(Y, mean, Sigma, sm, sa, ar, torch.ones(n, dtype=torch.int32, device=dev), jitter_rel=jitter_rel,
                            want_logdet=want_logdet, want_info=want_info, item_mean=sme, strides=strides)
    quad = torch.zeros(n, dtype=torch.float64, device=dev)
    logdet = torch.zeros(n, dtype=torch.float64, device=dev) if want_logdet else None
    info = torch.zeros(n, dtype=torch.int32, device=dev) if want_info else None
    _ffi.check(_ffi.lib.hgp_score_each_f64(_ptr(Y), T, _ptr(mean), mstride, _ptr(Sigma), sstride, T, _ptr(sm), _ptr(sme), _ptr(sa), n,
                                           jitter_rel, int(bool(symmetric)), _ptr(quad), _ptr(logdet), _ptr(info), _stream()),
               "score_each")
    return quad, logdet, info


class PairsPlan:
    """a2+a5 for an N x K batch: per-cluster operators (plan) + the per-pair kernels.

    acc_tol selects, per cluster and on the device, between the two evaluations of cov_f (hgp_pairs_plan_set_accuracy):
    clusters whose accuracy_bound() exceeds it (ill-conditioned K~, e.g. the drivers' ini_lengthscale = 3.0) are scored
    by the solve-based kernel (the reference's operation order, GPI.py:489-501); 0 = all clusters, < 0 = none.

    Segment-operator store (hgp_loglik_pairs_segops_f64, padded sizes 96 and 128): a sampler scores the same segments against
    changing cluster states, so loglik() keeps what the band kernel builds per segment - E blocks, K** tiles, band decision - in one
    device buffer per plan, for the (N, row length, device) of the last call; the kernels compare each record's key with the
    call's x, lengths and basis grid on the bits and rebuild what differs, so nothing is ever invalidated by hand.  The buffer
    costs about 75 KiB per segment and length-scale group at size 128 (56 KiB at 96); a batch that would need more than
    SEGOPS_MAX_BYTES (default 1 GiB: the headline batch of 2 048 segments takes 158 MB) is scored without a store, by the
    entries that build the operators inside the pair kernel."""

    SEGOPS_MAX_BYTES = 1 << 30

    def __init__(self, T, Ts_max, theta, device="cuda", acc_tol=1e-9):
        theta = np.ascontiguousarray(np.asarray(theta, dtype=np.float64).reshape(-1, 3))
        self.T, self.Ts_max, self.K = int(T), int(Ts_max), theta.shape[0]
        self.theta = theta
        nbytes = _ffi.lib.hgp_pairs_plan_device_bytes(self.T, self.Ts_max, self.K)
        if nbytes == 0:
            raise ValueError("bad plan shape")
        self._buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self._h = ctypes.c_void_p()
        self._score_out = False
        _ffi.check(_ffi.lib.hgp_pairs_plan_create(ctypes.byref(self._h), self.T, self.Ts_max, self.K,
                                                  theta.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  _ptr(self._buf), nbytes), "pairs_plan_create")
        self.info = torch.zeros(self.K, dtype=torch.int32, device=device)
        self._routed = False
        self._segops, self._segops_key = None, None
        self.set_accuracy(acc_tol)

    def set_accuracy(self, tol):
        """Threshold on accuracy_bound() above which a cluster takes the solve-based kernel (next update())."""
        self.acc_tol = float(tol)
        _ffi.check(_ffi.lib.hgp_pairs_plan_set_accuracy(self._h, self.acc_tol), "pairs_plan_set_accuracy")
        self._routed = False           # the per-cluster routing flags belong to the previous threshold until update() runs
        return self

    def update(self, x_basis, mean, Sigma):
        """x_basis [T]; mean [K,T] (= C f on the basis grid); Sigma [K,T,T]."""
        x_basis = _dev64(x_basis.reshape(-1), "x_basis")
        mean = _dev64(mean.reshape(self.K, self.T), "mean")
        Sigma = _dev64(Sigma.reshape(self.K, self.T, self.T), "Sigma")
        self._keep = (x_basis, mean, Sigma)
        _ffi.check(_ffi.lib.hgp_pairs_plan_update(self._h, _ptr(x_basis), _ptr(mean), _ptr(Sigma), _ptr(self.info),
                                                  _stream()), "pairs_plan_update")
        self._routed = True
        return self

    def scalars(self):
        """[K,8] device view: c, ell, noise, iso flag, mean diag Sigma, jitter, ||K~^-1||_inf, solve-based flag."""
        base = _ffi.lib.hgp_pairs_plan_scalars(self._h)
        off = base - self._buf.data_ptr()
        return self._buf[off:off + self.K * 64].view(torch.float64).view(self.K, 8)

    def accuracy_bound(self):
        """eps * (c ||K~^-1||_inf)^2 per cluster: growth of the rounding error of the explicit-operator evaluation
        relative to the reference's triangular solves (host sync).  ~1e-10 at the reference's length-scale.  The plan
        compares it with acc_tol on the device; nothing on the scoring path needs this host copy."""
        s = self.scalars().cpu().numpy()
        return np.finfo(np.float64).eps * (s[:, 0] * s[:, 6]) ** 2

    def solve_based(self):
        """Boolean [K] (host sync): clusters the last update() routed to the solve-based kernel."""
        return self.scalars()[:, 7].cpu().numpy() != 0.0

    def loglik(self, x, y, first_noise=None, want_logdet=True, want_info=True, sel=None, score=False, lengths=None):
        """x, y [N,Ts] -> (quad [N,K], logdet [N,K] or None, info [N,K] or None).

        lengths [N] int32 (optional; host array or device tensor): a ragged batch (hgp_loglik_pairs_ragged_f64).  x, y are then
        [N, ld] with segment n in the first lengths[n] entries of row n, 1 <= lengths[n] <= ld; the rest of a row is never read
        (ops.pad_ragged fills it with NaN).  Row n's outputs have the bits of loglik(x[n:n+1, :lengths[n]], y[n:n+1, :lengths[n]]).
        Host lengths outside [1, ld] raise ValueError; device lengths are not looked at on the host: such a row comes back as
        NaN / info = -1 and the others are unaffected.

        sel [N] int32 (optional): segment n is scored against cluster sel[n] only; outputs (and first_noise) are [N].
        score=True: the first output is the reference's score -0.5 quad - 0.5 Ts log(2 pi) (GPI_model.py:285), written by the
        kernels themselves (hgp_pairs_plan_set_score_output) - no arithmetic launch behind the pair kernels.
        Every output element is written by exactly one pair kernel: the buffers are not cleared first."""
        if not self._routed:
            raise RuntimeError("PairsPlan: update() must run after set_accuracy() / before the first loglik() - the kernels skip "
                               "clusters by the routing flags update() writes, and the outputs are not cleared")
        x = _dev64(x, "x")
        y = _dev64(y, "y")
        N, Ts = x.shape
        dev = x.device
        shape = (N,) if sel is not None else (N, self.K)
        if first_noise is not None:
            first_noise = _dev64(first_noise.reshape(shape), "first_noise")
        if sel is not None:
            # a selection outside [0, K) would leave its output element unwritten: host arrays are checked here, device arrays
            # get outputs that start as NaN / info = 1 (two fill launches on the per-segment path only)
            if not torch.is_tensor(sel) or not sel.is_cuda:
                sel_h = np.asarray(sel)
                if sel_h.size and (sel_h.min() < 0 or sel_h.max() >= self.K):
                    raise ValueError(f"PairsPlan.loglik: sel must lie in [0, {self.K})")
                quad = torch.empty(shape, dtype=torch.float64, device=dev)
                info = torch.empty(shape, dtype=torch.int32, device=dev) if want_info else None
            else:
                quad = torch.full(shape, float("nan"), dtype=torch.float64, device=dev)
                info = torch.ones(shape, dtype=torch.int32, device=dev) if want_info else None
            sel = to_dev(sel, torch.int32, dev)
        else:
            quad = torch.empty(shape, dtype=torch.float64, device=dev)
            info = torch.empty(shape, dtype=torch.int32, device=dev) if want_info else None
        logdet = torch.empty(shape, dtype=torch.float64, device=dev) if want_logdet else None
        if lengths is not None:
            lengths = _ragged_lengths("PairsPlan.loglik", lengths, N, Ts, dev)
        if bool(score) != self._score_out:
            _ffi.check(_ffi.lib.hgp_pairs_plan_set_score_output(self._h, int(bool(score))), "pairs_plan_set_score_output")
            self._score_out = bool(score)
        need = _ffi.lib.hgp_pairs_segops_bytes(self._h, N, Ts)
        if 0 < need <= self.SEGOPS_MAX_BYTES:
            if self._segops_key != (N, Ts, str(dev)) or self._segops.numel() < need:
                self._segops = None                      # the old store goes before the new one comes
                self._segops = torch.zeros(need, dtype=torch.uint8, device=dev)
                self._segops_key = (N, Ts, str(dev))
            _ffi.check(_ffi.lib.hgp_loglik_pairs_segops_f64(self._h, _ptr(self._segops), need, _ptr(x), _ptr(y), N, Ts, _ptr(lengths),
                                                            _ptr(first_noise), _ptr(sel), _ptr(quad), _ptr(logdet), _ptr(info),
                                                            _stream()), "loglik_pairs_segops")
            return quad, logdet, info
        if lengths is not None:
            _ffi.check(_ffi.lib.hgp_loglik_pairs_ragged_f64(self._h, _ptr(x), _ptr(y), N, Ts, _ptr(lengths), _ptr(first_noise),
                                                            _ptr(sel), _ptr(quad), _ptr(logdet), _ptr(info), _stream()),
                       "loglik_pairs_ragged")
            return quad, logdet, info
        _ffi.check(_ffi.lib.hgp_loglik_pairs_f64(self._h, _ptr(x), _ptr(y), N, Ts, _ptr(first_noise), _ptr(sel), _ptr(quad),
                                                 _ptr(logdet), _ptr(info), _stream()), "loglik_pairs")
        return quad, logdet, info

    def score(self, x, y, first_noise=None, sel=None, lengths=None):
        """The reference's score: -0.5 quad - 0.5 Ts log(2 pi)  (GPI_model.py:285, no log-determinant); with `lengths` (see
        loglik) Ts is each segment's own length."""
        q, _, info = self.loglik(x, y, first_noise, want_logdet=False, sel=sel, score=True, lengths=lengths)
        return q, info

    def device_bytes(self):
        """Device bytes this plan holds: its operator buffer and, once loglik() has made one, its segment-operator store."""
        return self._buf.numel() + (self._segops.numel() if self._segops is not None else 0)

    def close(self):
        if self._h:
            _ffi.lib.hgp_pairs_plan_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pad_ragged(xs, ys, device="cuda"):
    """Segments of different lengths as one ragged batch: xs, ys are lists of per-segment 1-D arrays (ys[n] may also be
    [len, D] for D leads) -> (X [N, ld], Y [N, ld] or [N, ld, D], lengths [N] int32) on the device, ld the longest segment, NaN
    in the padding (the kernels never read it: PairsPlan.loglik(..., lengths=))."""
    host = lambda a: np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)  # noqa: E731
    xs = [host(a).reshape(-1) for a in xs]
    ys = [host(a) for a in ys]
    if len(xs) != len(ys) or not xs:
        raise ValueError("pad_ragged: xs and ys must be non-empty lists of the same length")
    ys = [a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1) for a in ys]
    lens = np.array([a.shape[0] for a in xs], dtype=np.int32)
    tail = ys[0].shape[1:]
    if any(b.shape[0] != n or b.shape[1:] != tail for n, b in zip(lens, ys)) or lens.min() < 1:
        raise ValueError("pad_ragged: every segment needs a grid and values of one length >= 1 (and one number of leads)")
    ld = int(lens.max())
    X = np.full((len(xs), ld), np.nan)
    Y = np.full((len(xs), ld) + tail, np.nan)
    for n, (a, b) in enumerate(zip(xs, ys)):
        X[n, :lens[n]] = a
        Y[n, :lens[n]] = b
    return (torch.as_tensor(X, device=device), torch.as_tensor(Y, device=device), torch.as_tensor(lens, device=device))


_PLANS = {}                        # (device, T, Ts, K, theta) -> PairsPlan, in least-recently-used order
PLAN_CACHE_BYTES = 1 << 30         # device bytes the cached plans may hold together (the newest plan always stays)


def plan_cache(T, Ts, K, theta, device):
    """A PairsPlan for K clusters that share one theta, from a process-wide LRU cache bounded by PLAN_CACHE_BYTES.  Plans are
    stateless between calls as far as callers are concerned: every use starts with update()."""
    key = (str(device), int(T), int(Ts), int(K), tuple(theta))
    plan = _PLANS.pop(key, None)
    if plan is None:
        plan = PairsPlan(T, Ts, np.repeat(np.asarray(theta, dtype=np.float64)[None], int(K), 0), device=device)
    _PLANS[key] = plan                                     # most recently used = last
    total = sum(p.device_bytes() for p in _PLANS.values())
    for k in list(_PLANS):
        if total <= PLAN_CACHE_BYTES or k == key:
            break
        old = _PLANS.pop(k)
        total -= old.device_bytes()
        old.close()
        old._buf = old._segops = old._segops_key = None
    return plan


def gemm_batched(A, B, transA=False, transB=False, alpha=1.0, add=None, beta=1.0, out=None):
    """C[b] = alpha op(A[b]) op(B[b]) (+ beta add[b]) on v_mfma_f64_16x16x4_f64; A [b,m,k] (or [m,k]), B [b,k,n] (or [k,n]).
    add: optional [m,n] (shared by the batch) or [b,m,n] addend fused into the epilogue; out: optional preallocated
    contiguous [b,m,n] (or [m,n]) result."""
    A = _dev64(A, "A")
    B = _dev64(B, "B")
    a3 = A if A.dim() == 3 else A.unsqueeze(0)
    b3 = B if B.dim() == 3 else B.unsqueeze(0)
    batch = max(a3.shape[0], b3.shape[0])
    M, Kd = (a3.shape[2], a3.shape[1]) if transA else (a3.shape[1], a3.shape[2])
    N = b3.shape[1] if transB else b3.shape[2]
    sA = 0 if a3.shape[0] == 1 else a3.shape[1] * a3.shape[2]
    sB = 0 if b3.shape[0] == 1 else b3.shape[1] * b3.shape[2]
    if out is None:
        C = torch.empty((batch, M, N), dtype=torch.float64, device=A.device)
    else:
        C = out if out.dim() == 3 else out.unsqueeze(0)
        if tuple(C.shape) != (batch, M, N) or not C.is_contiguous() or C.dtype != torch.float64:
            raise ValueError("gemm_batched: out must be a contiguous float64 [batch, M, N]")
    if add is None:
        _ffi.check(_ffi.lib.hgp_gemm_batched_f64(int(transA), int(transB), M, N, Kd, alpha, _ptr(a3), a3.shape[2], sA, _ptr(b3),
                                                 b3.shape[2], sB, 0.0, _ptr(C), N, M * N, batch, _stream()), "gemm_batched")
    else:
        D = _dev64(add, "add")
        d3 = D if D.dim() == 3 else D.unsqueeze(0)
        if tuple(d3.shape[1:]) != (M, N) or d3.shape[0] not in (1, batch):
            raise ValueError("gemm_batched: add must be [M, N] or [batch, M, N]")
        sD = 0 if d3.shape[0] == 1 else M * N
        _ffi.check(_ffi.lib.hgp_gemm_add_batched_f64(int(transA), int(transB), M, N, Kd, alpha, _ptr(a3), a3.shape[2], sA, _ptr(b3),
                                                     b3.shape[2], sB, beta, _ptr(d3), N, sD, _ptr(C), N, M * N, batch, _stream()),
                   "gemm_add_batched")
    if out is not None:
        return out
    return C if (A.dim() == 3 or B.dim() == 3) else C[0]


def _kl_precisions(cov, what):
    """cov^-1 = Z^T Z with Z = chol(0.5 (cov + cov^T))^-1, no jitter (the reference's KL_divergence inverts the covariance
    as it is, GPI.py:1080-1081); a covariance that is not positive-definite raises, naming the state."""
    T = cov.shape[1]
    work = torch.empty_like(cov) if T > _ffi.MAX_T_WAVE else None
    Z, info = chol_inverse(cov, 0.0, 0.0, work=work)
    raise_on_info(info, f"kl_sym: covariance of {what}")
    return gemm_batched(Z, Z, transA=True)


def kl_sym(meanA, covA, meanB=None, covB=None):
    """a13: the symmetric Kullback-Leibler distance (GPI.py:1058-1094) between every Gaussian (meanA[i], covA[i]) and every
    (meanB[j], covB[j]); B omitted = A against itself (bitwise symmetric, zero diagonal up to rounding).  mean [n,T] (or
    [n,T,1]), cov [n,T,T].  Returns [nA,nB]; an entry depends on its own pair only (same bits in any call that holds it)."""
    covA = _dev64(covA, "covA")
    nA, T = covA.shape[0], covA.shape[-1]
    meanA = _dev64(meanA, "meanA").reshape(nA, T)
    if (meanB is None) != (covB is None):
        raise ValueError("kl_sym: meanB and covB go together")
    self_call = covB is None
    if not self_call:
        covB = _dev64(covB, "covB")
        if covB.shape[-1] != T:
            raise ValueError("kl_sym: the two sets of states live on different grids")
        meanB = _dev64(meanB, "meanB").reshape(covB.shape[0], T)
    nB = nA if self_call else covB.shape[0]
    out = torch.empty((nA, nB), dtype=torch.float64, device=covA.device)
    if nA == 0 or nB == 0:
        return out
    precA = _kl_precisions(covA, "state (first set)")
    precB = None if self_call else _kl_precisions(covB, "state (second set)")
    _ffi.check(_ffi.lib.hgp_kl_sym_f64(_ptr(meanA), _ptr(covA), _ptr(precA), nA, _ptr(meanB), _ptr(covB), _ptr(precB), nB, T,
                                       _ptr(out), _stream()), "kl_sym")
    return out


_WS = {}    # wrapper name -> {(device index, raw stream handle): fp64 workspace}


def _workspace(wrapper, dev, nbytes):
    """(workspace of at least nbytes bytes - what the library's size function returned - for `wrapper`'s entry point, current stream
    of dev).  One per wrapper and stream, so calls queued on different streams of a device never share buffers; it grows to the
    largest call seen and is kept until the wrapper's *_release() (pred_bands: S = 2 000 states at T = 90 hold 259 MB).  The key
    is the raw stream handle: a stream that is created, used for a call and destroyed leaves its entry behind until then."""
    with torch.cuda.device(dev):
        stream = _stream()
    cache = _WS.setdefault(wrapper, {})
    key = (dev.index, stream.value)
    ws = cache.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        ws = cache[key] = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    return ws, stream


def _release_of(wrapper):
    def release():
        _WS.pop(wrapper, None)
    release.__doc__ = f"Drop the cached workspaces of {wrapper} (the memory returns to torch's allocator once queued calls have finished)."
    return release


pred_bands_release, sample_release, kernel_fit_release, smacof_release, project_release = map(
    _release_of, ("pred_bands", "sample_states", "kernel_fit_steps", "smacof_steps", "project_ragged"))


def _stack_index(who, stack, what, idx, idx_name, S, check):
    """State s of S reads matrix idx[s] of the stack [*,T,T] (int32 device tensor [S]; None: s).  check: the values too (host sync)."""
    if idx is None:
        if stack.shape[0] != S:
            raise ValueError(f"{who}: without {idx_name} the stack holds one {what} per state")
        return
    _dev_i32(idx, S, who, idx_name, "S")
    if check and not bool(((idx >= 0) & (idx < stack.shape[0])).all()):
        raise IndexError(f"{who}: {idx_name} out of range")


def pred_bands_ws_doubles(S, T):
    """hgp_pred_bands_ws_bytes of include/hdpgpc_hip.h, in doubles."""
    return _ffi.lib.hgp_pred_bands_ws_bytes(S, T) // 8


def pred_bands(x_basis, theta, mean, Sigma, xq, sigma_idx=None, check=False):
    """a2 on a query grid for S states in one call (hgp_pred_bands_f64): what pred_dist returns as f_star and diag(cov_f).
    x_basis [T]; theta [S,3] = (c, ell, noise) per state (or one triple for all); mean [S,T]; Sigma a stack [*,T,T] of which
    state s reads Sigma[sigma_idx[s]] (int32 device tensor; None: s); xq [Q].  Returns (mean_q [S,Q], var_q [S,Q], info [S]);
    a state with info != 0 has NaN rows.  The values of sigma_idx must lie in [0, len(Sigma)): the kernels do not check them
    (an index outside reads outside the stack).  No synchronisation unless check=True, which validates sigma_idx on the host
    before the launch and raises on info after it.  The equal-grid short-circuit of GPI.py:467 is the caller's."""
    x_basis = _dev64(x_basis.reshape(-1), "x_basis")
    xq = _dev64(xq.reshape(-1), "xq")
    Sigma = _dev64(Sigma, "Sigma")
    T, Q, dev = x_basis.numel(), xq.numel(), x_basis.device
    if Sigma.dim() != 3 or tuple(Sigma.shape[1:]) != (T, T):
        raise ValueError("pred_bands: Sigma must be a stack [*, T, T] on the basis grid")
    mean = _dev64(mean, "mean")
    if mean.numel() % T:
        raise ValueError("pred_bands: mean must be [S, T]")
    mean = mean.reshape(-1, T)
    S = mean.shape[0]
    if not torch.is_tensor(theta):
        theta = to_dev(np.broadcast_to(np.asarray(theta, dtype=np.float64).reshape(-1, 3), (S, 3)), torch.float64, dev)
    theta = _dev64(theta, "theta")
    if tuple(theta.shape) != (S, 3):
        raise ValueError("pred_bands: theta must be [S, 3]")
    _stack_index("pred_bands", Sigma, "Sigma", sigma_idx, "sigma_idx", S, check and Q > 0)    # an empty call launches nothing
    mean_q = torch.empty((S, Q), dtype=torch.float64, device=dev)
    var_q = torch.empty((S, Q), dtype=torch.float64, device=dev)
    info = torch.zeros(S, dtype=torch.int32, device=dev)
    if S == 0 or Q == 0:
        return mean_q, var_q, info
    need = _ffi.lib.hgp_pred_bands_ws_bytes(S, T)
    ws, stream = _workspace("pred_bands", dev, need)
    _ffi.check(_ffi.lib.hgp_pred_bands_f64(_ptr(x_basis), T, _ptr(theta), _ptr(mean), _ptr(Sigma), _ptr(sigma_idx), S, _ptr(xq), Q,
                                           _ptr(mean_q), _ptr(var_q), _ptr(info), _ptr(ws), need, stream), "pred_bands")
    if check:
        raise_on_info(info, "pred_bands")
    return mean_q, var_q, info


def sample_ws_doubles(S, T):
    """hgp_sample_states_ws_bytes of include/hdpgpc_hip.h, in doubles."""
    return _ffi.lib.hgp_sample_states_ws_bytes(S, T) // 8


def sample_states(mean, cov, z, cov_idx=None, jitter_rel=0.0, check=True):
    """a14: draws from the Gaussians of S states in one call (hgp_sample_states_f64): out[s,j] = mean[s] + chol(A_s) z_j with
    A_s = 0.5 (cov_m + cov_m^T) + jitter_rel mean|diag cov_m| I, m = cov_idx[s] (int32 device tensor; None: s).
    mean [S,T]; cov a stack [*,T,T] (not modified); z standard normals, [n,T] shared by every state or [S,n,T].  Returns
    (out [S,n,T], info [S]); a state with info != 0 (failing pivot; -1: non-finite diagonal) has NaN draws, the others are
    unaffected.  The values of cov_idx must lie in [0, len(cov)): the kernels do not check them.  No synchronisation unless
    check=True, which validates cov_idx on the host before the launch and raises on info after it."""
    cov = _dev64(cov, "cov")
    if cov.dim() != 3 or cov.shape[1] != cov.shape[2]:
        raise ValueError("sample_states: cov must be a stack [*, T, T]")
    T, dev = cov.shape[1], cov.device
    mean = _dev64(mean, "mean")
    if T == 0 or mean.numel() % T:
        raise ValueError("sample_states: mean must be [S, T]")
    mean = mean.reshape(-1, T)
    S = mean.shape[0]
    z = _dev64(z, "z")
    if z.dim() not in (2, 3) or z.shape[-1] != T or (z.dim() == 3 and z.shape[0] != S):
        raise ValueError("sample_states: z must be [n, T] (shared) or [S, n, T]")
    n = z.shape[-2]
    _stack_index("sample_states", cov, "covariance", cov_idx, "cov_idx", S, check and n > 0)  # an empty call launches nothing
    out = torch.empty((S, n, T), dtype=torch.float64, device=dev)
    info = torch.zeros(S, dtype=torch.int32, device=dev)
    if S == 0 or n == 0:
        return out, info
    need = _ffi.lib.hgp_sample_states_ws_bytes(S, T)
    ws, stream = _workspace("sample_states", dev, need)
    _ffi.check(_ffi.lib.hgp_sample_states_f64(_ptr(mean), _ptr(cov), _ptr(cov_idx), T, S, _ptr(z), n, int(z.dim() == 2),
                                              float(jitter_rel), _ptr(out), _ptr(info), _ptr(ws), need, stream), "sample_states")
    if check:
        raise_on_info(info, "sample_states")
    return out, info


def kernel_fit_ws_doubles(B, T):
    """hgp_kernel_fit_ws_bytes of include/hdpgpc_hip_fit.h, in doubles."""
    return _ffi.lib.hgp_kernel_fit_ws_bytes(B, T) // 8


def kernel_fit_steps(x, Y, bounds, state, status, n_steps, lr=0.1, min_iter=1000, max_iter=4000, loss_out=None):
    """8f-2, batched (hgp_kernel_fit_steps_f64): advance every running fit of Y [B,T] by up to n_steps Adam iterations, in place
    in state [B, FIT_STATE_DOUBLES] / status [B] (int32; all zeros = the start of a fit).  x [T] (one grid for all) or [B,T];
    bounds [B,2] = the noise interval of each fit; loss_out (optional) [B, ld]: iteration it writes column it - 1.
    Nothing is synchronised and nothing returns to the host."""
    Y = _dev64(Y, "Y")
    if Y.dim() != 2:
        raise ValueError("kernel_fit_steps: Y must be [B, T]")
    B, T = Y.shape
    x = _dev64(x, "x")
    if tuple(x.shape) not in ((T,), (B, T)):
        raise ValueError("kernel_fit_steps: x must be [T] or [B, T]")
    bounds, state = _dev64(bounds, "bounds"), _dev64(state, "state")
    if tuple(bounds.shape) != (B, 2) or tuple(state.shape) != (B, _ffi.FIT_STATE_DOUBLES):
        raise ValueError("kernel_fit_steps: bounds must be [B, 2] and state [B, FIT_STATE_DOUBLES]")
    _dev_i32(status, B, "kernel_fit_steps", "status", "B")
    ld = 0
    if loss_out is not None:
        loss_out = _dev64(loss_out, "loss_out")
        if loss_out.dim() != 2 or loss_out.shape[0] != B:
            raise ValueError("kernel_fit_steps: loss_out must be [B, ld]")
        ld = loss_out.shape[1]
    if B == 0 or n_steps == 0:
        return
    need = _ffi.lib.hgp_kernel_fit_ws_bytes(B, T)
    ws, stream = _workspace("kernel_fit_steps", Y.device, need)
    _ffi.check(_ffi.lib.hgp_kernel_fit_steps_f64(_ptr(x), 0 if x.dim() == 1 else T, _ptr(Y), T, B, _ptr(bounds), float(lr), int(n_steps),
                                                 int(min_iter), int(max_iter), _ptr(state), _ptr(status),
                                                 _ptr(loss_out) if ld else None, ld, _ptr(ws), need, stream), "kernel_fit_steps")


def smacof_ws_doubles(B, n, p):
    """hgp_smacof_ws_bytes of include/hdpgpc_hip_mds.h, in doubles."""
    return _ffi.lib.hgp_smacof_ws_bytes(B, n, p) // 8


def smacof_steps(delta, X, state, status, stress, n_iter, n_steps, eps=1e-6, max_iter=300):
    """a15 (hgp_smacof_steps_f64): advance every running start of X [B,n,p] (p = 1..3) on the distance matrix delta [n,n] (a
    row-strided view [n, ld >= n] is taken as it is) by up to n_steps SMACOF passes, in place in X, state [B, MDS_STATE_DOUBLES]
    and status [B] (int32; all zeros = the beginning).  A start that ends (status 1: stop rule, 2: max_iter, -2: non-finite
    stress) leaves scikit-learn's X, stress [B] and n_iter [B] (int32); one that ends at max_iter has run max_iter + 1 passes.
    Nothing is synchronised and nothing returns to the host."""
    if not (torch.is_tensor(delta) and delta.is_cuda and delta.dtype == torch.float64 and delta.dim() == 2
            and delta.shape[0] == delta.shape[1] and delta.shape[0] >= 1 and (delta.shape[0] == 1 or delta.stride(1) == 1)
            and delta.stride(0) >= delta.shape[1]):
        raise ValueError("smacof_steps: delta must be a square fp64 matrix on the GPU with unit column stride")
    n = delta.shape[0]
    ld = delta.stride(0) if n > 1 else max(delta.stride(0), 1)
    X = _dev64(X, "X")
    if X.dim() != 3 or X.shape[1] != n or not 1 <= X.shape[2] <= 3:
        raise ValueError("smacof_steps: X must be [B, n, p] with p = 1, 2 or 3")
    B, _, p = X.shape
    state, stress = _dev64(state, "state"), _dev64(stress, "stress")
    if tuple(state.shape) != (B, _ffi.MDS_STATE_DOUBLES) or stress.numel() != B:
        raise ValueError("smacof_steps: state must be [B, MDS_STATE_DOUBLES] and stress [B]")
    _dev_i32(status, B, "smacof_steps", "status", "B")
    _dev_i32(n_iter, B, "smacof_steps", "n_iter", "B")
    if n_steps < 0:
        raise ValueError("smacof_steps: n_steps < 0")
    if B == 0 or n_steps == 0:
        return
    need = _ffi.lib.hgp_smacof_ws_bytes(B, n, p)
    ws, stream = _workspace("smacof_steps", X.device, need)
    _ffi.check(_ffi.lib.hgp_smacof_steps_f64(_ptr(delta), int(ld), n, p, B, _ptr(X), float(eps), int(n_steps), int(max_iter), _ptr(state),
                                             _ptr(status), _ptr(stress), _ptr(n_iter), _ptr(ws), need, stream), "smacof_steps")


def project_ragged(x, y, lengths, xb, c, ell, jitter=1e-4):
    """IterativeGaussianProcess.project_y (GPI.py:194-238, C = I) for a ragged batch in one call (hgp_project_ragged_f64):
    yp[n] = K(xb, x_n) (K(x_n, x_n) + jitter I)^-1 y_n with the two-argument kernel c * RBF(ell) (no white noise).

    x [N, ld], y [N, ld, D] (or [N, ld]: one lead) with segment n in the first lengths[n] entries of row n; lengths [N] int32
    (host array or device tensor; None: every row has ld points); xb [T], T and ld <= 256.  The rest of a row is never read
    (ops.pad_ragged fills it with NaN).  Returns (yp [N, T, D] or [N, T], info [N] int32).  A row of T points whose grid is xb bit
    for bit is copied (info 0); a row whose matrix is not positive definite has info > 0 and NaN values (raise_on_info raises
    on it); no row affects another.  Host lengths outside [1, ld] raise ValueError; device lengths are not looked at on the host:
    such a row comes back as NaN / info = -1."""
    x = _dev64(x, "x")
    y = _dev64(y, "y")
    xb = _dev64(xb.reshape(-1), "xb")
    if x.dim() != 2 or y.dim() not in (2, 3) or tuple(y.shape[:2]) != tuple(x.shape):
        raise ValueError("project_ragged: x must be [N, ld] and y [N, ld] or [N, ld, D]")
    N, ld = x.shape
    D = 1 if y.dim() == 2 else y.shape[2]
    T, dev = xb.numel(), x.device
    if lengths is not None:
        lengths = _ragged_lengths("project_ragged", lengths, N, ld, dev)
    yp = torch.empty((N, T) if y.dim() == 2 else (N, T, D), dtype=torch.float64, device=dev)
    info = torch.empty(N, dtype=torch.int32, device=dev)
    if N == 0:
        return yp, info
    need = int(_ffi.lib.hgp_project_ragged_ws_bytes(N, ld, T, D))
    ws = None
    if need:
        ws, stream = _workspace("project_ragged", dev, need)
    else:
        with torch.cuda.device(dev):
            stream = _stream()
    _ffi.check(_ffi.lib.hgp_project_ragged_f64(_ptr(x), _ptr(y), _ptr(lengths), N, ld, D, _ptr(xb), T, float(c), float(ell),
                                               float(jitter), _ptr(yp), _ptr(info), _ptr(ws), need, stream), "project_ragged")
    return yp, info


def static_chain_ws_doubles(B, T):
    """hgp_static_chain_ws_bytes of include/hdpgpc_hip_static.h, in doubles."""
    return _ffi.lib.hgp_static_chain_ws_bytes(B, T) // 8


def static_chain_desc(A, C, Sigma, Fs, Ps, pos, Y, y_idx, info, n, pos0, first=False, white=0.0, flags=0):
    """hgp_static_chain_desc of one chain (include/hdpgpc_hip_static.h): device tensors A, C, Sigma [T,T], the stacks Fs [rows,T]
    and Ps [rows,T,T] with rows >= pos0 + n + 1, pos [1] int64, Y [*,T], y_idx [n] int64, info [1] int32.  The tensors must outlive
    the calls that read the descriptor."""
    T = A.shape[-1]
    for t, name, shape in ((A, "A", (T, T)), (C, "C", (T, T)), (Sigma, "Sigma", (T, T))):
        if tuple(_dev64(t, name).shape) != shape:
            raise ValueError(f"static_chain_desc: {name} must be [T, T]")
    Fs, Ps, Y = _dev64(Fs, "Fs"), _dev64(Ps, "Ps"), _dev64(Y, "Y")
    rows = Ps.shape[0]
    if Fs.numel() != rows * T or tuple(Ps.shape[1:]) != (T, T) or Y.dim() != 2 or Y.shape[1] != T:
        raise ValueError("static_chain_desc: Fs must be [rows, T], Ps [rows, T, T] and Y [*, T]")
    if not 0 <= pos0 or pos0 + n + 1 > rows:
        raise ValueError("static_chain_desc: the stacks need pos0 + n + 1 rows")
    for t, name, dt, cnt in ((pos, "pos", torch.int64, 1), (y_idx, "y_idx", torch.int64, n), (info, "info", torch.int32, 1)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= cnt):
            raise TypeError(f"static_chain_desc: {name} must be a contiguous {dt} tensor on the GPU")
    d = _ffi.StaticChainDesc()
    d.A, d.C, d.Sigma, d.Fs, d.Ps, d.pos, d.Y, d.y_idx, d.info = (t.data_ptr() for t in (A, C, Sigma, Fs, Ps, pos, Y, y_idx, info))
    d.white, d.pos0, d.n, d.first, d.flags, d.reserved = float(white), int(pos0), int(n), int(bool(first)), int(flags), 0
    return d


def static_chain_steps(descs_dev, B, T, max_steps):
    """Up to max_steps members of each of the B static filter chains whose descriptors (static_chain_desc, uploaded as one array:
    member_step.upload_descs) lie in descs_dev - ONE launch (hgp_static_chain_steps_f64); T <= 128, NotImplementedError above.
    Nothing is synchronised; the workspace is kept per stream (static_chain_release drops it)."""
    if not (torch.is_tensor(descs_dev) and descs_dev.is_cuda and descs_dev.dtype == torch.uint8 and descs_dev.is_contiguous()
            and descs_dev.numel() >= B * ctypes.sizeof(_ffi.StaticChainDesc)):
        raise TypeError("static_chain_steps: descs_dev must hold B descriptors as bytes on the GPU")
    if B == 0 or max_steps == 0:
        return
    need = int(_ffi.lib.hgp_static_chain_ws_bytes(B, T))
    ws, stream = _workspace("static_chain_steps", descs_dev.device, max(need, 8))
    _ffi.check(_ffi.lib.hgp_static_chain_steps_f64(_ptr(descs_dev), int(B), int(T), int(max_steps), _ptr(ws), need, stream),
               "static_chain_steps")


static_chain_release = _release_of("static_chain_steps")


def rts_chain(J, P, AM, M, Cv):
    """Sequential part of the RTS smoother for all steps in one launch (in place on M [n,T] and Cv [n,T,T]); T <= 96."""
    n, T = M.shape[0], Cv.shape[1]
    _ffi.check(_ffi.lib.hgp_rts_chain_f64(_ptr(J), _ptr(P), _ptr(AM), _ptr(M), _ptr(Cv), n, T, _stream()), "rts_chain")


def _matrix_lik_ws(T, b, dev):
    """(workspace, its bytes) of the a8 / a9 calls: none for T <= HGP_MAX_T_WAVE, where each term is one fused kernel."""
    nws = _ffi.lib.hgp_matrix_lik_ws_bytes(T, b) if T > _ffi.MAX_T_WAVE else 0
    return (torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None), nws


def lat_error(f_cur, f_prev, A, Gamma, covprev):
    """a8 batched: returns (-0.5 (mahal + trace) [b], info [b]); the caller adds -0.5 T log 2pi."""
    f_cur, f_prev = _dev64(f_cur, "f_cur"), _dev64(f_prev, "f_prev")
    A, Gamma, covprev = _dev64(A, "A"), _dev64(Gamma, "Gamma"), _dev64(covprev, "covprev")
    b, T = f_cur.shape
    out = torch.empty(b, dtype=torch.float64, device=A.device)
    info = torch.zeros(b, dtype=torch.int32, device=A.device)
    ws, nws = _matrix_lik_ws(T, b, A.device)
    _ffi.check(_ffi.lib.hgp_lat_error_f64(_ptr(f_cur), _ptr(f_prev), _ptr(A), _ptr(Gamma), _ptr(covprev), T, b, _ptr(out),
                                          _ptr(info), _ptr(ws), nws, _stream()), "lat_error")
    return out, info


def mniw_loglik(M, Sigma, m_mean, m_r_cov, scale, scale_is_diagonal=None):
    """a9 batched.  M, Sigma [b,T,T]; prior (m_mean, scale, optional m_r_cov) [T,T] shared or [b,T,T] per item.
    scale_is_diagonal: None = check it here (one device comparison, host sync); callers that know (the hot path's
    prior scale is sigma I) pass True / False."""
    M, Sigma = _dev64(M, "M"), _dev64(Sigma, "Sigma")
    b, T, _ = M.shape
    m_mean, scale = _dev64(m_mean, "m_mean"), _dev64(scale, "scale")
    stride = 0 if m_mean.dim() == 2 else T * T
    if scale_is_diagonal is None:
        scale_is_diagonal = bool(torch.equal(scale, torch.diag_embed(torch.diagonal(scale, dim1=-2, dim2=-1))))
    if m_r_cov is not None:
        m_r_cov = _dev64(m_r_cov, "m_r_cov")
    out = torch.empty(b, dtype=torch.float64, device=M.device)
    info = torch.zeros(b, dtype=torch.int32, device=M.device)
    ws, nws = _matrix_lik_ws(T, b, M.device)
    _ffi.check(_ffi.lib.hgp_mniw_loglik_f64(_ptr(M), _ptr(Sigma), _ptr(m_mean), _ptr(m_r_cov), _ptr(scale), int(scale_is_diagonal), stride, T, b,
                                            _ptr(out), _ptr(info), _ptr(ws), nws, _stream()), "mniw_loglik")
    return out, info


def warp_cov(x, rho, omega, diag_add, normalize=True):
    x = _dev64(x.reshape(-1), "x")
    K = torch.empty((x.numel(), x.numel()), dtype=torch.float64, device=x.device)
    _ffi.check(_ffi.lib.hgp_warp_cov_f64(_ptr(x), x.numel(), rho, omega, diag_add, int(bool(normalize)), _ptr(K), _stream()),
               "warp_cov")
    return K


def chol_rank1(L, v, alpha=None, beta=None):
    """config 5: chol(alpha L L^T + beta v v^T) by a rank-1 update (O(T^2)), batched; returns (L_new, info)."""
    L = _dev64(L, "L")
    L3 = (L if L.dim() == 3 else L.unsqueeze(0)).clone()
    b, T, _ = L3.shape
    v = _dev64(v.reshape(b, T), "v")
    al = None if alpha is None else torch.as_tensor(alpha, dtype=torch.float64, device=L.device).reshape(b).contiguous()
    be = None if beta is None else torch.as_tensor(beta, dtype=torch.float64, device=L.device).reshape(b).contiguous()
    info = torch.zeros(b, dtype=torch.int32, device=L.device)
    _ffi.check(_ffi.lib.hgp_chol_rank1_f64(_ptr(L3), _ptr(v), _ptr(al), _ptr(be), T, b, _ptr(info), _stream()), "chol_rank1")
    return (L3 if L.dim() == 3 else L3[0]), info


class GemmList:
    """A device-resident list of products  C = alpha op(A) op(B) + beta D (+ add_eye I), run as ONE launch (hgp_gemm_list_f64).
    Built once from tensors whose storage outlives the list; `add` takes tensors (2-D, or 1-D read as a column)."""

    def __init__(self, device):
        self.device = device
        self._items, self._keep, self.tiles, self._item_tiles = [], [], 0, []
        self._dev = self._map = None

    @staticmethod
    def _dims(t):
        if t.dim() == 1:
            if t.numel() > 1 and t.stride(0) != 1:
                raise ValueError("gemm list vectors must be contiguous (a strided 1-D view would be read as a column of stride 1)")
            return t.shape[0], 1, 1
        if t.stride(-1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
            raise ValueError("gemm list operands must have unit inner stride and non-overlapping rows")
        return t.shape[0], t.shape[1], t.stride(0)

    def add(self, A, B, out, D=None, transA=False, transB=False, alpha=1.0, beta=1.0, add_eye=0.0, out2=None):
        ar, ac, lda = self._dims(A)
        br, bc, ldb = self._dims(B)
        M, K = (ac, ar) if transA else (ar, ac)
        K2, N = (bc, br) if transB else (br, bc)
        orow, ocol, ldc = self._dims(out)
        if K != K2 or (orow, ocol) != (M, N) or max(M, N, K) > 256:
            raise ValueError(f"gemm list item {M}x{K} . {K2}x{N} -> {orow}x{ocol}")
        ldd = 0
        if D is not None:
            dr, dc, ldd = self._dims(D)
            if (dr, dc) != (M, N):
                raise ValueError("gemm list addend shape")
        if out2 is not None and self._dims(out2) != (orow, ocol, ldc):
            raise ValueError("gemm list second output must match the first")
        for t in (A, B, out, D, out2):
            if t is not None:
                _dev64_any(t)
                self._keep.append(t)
        it = _ffi.GemmItem(A.data_ptr(), B.data_ptr(), D.data_ptr() if D is not None else None, out.data_ptr(),
                           out2.data_ptr() if out2 is not None else None, M, N, K, lda, ldb, ldc, ldd, int(transA), int(transB),
                           float(alpha), float(beta), float(add_eye))
        self._items.append(it)
        self._item_tiles.append(((M + 15) // 16) * ((N + 15) // 16))
        self.tiles += self._item_tiles[-1]
        self._dev = None
        return out

    @classmethod
    def concat(cls, lists):
        """One list holding the items of several lists, in order (chain_batch: one launch per level for many chains)."""
        out = cls(lists[0].device)
        for l_ in lists:
            out._items += l_._items
            out._keep += l_._keep
            out._item_tiles += l_._item_tiles
            out.tiles += l_.tiles
        return out

    def finalize(self):
        arr = (_ffi.GemmItem * len(self._items))(*self._items)
        host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
        self._dev = host.to(self.device)
        self._map = None
        # per-tile map instead of the per-wave walk over the list (one dependent load per item: 7.8 vs 6.9 us for a 5-item level of one
        # chain under rocprofv3, tools/time_gemm_list.py); 16-bit item index, longer lists walk
        if 1 < len(self._items) <= 65535:
            m = np.concatenate([(i << 16) | np.arange(n, dtype=np.uint32) for i, n in enumerate(self._item_tiles)]).astype(np.uint32)
            self._map = torch.from_numpy(m.view(np.int32)).to(self.device)
            self._cum = np.concatenate([[0], np.cumsum(self._item_tiles)])
        return self

    def run(self):
        if self._dev is None:
            self.finalize()
        if self._map is not None:
            _ffi.check(_ffi.lib.hgp_gemm_list_mapped_f64(_ptr(self._dev), len(self._items), _ptr(self._map), self.tiles, _stream()),
                       "gemm_list_mapped")
            return
        _ffi.check(_ffi.lib.hgp_gemm_list_f64(_ptr(self._dev), len(self._items), self.tiles, _stream()), "gemm_list")

    def run_range(self, first, count):
        """One launch over the items [first, first + count) of the list (a long list holding the levels of many steps)."""
        if self._dev is None:
            self.finalize()
        if self._map is not None and first == 0:
            _ffi.check(_ffi.lib.hgp_gemm_list_mapped_f64(_ptr(self._dev), int(count), _ptr(self._map), int(self._cum[count]), _stream()),
                       "gemm_list_mapped")
            return
        base = ctypes.c_void_p(self._dev.data_ptr() + first * ctypes.sizeof(_ffi.GemmItem))
        _ffi.check(_ffi.lib.hgp_gemm_list_f64(base, int(count), sum(self._item_tiles[first:first + count]), _stream()), "gemm_list")


def _dev64_any(t):
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64):
        raise TypeError("gemm list operands must be fp64 tensors on the GPU")


def chol_inverse_rhs(A, Linv, rhs, rhs_out, info, rhs_on=None, rhs_trans=False, jitter_rel=0.0, add_diag=0.0):
    """Z = chol(0.5 (A + A^T) + shift I)^{-1} -> Linv and Y = Z op(rhs) -> rhs_out from ONE factorisation per matrix of the batch
    [b,T,T] (T <= 128), all outputs caller-allocated (capture-safe, no allocation)."""
    A = _dev64(A, "A")
    b, T, _ = A.shape
    _ffi.check(_ffi.lib.hgp_chol_inverse_rhs_batched_f64(_ptr(A), T, b, float(jitter_rel), float(add_diag), _ptr(Linv), _ptr(rhs),
                                                         _ptr(rhs_on), int(bool(rhs_trans)), _ptr(rhs_out), _ptr(info), _stream()),
               "chol_inverse_rhs")


def trsv_lower_quad(G, y):
    """|| tril(G)^{-1} y ||^2 (a10 as written in the reference)."""
    G, y = _dev64(G, "G"), _dev64(y.reshape(-1), "y")
    out = torch.empty(1, dtype=torch.float64, device=G.device)
    _ffi.check(_ffi.lib.hgp_trsv_lower_quad_f64(_ptr(G), G.shape[1], _ptr(y), y.numel(), _ptr(out), _stream()), "trsv_lower_quad")
    return out[0]


def trsv_lower_solve(G, y):
    """alpha = tril(G)^{-T} tril(G)^{-1} y and || tril(G)^{-1} y ||^2  (the reference's cho_solve((K, True), y), GPI.py:1043)."""
    G, y = _dev64(G, "G"), _dev64(y.reshape(-1), "y")
    alpha = torch.empty_like(y)
    quad = torch.empty(1, dtype=torch.float64, device=G.device)
    _ffi.check(_ffi.lib.hgp_trsv_lower_solve_f64(_ptr(G), G.shape[1], _ptr(y), y.numel(), _ptr(alpha), _ptr(quad), _stream()),
               "trsv_lower_solve")
    return alpha, quad[0]


def lml_grad(x, alpha, Kinv, c, ell, noise):
    """a10 gradient w.r.t. (log c, log ell, log noise): 0.5 tr((alpha alpha^T - Kinv) dK/dtheta)  (GPI.py:1046-1051)."""
    x, alpha, Kinv = _dev64(x.reshape(-1), "x"), _dev64(alpha.reshape(-1), "alpha"), _dev64(Kinv, "Kinv")
    out = torch.empty(3, dtype=torch.float64, device=x.device)
    _ffi.check(_ffi.lib.hgp_lml_grad_f64(_ptr(x), _ptr(alpha), _ptr(Kinv), x.numel(), float(c), float(ell), float(noise), _ptr(out),
                                         _stream()), "lml_grad")
    return out



def hmm_messages(q, log_pi, log_trans, want_pair=True):
    """forward / backward messages of the switching variable and the log pair responsibilities
    (GPI_HDP.forward, backward, coupled_state_coef).  q [N,K] log-observations; returns (fmsg, marg, bmsg, log_resp_pair)."""
    q, log_pi, log_trans = _dev64(q, "q"), _dev64(log_pi.reshape(-1), "log_pi"), _dev64(log_trans, "log_trans")
    N, K = q.shape
    fmsg = torch.empty((N, K), dtype=torch.float64, device=q.device)
    marg = torch.empty(N, dtype=torch.float64, device=q.device)
    bmsg = torch.empty((N, K), dtype=torch.float64, device=q.device)
    pair = torch.empty((N, K, K), dtype=torch.float64, device=q.device) if want_pair else None
    _ffi.check(_ffi.lib.hgp_hmm_messages_f64(_ptr(q), _ptr(log_pi), _ptr(log_trans), N, K, _ptr(fmsg), _ptr(marg), _ptr(bmsg),
                                             _ptr(pair), _stream()), "hmm_messages")
    return fmsg, marg, bmsg, pair


def hmm_local_terms(Q, log_pi, log_trans, want_pair=True):
    """The local step of the switching variable for a batch of score matrices Q [B,N,K] sharing log_pi / log_trans
    (hgp_hmm_local_terms_f64): LogLik normalisation, messages and hard assignment per matrix.  Returns device tensors
    (labels [B,N] int64, pair_first [B,N] int64 or None, last_log [B,K])."""
    Q, log_pi, log_trans = _dev64(Q, "Q"), _dev64(log_pi.reshape(-1), "log_pi"), _dev64(log_trans, "log_trans")
    B, N, K = Q.shape
    dev = Q.device
    qn, fm, bm = torch.empty_like(Q), torch.empty_like(Q), torch.empty_like(Q)
    marg = torch.empty((B, N), dtype=torch.float64, device=dev)
    labels = torch.empty((B, N), dtype=torch.int64, device=dev)
    pair = torch.empty((B, N), dtype=torch.int64, device=dev) if want_pair else None
    last = torch.empty((B, K), dtype=torch.float64, device=dev)
    _ffi.check(_ffi.lib.hgp_hmm_local_terms_f64(_ptr(Q), _ptr(log_pi), _ptr(log_trans), N, K, B, _ptr(qn), _ptr(fm), _ptr(marg), _ptr(bm),
                                                _ptr(labels), _ptr(pair), _ptr(last), _stream()), "hmm_local_terms")
    return labels, pair, last


def loglik_rows(q):
    """GPI_HDP.LogLik(axis=1) on the device: (q - rowmax, rowmax); unchanged input if any row maximum is infinite."""
    q = _dev64(q, "q")
    N, K = q.shape
    out = torch.empty_like(q)
    rowmax = torch.empty(N, dtype=torch.float64, device=q.device)
    _ffi.check(_ffi.lib.hgp_loglik_rows_f64(_ptr(q), N, K, _ptr(out), _ptr(rowmax), _stream()), "loglik_rows")
    return out, rowmax


def assign(fmsg, bmsg, want_resp=False):
    """GPI_HDP._safe_exp(LogLik(log(alpha * beta))): labels [N] int64 (first arg-max per row) and, optionally, the one-hot resp."""
    fmsg, bmsg = _dev64(fmsg, "fmsg"), _dev64(bmsg, "bmsg")
    N, K = fmsg.shape
    labels = torch.empty(N, dtype=torch.int64, device=fmsg.device)
    resp = torch.empty((N, K), dtype=torch.float64, device=fmsg.device) if want_resp else None
    _ffi.check(_ffi.lib.hgp_assign_f64(_ptr(fmsg), _ptr(bmsg), N, K, _ptr(labels), _ptr(resp), _stream()), "assign")
    return (labels, resp) if want_resp else labels


def warp_batch(x, Yt, Ym, n_ctrl, iters, noise, lam_s, lam_a, lr, weights=None, u0=None, want_trace=True):
    """8f-4: B monotone time-warps fitted by Adam in one launch.  x [T]; Yt [B,T,D]; Ym [T,D] (shared) or [B,T,D].
    Returns (u [B,n_ctrl], x_warp [B,T], y_warp [B,T,D], trace [B,iters,4] or None)."""
    x, Yt, Ym = _dev64(x.reshape(-1), "x"), _dev64(Yt, "Yt"), _dev64(Ym, "Ym")
    B, T, D = Yt.shape
    stride = 0 if Ym.dim() == 2 else T * D
    dev = x.device
    w = None if weights is None else _dev64(weights.reshape(B), "weights")
    u0 = None if u0 is None else _dev64(u0.reshape(n_ctrl), "u0")
    u = torch.empty((B, n_ctrl), dtype=torch.float64, device=dev)
    xw = torch.empty((B, T), dtype=torch.float64, device=dev)
    yw = torch.empty((B, T, D), dtype=torch.float64, device=dev)
    tr = torch.empty((B, iters, 4), dtype=torch.float64, device=dev) if want_trace else None
    _ffi.check(_ffi.lib.hgp_warp_batch_f64(_ptr(x), _ptr(Yt), _ptr(Ym), stride, T, B, D, int(n_ctrl), int(iters), float(noise),
                                           float(lam_s), float(lam_a), float(lr), _ptr(w), _ptr(u0), _ptr(u), _ptr(xw), _ptr(yw),
                                           _ptr(tr), _stream()), "warp_batch")
    return u, xw, yw, tr
