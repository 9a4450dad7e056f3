"""The online step's member updates as PERSISTENT chains (BASELINE configs[4]; GPI_HDP.py:1906-2208 with
GPI_model.py:325-375,705-716,966-1115,1300-1344).

Per beat the reference asks every cluster "what would you look like with this beat?": a deep copy, one Kalman update
(estimate_new), the same update again (include_weighted_sample), the two-step smoother (backwards_pair), the two MNIW updates
(bayesian_new_params), then the latent-transition scores of ALL the copy's members and the MNIW likelihood of its new
parameters - candidate after candidate, ~150 dependent launches each (round 3: 3 700 launches and 62-80 ms per beat at T = 256).
Nothing a candidate computes feeds another one.  Here every cluster model of a lead owns a slot of an ``OnlinePool``:

* its per-step lists live in growing stacks ([rows, T, T]; the model's lists are views, a12) with the device-side position,
  counters and MNIW distributions of member_step.Chain - the cluster IS a chain that is never torn down;
* ``candidates(y)`` runs the member step of ALL clusters side by side with the level-fused lists of the offline chains
  (hgp_gemm_list_f64, one launch per dependency level over every cluster's items; the two inversions batched over
  [4 x clusters] / [2 x clusters] matrices) as a DRY run: the new rows land behind each chain's end, the re-smoothed previous
  state stays in the step's buffers, nothing of the cluster changes (finish flags 2 | 4, include/hdpgpc_hip.h).  One Kalman
  update serves estimate_new and the inclusion (the last filtered and smoothed states of an online chain coincide);
* of a candidate's latent-transition scores only three can differ from the cluster's cached ones (member 0 reads the LAST
  transition parameters, the previous member was re-smoothed, the new member): 3 x clusters a8 items and 2 x clusters a9 items
  are gathered by ONE copy-list launch and scored by one batched call each;
* ``commit(g, ...)`` is the same step for the cluster that absorbs the beat, for real and without the smoother (the reference's
  commit does not call backwards_pair, GPI_HDP.py:2186-2196): the previous smoothed mean takes the smoother's place in the
  MNIW update and the previous row is left alone (finish flag 4);
* a cluster with an estimation limit E keeps its slot: from the member that makes N' = E on, its finish descriptors (dry and
  real) carry flag 8 - the state rows as always, no MNIW update, the parameter rows copied forward - so the row-indexed gathers
  above keep finding the last estimated parameters at row N + 1.  The slot still runs the full level lists: all slots share
  one set of tile maps.
"""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _ffi, ops
from .GPI_model import LOG2PI
from .member_step import (Chain, finish_desc, gather, gather_desc, member_step, shared_buffers, upload_descs, ws_offset, ws_size,
                          ws_view)

f64 = torch.float64
# every cluster with the beat added, in CLUSTER order: est [M] device (estimate_new's score), cols [T_all, M] device (the
# candidates' latent-transition columns), lds [M] host floats (return_LDS_param_likelihood); the would-be NEW cluster's single
# latent-transition score (device scalar) and parameter likelihood (host float), None when `extra` was not taken
Candidates = namedtuple("Candidates", "est cols lds extra_lat extra_lds")


def _copy_rows(rows, src, dbuf, item, n):
    """One more block of the copy-list table `rows`: n doubles from byte address src[i] to item item[i] (n doubles each) of dbuf."""
    src, item = np.atleast_1d(np.asarray(src, dtype=np.int64)), np.atleast_1d(np.asarray(item, dtype=np.int64))
    rows.append(np.stack([src, dbuf.data_ptr() + item * (8 * n), np.full(len(src), n, dtype=np.int64)], axis=1))


class _LevelLists:
    """The level lists of every slot, level-major in device memory with room for `cap` slots.  All slots have the same item
    shapes, so the per-tile maps of hgp_gemm_list_mapped_f64 depend on the slot index only and are laid down once for the whole
    capacity; adopting a cluster uploads that slot's items (one small copy per level) instead of rebuilding every list."""

    def __init__(self, cap, device):
        self.cap, self.device = cap, device
        self.per = self.tiles = self.dev = self.map = None
        self.keep = {}

    def set_slot(self, c, lv):
        isz = ctypes.sizeof(_ffi.GemmItem)
        if self.per is None:
            self.per = [len(l_._items) for l_ in lv]
            self.tiles = [list(l_._item_tiles) for l_ in lv]
            self.dev, self.map = [], []
            for per, tiles in zip(self.per, self.tiles):
                if self.cap * per > 65535:
                    raise ValueError("online pool: too many clusters for the 16-bit item index of the tile map")
                self.dev.append(torch.zeros(self.cap * per * isz, dtype=torch.uint8, device=self.device))
                one = np.concatenate([(i << 16) | np.arange(n, dtype=np.uint32) for i, n in enumerate(tiles)]).astype(np.uint32)
                allm = (one[None, :] + ((np.arange(self.cap, dtype=np.uint32) * per) << 16)[:, None]).reshape(-1)
                self.map.append(torch.from_numpy(allm.view(np.int32)).to(self.device))
        for l, l_ in enumerate(lv):
            assert len(l_._items) == self.per[l] and list(l_._item_tiles) == self.tiles[l]
            arr = (_ffi.GemmItem * self.per[l])(*l_._items)
            host = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy())
            self.dev[l][c * self.per[l] * isz:(c + 1) * self.per[l] * isz].copy_(host)
        self.keep[c] = lv                      # the operands' storage must outlive the lists

    def run(self, l, lo, hi):
        per, tps = self.per[l], sum(self.tiles[l])
        isz = ctypes.sizeof(_ffi.GemmItem)
        if lo == 0:
            _ffi.check(_ffi.lib.hgp_gemm_list_mapped_f64(ops._ptr(self.dev[l]), per * hi, ops._ptr(self.map[l]), tps * hi, ops._stream()),
                       "gemm_list_mapped")
        else:
            base = ctypes.c_void_p(self.dev[l].data_ptr() + lo * per * isz)
            _ffi.check(_ffi.lib.hgp_gemm_list_f64(base, per * (hi - lo), tps * (hi - lo), ops._stream()), "gemm_list")


class _Slot:
    __slots__ = ("g", "ch", "rows", "N", "def_diag", "bad0")


class OnlinePool:
    """All cluster models of one lead of an online GPI_HDP, as persistent chains (see the module docstring)."""

    def __init__(self, T, device, annealing, cap=32):
        self.T, self.device, self.annealing = int(T), device, bool(annealing)
        self.slots = []
        self.cap = 0
        self.ybuf = torch.zeros((1, T), dtype=f64, device=device)
        self._pending = None
        self._alloc(cap)

    # ------------------------------------------------------------------ storage
    def _alloc(self, cap):
        T, dev = self.T, self.device
        new = lambda *shape: torch.zeros(shape, dtype=f64, device=dev)            # noqa: E731
        self.cap = cap
        self.WS = ws_size(T)
        self.ws_all = new(cap, self.WS)
        self.shared = shared_buffers(cap, T, dev, work=True)
        self.bad_all = torch.zeros((cap, 2), dtype=torch.int32, device=dev)      # committed steps
        self.badc_all = torch.zeros((cap, 2), dtype=torch.int32, device=dev)     # candidate steps (cleared per beat)
        self.sync_all = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.est_mean, self.mean_last = new(cap, T), new(cap, T)
        # the step buffers of every slot (Chain.build_lists: 21 T x T matrices and 6 vectors) come out of ONE arena, zeroed once:
        # adopting a cluster used to cost 43 allocations and 22 MB of memsets at T = 256
        self.ARENA = 21 * T * T + 6 * T + 128          # (every piece starts on a 32-byte boundary)
        self.arena = new(cap, self.ARENA)
        self.ini_noise_all = new(cap)
        self.lists = _LevelLists(cap, dev)
        self.descs_dirty = True
        self._base = np.zeros((cap, 8), dtype=np.int64)        # byte addresses of the stacks / step buffers of every slot
        self._bufp = np.zeros((cap, 3), dtype=np.int64)
        # inputs of the batched a8 (three members per cluster) and a9 (two parameter pairs per cluster) calls
        self.LF_cur, self.LF_prev = new(cap * 3, T), new(cap * 3, T)
        self.LA, self.LG, self.LC = new(cap * 3, T, T), new(cap * 3, T, T), new(cap * 3, T, T)
        self.MN_M, self.MN_S, self.MN_mean, self.MN_scale = (new(cap * 2, T, T) for _ in range(4))

    def _grow(self):
        """Twice the cluster capacity: the per-cluster slices of the shared buffers move, so every slot's lists are rebuilt.
        A commit in flight is finished first (its status words live in the buffers that go), and the committed steps' status
        words move with their slots: bad_all[c, 0] counts the skipped MNIW updates of slot c for the life of its chain, and
        sl.bad0 is the host's copy of that count."""
        self.finish_commit()
        old, bad = self.slots, self.bad_all
        self.slots = []
        self._alloc(self.cap * 2)
        self.bad_all[:bad.shape[0]].copy_(bad)
        for sl in old:
            self._bind(sl)

    def _bind(self, sl, c=None):
        """Give the slot its index (c: the index of the slot it replaces; default: the next free one), its slices of the shared
        buffers and its level lists."""
        c = len(self.slots) if c is None else c
        sl.g._slot = c
        ch = sl.ch
        ch.ws = self.ws_all[c]
        ch.bad, ch.sync = self.bad_all[c], self.sync_all[c:c + 1]
        ch.Y, ch.y_row0 = self.ybuf, -1
        arena, used = self.arena[c], [0]                       # build_lists must stay inside it (asserted below)
        arena.zero_()

        def alloc(*shape):
            n = int(np.prod(shape))
            out = arena[used[0]:used[0] + n].view(*shape)
            used[0] += (n + 3) & ~3
            return out

        ch.build_lists(self.shared, c, alloc)
        assert used[0] <= self.ARENA, "online pool: the step buffers of Chain.build_lists outgrew the slot's arena"
        Cw = ws_view(ch.ws, "C", self.T)
        ch.lv[6].add(Cw, ch.bufs["f_post"], self.est_mean[c])                # C_last f_post: the mean estimate_new scores against
        lvm = ops.GemmList(self.device)                                      # C_last f_last: the mean the beat is scored against
        lvm.add(Cw, ws_view(ch.ws, "m0", self.T), self.mean_last[c])
        self.lv_mean_last = len(ch.lv)                                       # the pool's own level, behind the step's
        self.lists.set_slot(c, ch.lv + [lvm])
        self._base[c] = ch.stack_ptrs()
        self._bufp[c] = [ch.bufs[k].data_ptr() for k in ("f_post", "f_sm_prev", "P_sm_prev")]
        self.descs_dirty = True
        dd = sl.g
        self.ini_noise_all[c] = 1e-2 * torch.mean(torch.diagonal(dd.Sigma[0]))
        self.MN_mean[2 * c].copy_(dd.C_def), self.MN_mean[2 * c + 1].copy_(dd.A_def)
        self.MN_scale[2 * c].copy_(dd.Sigma_def), self.MN_scale[2 * c + 1].copy_(dd.Gamma_def)
        if c == len(self.slots):
            self.slots.append(sl)
        else:
            self.slots[c] = sl

    @staticmethod
    def supports(g):
        """The chain step covers: dynamic model, at least one member, last filtered = last smoothed state (always true for a
        chain grown online), no tracked rank-1 factor; the parameter lists as long as the state lists, or as the estimation
        limit once the cluster has reached it."""
        if g.N < 1 or g._rank1_on() or not g._is_dynamic() or not g._dyn_prior():
            return False
        n = len(g.f_star)
        if not (n == len(g.f_star_sm) == len(g.cov_f) == len(g.cov_f_sm)):
            return False
        if not (min(n, g.estimation_limit) == len(g.A) == len(g.Gamma) == len(g.C) == len(g.Sigma)):
            return False
        same = lambda a, b: a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape) or bool(torch.equal(a, b))   # noqa: E731
        return same(g.f_star[-1], g.f_star_sm[-1]) and same(g.cov_f[-1], g.cov_f_sm[-1])

    def _slot_of(self, g):
        """The slot that was made for the model g, or None."""
        c = getattr(g, "_slot", None)
        return self.slots[c] if c is not None and c < len(self.slots) and self.slots[c].g is g else None

    def holds(self, g):
        """Does a slot of this pool carry the model g - as it is now?  The chain is the cluster only as long as nobody else
        changes the model: a member step taken with the one-by-one methods (a beat off the basis grid, OnlineLoop._member_update)
        turns the lists into real ones and moves N, and the slot's stacks, position and device-side distributions stay behind.
        Such a model is not held any more; adopt(g) gives it its slot back, rebuilt."""
        sl = self._slot_of(g)
        return sl is not None and sl.N == g.N and len(g.f_star) == sl.N + 1 and sl.ch.bound_to(g)

    def adopt(self, g):
        """Move the model's per-step lists into a slot's stacks (the model keeps reading them through views).  A model that has
        a slot already keeps it: the slot gets a new chain built from the model as it is now (see holds())."""
        c = None
        if self._slot_of(g) is not None:
            self.finish_commit()
            c = g._slot
            self.bad_all[c].zero_()
        elif len(self.slots) == self.cap:
            self._grow()
        L = len(g.f_star)
        sl = _Slot()
        sl.g, sl.N, sl.rows = g, L - 1, max(8, 2 * L)
        sl.ch = Chain.from_model(g, sl.rows)
        sl.def_diag = g._defs_diagonal()
        sl.bad0 = 0
        self._bind(sl, c)
        self._rebind_lists(sl, float(g.internal_params.n0))
        return sl

    def _rebind_lists(self, sl, n0, lat=None):
        """The model's lists and MNIW objects as views of the slot's stacks.  The new lists hold what the old ones held, so the
        members' latent-transition scores stay valid: the memo of them (lat, when given: the scores after a commit) goes with
        the new lists."""
        g = sl.g
        if lat is None:
            lat = self._lat_memo(g)
        sl.ch.bind_model(g, sl.N + 1, n0, Lp=int(min(sl.N + 1, g.estimation_limit)))
        if lat is not None:
            g._memo_put("lat_all", g._LAT_LISTS, lat, (1.0, len(g.indexes)))

    @staticmethod
    def _lat_memo(g):
        """The model's memoised latent-transition scores (compute_q_lat_all, h_ini = 1) if they are current, else None."""
        return g._memo_get("lat_all", g._LAT_LISTS, (1.0, len(g.indexes)))

    def _more_rows(self, sl):
        sl.rows *= 2
        sl.ch.more_rows(sl.rows)
        self._rebind_lists(sl, float(sl.g.internal_params.n0))
        self._base[sl.g._slot] = sl.ch.stack_ptrs()
        self.descs_dirty = True

    # ------------------------------------------------------------------ launch tables
    def _prepare(self):
        """Descriptor arrays of the gather / finish launches for the current slots (re-uploaded when a slot is added or its
        stacks move)."""
        gd, fd_dry, fd_real = [], [], []
        for c, sl in enumerate(self.slots):
            gd.append(gather_desc(sl.ch))
            fz = 8 if self._frozen(sl) else 0      # the slot runs the full lists (uniform tile maps); only its finish freezes
            fd_dry.append(finish_desc(sl.ch, int(self.annealing) | 2 | 4 | fz, self.badc_all[c]))
            fd_real.append(finish_desc(sl.ch, int(self.annealing) | 4 | fz, self.bad_all[c]))
        self.gdev, self.fdev_dry, self.fdev_real = (upload_descs(d, self.device) for d in (gd, fd_dry, fd_real))
        self.descs_dirty = False

    @staticmethod
    def _frozen(sl):
        """Does the slot's next member reach the cluster's estimation limit (N' >= E: no MNIW update, GPI_model.py:974,1092)?"""
        return sl.N + 1 >= sl.g.estimation_limit

    def _step(self, lo, hi, dry, gather_first=True):
        """The member step of slots [lo, hi): a dry run for candidates (nothing of the cluster changes), else the committed step
        without the smoother (see the module docstring)."""
        if self.descs_dirty:
            self._prepare()
        member_step(self.lists, self.shared, self.gdev, self.fdev_dry if dry else self.fdev_real, lo, hi, self.T,
                    gather_first=gather_first, no_smoother=() if dry else [sl.ch for sl in self.slots[lo:hi]])

    # ------------------------------------------------------------------ the beat under the clusters' last states
    def _score_gathered(self, mean, add=None):
        """The beat in ybuf against (mean[c], the gathered Sigma_last of slot c) for every slot -> (scores, LAPACK infos) [M]."""
        M, T = len(self.slots), self.T
        ar = np.arange(M, dtype=np.int32)
        quad, _, info = ops.score_each(self.ybuf.expand(M, T).contiguous(), mean, self.ws_all[0, ws_offset("S", T):], ar, ar, add,
                                       strides=(T, self.WS))
        return -0.5 * quad - 0.5 * T * LOG2PI, info

    def begin_beat(self, y, models):
        """Gather every cluster's last state (row pos of its stacks) and score the beat y [T] under it: log_sq_error(x, y, i=-1)
        of GPI_HDP.py:1973 for all clusters in three launches.  models: the lead's cluster list - the one place where the
        slot <-> cluster permutation of the beat is built; every result of this beat is in that CLUSTER order.  Returns
        (scores [M] device, their LAPACK infos - any order); the gathered state stays valid for candidates() of the same beat."""
        M, T = len(self.slots), self.T
        self.slot_of = [g._slot for g in models]                               # slot of every cluster
        self.slot_dev = ops.to_dev(self.slot_of, torch.int64, self.device)
        for sl in self.slots:
            if sl.N + 2 > sl.rows:
                self._more_rows(sl)
        self.ybuf.copy_(y.reshape(1, T))
        if self.descs_dirty:
            self._prepare()
        gather(self.gdev, 0, M, T)
        self.lists.run(self.lv_mean_last, 0, M)                # mean_last = C_last f_last
        sc, info = self._score_gathered(self.mean_last)
        return sc[self.slot_dev], info

    # ------------------------------------------------------------------ candidates
    def candidates(self, t_new, q_lat_cols, extra=None):
        """Every cluster with the beat of begin_beat(y, models) added (dry run) -> Candidates, in the cluster order of `models`.
        q_lat_cols [T_all, M]: the clusters' current latent-transition columns in that order.  extra (optional): the would-be
        NEW cluster (one member, GPI_HDP.py:1990-1996) - its single latent-transition score and its two parameter likelihoods
        ride the same batched a8 / a9 calls when there is room behind the last slot and it is the plain case (else the
        result's extra_* are None: the caller's job)."""
        M = len(self.slots)
        if extra is not None and (M >= self.cap or extra.N != 1 or not extra._dyn_prior()):
            extra = None
        est, info = self._dry_step()
        table, nl, nm, diag = self._copy_table(extra)
        lat, lds, extra_lds = self._score_copies(table, nl, nm, diag, info)
        slot_cols = q_lat_cols[:, ops.to_dev(np.argsort(self.slot_of), torch.int64, self.device)]      # cluster of every slot
        cols = self._candidate_columns(slot_cols, lat, t_new)
        return Candidates(est[self.slot_dev], cols[:, self.slot_dev], [float(lds[c]) for c in self.slot_of],
                          None if extra is None else lat[3 * M], extra_lds)

    def _dry_step(self):
        """The member step of every slot as a dry run on the state begin_beat gathered, and estimate_new: the beat against
        (C_last f_post, Sigma_last), `first` inflation for one-member clusters.  Reads row N of every stack; writes row N + 1."""
        M = len(self.slots)
        self.badc_all[:M].zero_()
        self._step(0, M, dry=True, gather_first=False)
        add = self.ini_noise_all[:M] * ops.to_dev(np.array([1.0 if sl.N == 1 else 0.0 for sl in self.slots]), f64, self.device)
        return self._score_gathered(self.est_mean, add)

    def _copy_table(self, extra):
        """The copy-list table that lays out the a8 / a9 inputs: three a8 items and two a9 items per slot, extra's one and two
        behind them.  Rows read per slot (N = members so far = index of the last row): 1, N - 1, N, the dry run's N + 1, and
        the step's f_post / f_sm_prev / P_sm_prev.  Returns (table [rows, 3] host, a8 items, a9 items, all default scales diagonal)."""
        M, T, tt = len(self.slots), self.T, self.T * self.T
        N = np.array([sl.N for sl in self.slots], dtype=np.int64)
        one = N == 1
        base = self._base[:M]
        iA, iG, iC, iS, iPsm, iP, iF, iFsm = range(8)
        row = lambda k, r, n: base[:, k] + r * (8 * n)                           # noqa: E731  (byte address of a stack row)
        f_post, f_smp, P_smp = self._bufp[:M].T
        rows = []
        put = lambda s, dbuf, j, n: _copy_rows(rows, s, dbuf, np.arange(M) * (dbuf.shape[0] // self.cap) + j, n)    # noqa: E731
        # member 0: cur = prev = row 1, cov = row 1 (the re-smoothed one when it is also the previous member), par = the NEW row
        f1 = np.where(one, f_smp, row(iFsm, 1, T))
        put(f1, self.LF_cur, 0, T), put(f1, self.LF_prev, 0, T)
        put(row(iA, N + 1, tt), self.LA, 0, tt), put(row(iG, N + 1, tt), self.LG, 0, tt)
        put(np.where(one, P_smp, row(iPsm, 1, tt)), self.LC, 0, tt)
        # member N - 1 (N >= 2; a repeat of member 0's inputs otherwise, ignored): cur = re-smoothed row N, prev / cov = row N - 1, par = N
        Nm = np.maximum(N - 1, 1)
        put(f_smp, self.LF_cur, 1, T), put(row(iFsm, Nm, T), self.LF_prev, 1, T)
        put(row(iA, N, tt), self.LA, 1, tt), put(row(iG, N, tt), self.LG, 1, tt), put(row(iPsm, Nm, tt), self.LC, 1, tt)
        # the new member: cur = f_post, prev / cov = the re-smoothed row N, par = the NEW row
        put(f_post, self.LF_cur, 2, T), put(f_smp, self.LF_prev, 2, T)
        put(row(iA, N + 1, tt), self.LA, 2, tt), put(row(iG, N + 1, tt), self.LG, 2, tt), put(P_smp, self.LC, 2, tt)
        # a9: (C, Sigma) and (A, Gamma) of the NEW row against their priors
        put(row(iC, N + 1, tt), self.MN_M, 0, tt), put(row(iS, N + 1, tt), self.MN_S, 0, tt)
        put(row(iA, N + 1, tt), self.MN_M, 1, tt), put(row(iG, N + 1, tt), self.MN_S, 1, tt)
        nl, nm = 3 * M, 2 * M
        diag = all(sl.def_diag for sl in self.slots)
        if extra is not None:   # one a8 item (member 0 of a one-member cluster: GPI_model._lat_indices) and two a9 items behind the slots'
            e = extra
            fs, cs = e.f_star_sm[1].contiguous(), e.cov_f_sm[1].contiguous()
            Ae, Ge, Ce, Se = (m_.contiguous() for m_ in (e.A[-1], e.Gamma[-1], e.C[-1], e.Sigma[-1]))
            defs = [m_.contiguous() for m_ in (e.C_def, e.Sigma_def, e.A_def, e.Gamma_def)]
            self._extra_keep = (fs, cs, Ae, Ge, Ce, Se, defs)
            for t_, buf, j, n in ((fs, self.LF_cur, nl, T), (fs, self.LF_prev, nl, T), (Ae, self.LA, nl, tt), (Ge, self.LG, nl, tt),
                                  (cs, self.LC, nl, tt), (Ce, self.MN_M, nm, tt), (Se, self.MN_S, nm, tt), (Ae, self.MN_M, nm + 1, tt),
                                  (Ge, self.MN_S, nm + 1, tt), (defs[0], self.MN_mean, nm, tt), (defs[1], self.MN_scale, nm, tt),
                                  (defs[2], self.MN_mean, nm + 1, tt), (defs[3], self.MN_scale, nm + 1, tt)):
                _copy_rows(rows, t_.data_ptr(), buf, j, n)
            nl, nm = nl + 1, nm + 2
            diag = diag and e._defs_diagonal()
        return np.concatenate(rows), nl, nm, diag

    def _score_copies(self, table, nl, nm, diag, info):
        """The copy-list launch, the batched a8 call (nl items) and a9 call (nm items), and ONE host round trip for everything
        the loop branches on (info: estimate_new's statuses ride it).  Reads only what _copy_table laid out.  Returns
        (lat [nl] device, lds [M] host in slot order, extra's lds or None)."""
        M, T = len(self.slots), self.T
        ops.copy_list(ops.to_dev(table, torch.int64, self.device), table.shape[0], T * T)
        lat, info_l = ops.lat_error(self.LF_cur[:nl], self.LF_prev[:nl], self.LA[:nl], self.LG[:nl], self.LC[:nl])
        lat = lat - 0.5 * T * LOG2PI
        mn, info_m = ops.mniw_loglik(self.MN_M[:nm], self.MN_S[:nm], self.MN_mean[:nm], None, self.MN_scale[:nm], scale_is_diagonal=diag)
        lds_dev = torch.sum(mn.view(nm // 2, 2), dim=1) / T * 100.0
        flat = torch.cat([lds_dev, info.to(f64), info_l.to(f64), info_m.to(f64), self.badc_all[:M].reshape(-1).to(f64)]).cpu().numpy()
        nx = nm // 2
        if flat[nx:nx + M + nl + nm].any():       # score [M] / a8 [nl] / a9 [nm] infos
            bad = int(np.nonzero(flat[nx:nx + M + nl + nm])[0][0])
            what = "log_sq_error" if bad < M else ("log_lat_error" if bad < M + nl else "log_likelihood_MNIW")
            raise torch.linalg.LinAlgError(f"{what}: the input is not positive-definite (online candidate step)")
        badc = flat[nx + M + nl + nm:].reshape(M, 2)
        if badc[:, 1].any():
            raise torch.linalg.LinAlgError("posterior / backwards_pair: the input is not positive-definite (online candidate step)")
        return lat, flat[:M], float(flat[M]) if nx > M else None

    def _candidate_columns(self, slot_cols, lat, t_new):
        """The candidates' columns (slot order): the cluster's own column slot_cols[:, c] with (up to) three entries replaced by
        the a8 scores lat[3 c : 3 c + 3] - rows = segment ids of member 0, of member N - 1 (N >= 2) and t_new."""
        cols = slot_cols.clone()
        rr, cc, vv = [], [], []
        for c, sl in enumerate(self.slots):
            idx = sl.g.indexes
            rr += [idx[0], t_new]
            cc += [c, c]
            vv += [3 * c, 3 * c + 2]
            if sl.N >= 2:
                rr.append(idx[sl.N - 1]), cc.append(c), vv.append(3 * c + 1)
        ix = ops.to_dev(np.array([rr, cc, vv]), torch.int64, self.device)
        cols[ix[0], ix[1]] = lat[ix[2]]
        return cols

    # ------------------------------------------------------------------ commit
    def commit(self, g, index, x_train, y):
        """include_weighted_sample(h = 1) + bayesian_new_params(1) of the cluster that absorbs the beat (no smoother).  The launches
        are enqueued and the host-side bookkeeping is done here; the two status words the reference looks at (a failed filter
        step raises, a failed MNIW factorisation keeps the previous distributions, GPI_model.py:1068) are read by finish_commit(),
        so that the caller's host work (the HDP global step) overlaps the device work."""
        self.finish_commit()
        sl = self.slots[g._slot]
        T = self.T
        if sl.N + 2 > sl.rows:
            self._more_rows(sl)
        lat_old = self._lat_memo(g)
        col = None if lat_old is None else g._memo_get("lat_col", (), (lat_old,))
        yv = g.cond_to_torch(y).reshape(-1, 1)
        self.ybuf.copy_(yv.reshape(1, T))
        c = g._slot
        frozen = self._frozen(sl)
        self._step(c, c + 1, dry=False)
        sl.N += 1
        g.N += 1
        if not frozen and self._frozen(sl):                    # from the next beat on this slot's finish carries flag 8
            self.descs_dirty = True
        g.indexes.append(int(index))
        g.x_train.append(x_train)
        g.y_train.append(yv)
        info = new = None
        if lat_old is not None:
            # latent-transition scores: member 0 now reads the new last parameters, the new member is added; the rest is unchanged
            n = sl.N                                          # members now; rows 0..n
            ch = sl.ch
            fs, ps = ch.Fsm, ch.Psm
            cur = torch.stack((fs[1], fs[n])).reshape(2, T)
            prv = torch.stack((fs[1], fs[n - 1])).reshape(2, T)
            A2, G2 = torch.stack((ch.A[n], ch.A[n])), torch.stack((ch.G[n], ch.G[n]))
            C2 = torch.stack((ps[1], ps[n - 1]))
            out, info = ops.lat_error(cur, prv, A2, G2, C2)
            out = out - 0.5 * T * LOG2PI
            new = torch.cat([out[0:1], lat_old[1:], out[1:2]])
            if col is not None and col.shape[0] > int(index):  # the scattered column: two entries change
                col[ops.to_dev([g.indexes[0], int(index)], torch.int64, self.device)] = out
                g._memo_put("lat_col", (), col, (new,))
        self._rebind_lists(sl, float(g.internal_params.n0) + (0.0 if frozen else 1.0), lat=new)
        self._pending = (sl, info, frozen)

    def finish_commit(self):
        if self._pending is None:
            return
        (sl, info, frozen), self._pending = self._pending, None
        g, c = sl.g, sl.g._slot
        flat = torch.cat([self.bad_all[c].to(f64)] + ([] if info is None else [info.to(f64)])).tolist()     # one round trip
        if flat[1] != 0:
            raise torch.linalg.LinAlgError("posterior: the input is not positive-definite (online step)")
        if any(flat[2:]):
            raise torch.linalg.LinAlgError("log_lat_error: the input is not positive-definite (online step)")
        updated = frozen or int(flat[0]) == sl.bad0           # (a frozen step has no MNIW update to skip, and did not count one)
        sl.bad0 = int(flat[0])
        if not updated:                                        # the MNIW update was skipped: the distributions kept their count
            if g.verbose:
                print("Alg error matrix ill conditioned.")
            g.internal_params.n0 -= 1.0
            g.observation_params.n0 -= 1.0
