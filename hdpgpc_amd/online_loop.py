"""The online variational step of GPI_HDP (hdpgpc/hdpgpc/GPI_HDP.py:1906-2208 ``include_sample`` with
``variational_local_terms`` :586, ``estimate_new`` :2830, ``reorder`` :1091) - one segment at a time: score it under every
cluster, compare "open a new cluster" against "give it to an existing one" through the one-sample bound, commit.

Host orchestration over the same kernels as the offline loop; per beat the device work is
* a5: the segment's score under the last state of every cluster (ONE shared-covariance launch for all clusters when the
  segment sits on the basis grid, the per-pair kernel otherwise),
* a8: the latent-transition scores of every cluster's members (kept per model until the model changes - only the cluster that
  absorbs the beat changes),
* a9 through the bound, the Kalman / MNIW update of the candidates (GPI_model.posterior_weighted, include_weighted_sample,
  backwards_pair, bayesian_new_params) and the switching-variable messages over the whole history (ops.hmm_messages).
``with_warp=True`` (the time-warp fit of every beat) and ``classify=True`` (no caller in the reference) are not built.
"""
from types import SimpleNamespace

import numpy as np
import torch
from scipy.special import digamma as _digamma

from . import online_chain, ops
from .online_chain import Candidates

f64 = torch.float64


class OnlineLoop:
    """Mixin of GPI_HDP: the streaming (online) variational step."""

    def variational_local_terms(self, q, transTheta=None, startTheta=None, liks=None, classify=False):
        """GPI_HDP.py:586-630: hard state / pair assignments of the whole history from the score matrix q [T, K, D] (device).
        Returns (resp one-hot [T,K] host, log resp of the LAST row (numpy), respPair one-hot [T,K,K] host, None)."""
        startPi = self._start_pi(self.startTheta if startTheta is None else startTheta)
        q = q.clone()
        if liks is not None:
            q[-1] = q[-1] + torch.as_tensor(np.asarray(liks, dtype=np.float64), device=q.device)[:, None]
        q_norm, _ = self.LogLik(self.weight_mean(q).contiguous())
        fmsg, _, bmsg, pair = self._messages(startPi, q_norm, True)
        resp, respPair = self._one_hot_tables(fmsg, bmsg, pair)
        last = torch.log(fmsg[-1] * bmsg[-1]).cpu().numpy()
        return resp, last - np.max(last) if np.isfinite(np.max(last)) else last, respPair, None

    def _start_pi(self, startTheta):
        """Expected log start probabilities of the M clusters under the Dirichlet pseudo-counts (GPI_HDP.py:610)."""
        st, M = _np(startTheta), self.M
        return torch.as_tensor(_digamma(st[:M]) - _digamma(np.sum(st[:M + 1])), dtype=f64)

    def estimate_new(self, t, gpmodel, x_train, y, h=1.0):
        """GPI_HDP.py:2830-2842: the segment's score under the state the model would have after absorbing it."""
        mean_, cov_, C_, Sigma_ = gpmodel.smoother_weighted(x_train, y, h)
        return gpmodel.log_sq_error(x_train, y, mean=mean_[-1], cov=cov_[-1], C=C_[-1], Sigma=Sigma_[-1], i=-1,
                                    first=len(gpmodel.indexes) == 1)

    def reorder(self, resp, respPair, q, q_lat):
        """GPI_HDP.py:1091-1110: clusters sorted by size, largest first (tables, score matrices and the model list)."""
        order, resp = _by_size(resp)
        respPair = respPair[:, order, :][:, :, order]
        od = ops.to_dev(order, torch.int64, q.device)
        q, q_lat = q.index_select(1, od), q_lat.index_select(1, od)
        for ld in range(self.n_outputs):
            self.gpmodels[ld] = [self.gpmodels[ld][int(order[i])] for i in range(self.M)]
        return resp, respPair, q, q_lat, order

    def _online_pool(self, ld, x):
        """The persistent chains of lead ld's clusters (online_chain.OnlinePool), or None when the beat does not sit on the
        basis grid (the chain step covers the shared-grid case; other grids take the one-by-one path)."""
        xb = self.gpmodels[ld][0].x_basis if self.gpmodels[ld] else None
        if xb is None or x.shape != xb.shape or not bool(torch.equal(x, xb)) or ops.env_flag("HGP_ONLINE_EAGER"):
            return None
        pools = self.__dict__.setdefault("_pools", {})
        models = self.gpmodels[ld]
        pool = pools.get(ld)
        if pool is not None and len(pool.slots) > 0:
            listed = {id(g) for g in models}
            if any(id(sl.g) not in listed for sl in pool.slots):
                # a slot's model has left the list (the list was replaced by copies, a cluster was dropped): the chains start over
                pool.finish_commit()
                pool = None
        if pool is None:
            pool = pools[ld] = online_chain.OnlinePool(xb.shape[0], self.device, self.annealing_def)
        for g in models:
            # (a model that was changed behind its chain's back - the one-by-one commit of a beat off the grid - is not held)
            if not pool.holds(g):
                if not pool.supports(g):
                    return None
                pool.adopt(g)
        return pool

    def _last_scores(self, x, y, ld):
        """log_sq_error(x, y, i=-1) of the segment under every cluster of lead ld (GPI_HDP.py:1973) -> [M] device.
        On the basis grid pred_dist short-circuits (GPI.py:467-468) and the M evaluations are one launch."""
        models = self.gpmodels[ld]
        xb = models[0].x_basis
        if x.shape == xb.shape and bool(torch.equal(x, xb)) and not any(g.rank1_scale_factor() is not None for g in models):
            sel = [g._select(-1) for g in models]
            means = torch.stack([g._mean_of(ci, fi).reshape(-1) for g, (ci, fi) in zip(models, sel)]).contiguous()
            Sig = torch.stack([g.Sigma[ci] for g, (ci, _) in zip(models, sel)]).contiguous()
            M, T = means.shape
            Y = y[:, ld].reshape(1, T).expand(M, T).contiguous()
            quad, _, info = ops.score_each(Y, means, Sig, np.arange(M, dtype=np.int32), np.arange(M, dtype=np.int32))
            ops.raise_on_info(info, "log_sq_error")
            return -0.5 * quad - 0.5 * T * ops.LOG2PI
        return torch.stack([g.log_sq_error(x, y[:, [ld]], i=-1) for g in models])

    # ------------------------------------------------------------------ the local step for many score matrices at once
    def _local_terms_many(self, Qw, liks=None):
        """variational_local_terms (GPI_HDP.py:586-630) for a batch Qw [B, T, K] of lead-combined score matrices (device): one
        launch sequence for all of them (ops.hmm_local_terms), one host round trip.  Returns host arrays
        (labels [B, T], pair_first [B, T] - flat index into the K x K pair table, last [B, K] - log resp of the newest row,
        max-shifted as the reference's)."""
        dev = self.device
        B, N, K = Qw.shape
        startPi = self._start_pi(self.startTheta)
        if liks is not None:
            Qw = Qw.clone()
            Qw[:, -1, :] += ops.to_dev(np.asarray(liks, dtype=np.float64), f64, dev)[None, :]
        labels, pairs, last = ops.hmm_local_terms(Qw.contiguous(), ops.to_dev(self.compute_trans_pi(K, startPi), f64, dev),
                                                  ops.to_dev(self.compute_trans_A(K), f64, dev))
        flat = torch.cat([labels.reshape(-1).to(f64), pairs.reshape(-1).to(f64), last.reshape(-1)]).cpu().numpy()
        lab = flat[:B * N].astype(np.int64).reshape(B, N)
        prs = flat[B * N:2 * B * N].astype(np.int64).reshape(B, N)
        last = flat[2 * B * N:].reshape(B, K).copy()
        for b in range(B):
            mx = np.max(last[b])
            if np.isfinite(mx):
                last[b] -= mx
        return lab, prs, last, labels

    def _bound_from_labels(self, labels, pairs, K, n_rows, n_cols, q_sum, lat_sum, lds, post):
        """compute_q_elbo(resp[:n_rows, :n_cols], respPair[:n_rows, :n_cols, :n_cols], ..., one_sample=True) (GPI_HDP.py:1796-1836)
        from the hard assignment itself (labels / pair_first of ONE score matrix, host ints), the two device sums over the
        assigned entries and the clusters' MNIW parameter likelihoods lds [n_cols] - no [T, K, K] table is built."""
        lab, prs = labels[:n_rows], pairs[:n_rows]
        # the HDP terms depend on the hard assignment only: candidates that move a score without moving an assignment share them
        memo = self.__dict__.setdefault("_lin_memo", {})
        key = (lab.tobytes(), prs.tobytes(), n_cols, post, id(self.rho), id(self.transTheta))
        elbo_lin = memo.get(key)
        if elbo_lin is None:
            start = np.zeros(n_cols)
            if lab[0] < n_cols:
                start[lab[0]] = 1.0
            i, j = prs // K, prs % K
            ok = (i < n_cols) & (j < n_cols)
            trans = np.zeros((n_cols, n_cols))
            np.add.at(trans, (i[ok], j[ok]), 1.0)
            elbo_lin = memo[key] = self._elbo_linears_counts(start, trans, n_cols, post=post, one_sample=True) * 1
        sums = [float(v) for v in np.bincount(lab[lab < n_cols], minlength=n_cols)]
        tot = sum(sums)
        elbo_lds = 0.0
        for k in range(n_cols):
            if sums[k] > 0:
                elbo_lds += lds[k] * (sums[k] / tot)
        elbo_lds = elbo_lds * 1.0                    # one lead: its share of the n_points = 1 sample is 1 (frac of GPI_HDP.py:1820-1826)
        q_bas = q_sum * self.static_factor
        elbo_latent = lat_sum * self.dynamic_factor
        return q_bas, (elbo_lin + elbo_lds + elbo_latent) if self.hmm_switch else elbo_latent

    def _eager_candidates(self, ld, t, x, y, n_hist):
        """The candidates one by one (a copy of every cluster takes the beat: GPI_HDP.py:2040-2056) - the path for beats off the
        basis grid; same result as online_chain.OnlinePool.candidates (the new cluster's own terms are left to the caller)."""
        est, cols, lds = [], [], []
        for g in self.gpmodels[ld]:
            cand = self.gpmodel_deepcopy(g)
            est.append(self.estimate_new(t, cand, x, y[:, [ld]], h=1.0))
            cand.include_weighted_sample(t, x, x, y[:, [ld]], 1.0)
            cand.backwards_pair(1.0)
            cand.bayesian_new_params(1.0)
            cols.append(cand.compute_q_lat_all(n_hist, h_ini=1.0))
            lds.append(cand.lds_param_likelihood_value())
        return Candidates(torch.stack(est), torch.stack(cols, dim=1), lds, None, None)

    # ------------------------------------------------------------------ include_sample, phase by phase (b: the beat's record)
    def include_sample(self, x_train, y, with_warp=True, force_model=None, minibatch=0, classify=False):
        """GPI_HDP.py:1906-2208.  Same decisions in the same order as the reference; what it evaluates one candidate after the
        other - the clusters with the beat added, and the local step + bound of every candidate's score table - is computed side
        by side (online_chain.OnlinePool.candidates, _local_terms_many) before the accept / reject walk.  One helper per phase,
        in the reference's order; what a phase leaves for the later ones travels in the beat's record b (_begin_beat)."""
        self._online_guards(with_warp, classify, minibatch)
        _tick("outside")
        b = self._begin_beat(x_train, y)
        self._score_current(b)
        _tick("scores")
        if b.t > 0:
            self._propose(b)
            _tick("candidates")
            self._score_tables(b)
            _tick("local_terms")
            self._walk_bounds(b)
            _tick("bounds")
        else:
            b.q_chos, b.q_lat_chos = b.q_aux, b.q_lat
            b.resp, b.resplog, b.respPair, _ = self.variational_local_terms(b.q_aux, self.transTheta, self.startTheta, b.liks)
        self._apply_choice(b, force_model)
        _tick("reorder")
        # the members' update of this beat (GPI_HDP.py:2186-2196, after the global step there): nothing below up to that point
        # reads the cluster models, and nothing in the update reads the HDP parameters, so its launches go out first and run
        # under the host-side optimisation of (rho, omega); finish_commit (in _record) reads their status after it
        committed = self._member_update(b)
        self._global_step(b)
        _tick("rho_omega")
        self._record(b, committed)
        _tick("commit")

    def _online_guards(self, with_warp, classify, minibatch):
        if self.model_type_def == 'static' or any(t == 'static' for t in self.model_type):
            # the reference's online static branch re-estimates Sigma through inv_wishart.posterior (GPI_model.py:1022-1043,
            # 1084-1110): a step of its own, not the dynamic one with Gamma = 0
            raise NotImplementedError("include_sample with static models (model_type='static') is not built: the online step "
                                      "covers dynamic clusters only; static models run offline (include_batch, "
                                      "reload_model_from_labels, cluster_new_batch)")
        if with_warp:
            # The reference itself cannot run this path: with one cluster (the second beat of any run) compute_warp_y's greedy
            # branch takes torch.max of an empty tensor (GPI_HDP.py:3313, liks[:-1] with M = 1) and raises RuntimeError -
            # hdpgpc/tests/test_online_warp.py stops there (tests/golden/make_golden.py `onlinew` reproduces it).  There is no
            # reference behaviour to mirror; the batched warp fit itself (hgp_warp_batch_f64) serves include_batch(warp=True).
            raise NotImplementedError("include_sample(with_warp=True): the reference's own path raises at its second beat "
                                      "(GPI_HDP.py:3313); not built")
        if classify:
            raise NotImplementedError("include_sample(classify=True) has no caller in the reference and is not built")
        if self.n_outputs != 1:
            raise NotImplementedError("include_sample: one lead (the reference's reorder() aliases the per-lead model lists)")
        if not self.bayesian_params or minibatch:
            raise NotImplementedError("include_sample: only the Bayesian one-step parameter update is built (bayesian_params=True, "
                                      "minibatch=0); the reference's new_params_weighted path (GPI_HDP.py:2195) is not")

    def _begin_beat(self, x_train, y):
        """Set-up: the beat joins the history; its record with the empty score tables q_aux (-inf; the history's rows from the
        last beat) and q_lat (0), [T_all, M + 1, D] each - the last column is the would-be new cluster's."""
        D, dev = self.n_outputs, self.device
        self._lin_memo = {}
        t, M = self.T, self.M
        self.T = T_all = t + 1
        self.snr_norm = torch.ones((T_all, D), dtype=f64, device=dev)
        y = self.cond_to_torch(y).reshape(-1, D)
        x = self.cond_to_torch(x_train).reshape(-1, 1)
        self.y.append(y)
        self.x_train.append(x)
        b = SimpleNamespace(ld=0, t=t, T_all=T_all, M=M, K=M + 1, x=x, y=y, liks=np.zeros(M + 1), pool=None, info0=None,
                            n_hist=torch.empty((T_all, 0)),                # compute_q_lat_all only reads the history length
                            q_aux=torch.full((T_all, M + 1, D), -np.inf, dtype=f64, device=dev),
                            q_lat=torch.zeros((T_all, M + 1, D), dtype=f64, device=dev))
        if t > 0:
            prev = self.q[-1]
            b.q_aux[:-1, :prev.shape[1], :] = prev
        return b

    def _score_current(self, b):
        """The beat under the current clusters (GPI_HDP.py:1973): the last row of q_aux, the clusters' columns of q_lat."""
        ld, M, mods = b.ld, b.M, self.gpmodels[b.ld]
        b.pool = self._online_pool(ld, b.x) if b.t > 0 else None           # the clusters as persistent chains (online_chain.py)
        if M > 0:
            b.q_lat[:, :M, ld] = torch.stack([gp.compute_q_lat_all(b.n_hist, h_ini=1.0) for gp in mods], dim=1)
        if b.pool is not None:
            b.q_aux[-1, :M, ld], b.info0 = b.pool.begin_beat(b.y[:, ld], mods)
        elif M > 0:
            b.q_aux[-1, :M, ld] = self._last_scores(b.x, b.y, ld)

    def _propose(self, b):
        """The provisional new cluster (GPI_HDP.py:1990-1996) and, when it scores the beat best, every cluster with the beat
        added (b.cand, else None).  How well does each existing cluster explain the beat?  candidates are tried best first
        (b.order); the worst one lends its kernel and priors to the would-be new cluster."""
        ld, M, t = b.ld, b.M, b.t
        last_row = self.weight_mean(b.q_aux)[-1, :-1]
        if b.info0 is not None:                                            # the scores' LAPACK status rides the same round trip
            host = torch.cat([last_row, b.info0.to(f64)]).cpu()
            if bool(host[M:].any()):
                ops.raise_on_info(b.info0, "log_sq_error")
            last_row = host[:M]
        q_ord = torch.argsort(last_row.cpu(), descending=True)
        b.q_prev, b.q_lat_prev = b.q_aux.clone(), b.q_lat.clone()
        prov = self.gpmodel_deepcopy(self.gpmodels[ld][int(q_ord[-1])])
        prov.reinit_GP(save_last=False)
        prov.reinit_LDS(save_last=False)
        prov._defer_checks = True                                    # its LAPACK statuses are read together, below
        b.q_prev[-1, -1, ld] = prov.estimate_new_and_include(t, b.x, b.y[:, [ld]]) + b.liks[-1]
        b.birth_best = int(torch.argmax(b.q_prev[-1])) == M          # the new cluster scores the beat best: is it worth it?
        b.order = q_ord.tolist() if b.birth_best else []
        b.lds_cur = [g.lds_param_likelihood_value() for g in self.gpmodels[ld]]
        b.cand = None
        if b.order and b.pool is not None:
            # the new cluster's own latent-transition score and parameter likelihoods ride the candidates' batched calls
            b.cand = b.pool.candidates(t, b.q_lat[:, :M, ld], extra=prov)
        elif b.order:
            b.cand = self._eager_candidates(ld, t, b.x, b.y, b.n_hist)
        if b.cand is not None and b.cand.extra_lds is not None:
            b.q_lat_prev[t, -1, ld], b.lds_prov = b.cand.extra_lat, b.cand.extra_lds
        else:
            b.q_lat_prev[:, -1, ld] = prov.compute_q_lat_all(b.n_hist, h_ini=1.0)
            b.lds_prov = float(prov.return_LDS_param_likelihood())
        prov._defer_checks = False
        prov._check_pending()

    def _score_tables(self, b):
        """Score tables of every evaluation of this beat, b.Qall / b.Lall [2 + R, T_all, K]: [0] current clusters, [1] with the new
        cluster, [2 + r] the r best clusters tried so far with the beat added (the reference's q_post is cumulative over its loop,
        GPI_HDP.py:2040-2075) - and the local step of all of them at once (b.lab, b.prs, b.last host, b.lab_dev)."""
        M, K, dev = b.M, b.K, self.device
        Qb, Lb = self.weight_mean(b.q_aux), self.weight_mean(b.q_lat)
        Qs, Ls = [Qb, self.weight_mean(b.q_prev)], [Lb, self.weight_mean(b.q_lat_prev)]
        if b.order:
            R = len(b.order)
            od = ops.to_dev(b.order, torch.int64, dev)
            tried = torch.zeros((R, K), dtype=torch.bool, device=dev)             # tried[r, m]: cluster m is among the r + 1 best
            tried[:, od] = torch.tril(torch.ones((R, R), dtype=torch.bool, device=dev))
            new_last = Qb[-1].clone()
            new_last[:M] = b.cand.est + ops.to_dev(b.liks[:M], f64, dev)
            Qc = Qb.unsqueeze(0).repeat(R, 1, 1)
            Qc[:, -1, :] = torch.where(tried, new_last[None, :], Qb[-1][None, :])
            cols_full = Lb.clone()
            cols_full[:, :M] = b.cand.cols
            Lc = torch.where(tried[:, None, :], cols_full[None], Lb[None])
            Qs += list(Qc.unbind(0))
            Ls += list(Lc.unbind(0))
        b.Qall, b.Lall = torch.stack(Qs), torch.stack(Ls)
        b.lab, b.prs, b.last, b.lab_dev = self._local_terms_many(b.Qall, b.liks)

    def _walk_bounds(self, b):
        """The sums of the bound over the assigned entries (all rows; all but the newest for the current clusters), the bound of
        every table and the accept / reject walk in the reference's order.  Leaves the kept table's resp, respPair, resplog,
        q_chos and q_lat_chos."""
        M, K, T_all, dev = b.M, b.K, b.T_all, self.device
        B = b.Qall.shape[0]
        n_cols = torch.full((B, 1), M, dtype=torch.int64, device=dev)
        n_cols[1] = M + 1
        valid = b.lab_dev < n_cols
        idx = torch.clamp(b.lab_dev, max=M)[..., None]
        zero = torch.zeros((), dtype=f64, device=dev)
        gq = torch.where(valid, b.Qall.gather(2, idx)[..., 0], zero)
        gl = torch.where(valid, b.Lall.gather(2, idx)[..., 0], zero)
        sums = torch.stack([torch.sum(gq[0, :-1]), torch.sum(gl[0, :-1])] + [v for i in range(1, B) for v in (torch.sum(gq[i]), torch.sum(gl[i]))])
        sums = sums.cpu().numpy().reshape(B, 2)
        bound = lambda i, rows, cols, lds, post: self._bound_from_labels(b.lab[i], b.prs[i], K, rows, cols, sums[i, 0], sums[i, 1], lds, post=post)   # noqa: E731
        q_all, elbo = bound(0, T_all - 1, M, b.lds_cur, False)
        q_prev_post, elbo_prev_post = bound(1, T_all, M + 1, b.lds_cur + [b.lds_prov], True)
        elbo_prev_post -= elbo
        q_prev_post -= q_all
        chosen = 0                                                  # index into Qall of the table that is kept
        if b.birth_best:
            chosen = 1
            for r, m in enumerate(b.order):
                lds_r = list(b.lds_cur)
                lds_r[m] = b.cand.lds[m]                            # only the cluster being tried is the candidate's (GPI_HDP.py:2071)
                q_bas_post, elbo_bas_post = bound(2 + r, T_all, M, lds_r, False)
                elbo_bas_post -= elbo
                q_bas_post -= q_all
                if q_bas_post + elbo_bas_post > q_prev_post + elbo_prev_post:
                    chosen = 2 + r
                    break
        b.resp, b.respPair = _tables(b.lab[chosen], b.prs[chosen], K)
        b.resplog = b.last[chosen]
        b.q_chos, b.q_lat_chos = b.Qall[chosen].unsqueeze(-1).clone(), b.Lall[chosen].unsqueeze(-1).clone()

    def _apply_choice(self, b, force_model):
        """The newest row's cluster (b.force: forced by the caller or by the cap max_models, else None), birth, clusters by
        size, and the counts of the global step (b.start_count, b.trans_count)."""
        model = int(np.argmax(b.resp[-1].numpy()))
        if self.max_models is not None and model >= self.max_models:
            force_model = int(np.argmax(b.resplog[:-1]))
        b.force = None if force_model is None else int(force_model)
        if b.force is not None:
            model = b.force
            _assign_newest(model, b.resp[-1].numpy())                # a view: the edit lands in the table, as in the reference
        birth = model == self.M
        if birth:
            self._log("Birth of new model: ", self.M + 1)
            self.M = self.M + 1
            for ld in range(self.n_outputs):
                self.gpmodels[ld].append(self.create_gp_default())
            self.x_basis.append(self.x_basis_ini)
        if birth or b.force is None:                     # quirk: a forced beat that opens no cluster leaves the clusters unsorted
            b.resp, b.respPair, b.q_chos, b.q_lat_chos, _ = self.reorder(b.resp, b.respPair, b.q_chos, b.q_lat_chos)
        M = self.M                                       # (after a birth the tables have exactly M columns)
        b.start_count, b.trans_count = b.resp[0, :M].numpy().copy(), torch.sum(b.respPair[:, :M, :M], dim=0).numpy()

    def _member_update(self, b):
        """The beat joins its cluster (weight 1; the others take it with weight 0: GPI_HDP.py:2186-2196): on the cluster's
        persistent chain when it has one.  Returns the pool with a commit in flight (finish_commit reads its status), or None."""
        ld, D, pool = b.ld, self.n_outputs, b.pool
        resp_mod = b.resp[-1].numpy()
        if b.force is not None:
            resp_mod = resp_mod.copy()
            _assign_newest(b.force, resp_mod)
        committed = None
        for m in range(self.M):
            h = float(resp_mod[m])
            gp = self.gpmodels[ld][m]
            chained = pool is not None and h == 1.0 and gp.N >= 1 and pool.holds(gp)
            if chained:               # the cluster's persistent chain takes the member step (Kalman + both MNIW updates)
                pool.commit(gp, b.t, b.x, b.y[:, [ld]])
                committed = pool
            else:
                gp.include_weighted_sample(b.t, b.x, b.x, b.y[:, [ld]], h)
            if h > 0.9:
                row = b.y.reshape(1, -1, D)
                self.y_train = row if self.y_train.numel() == 0 else torch.cat([self.y_train, row])
            if not chained:
                gp.bayesian_new_params(h, model_type=self.model_type_def)
        return committed

    def _global_step(self, b):
        """The HDP global step from the beat's counts (GPI_HDP.py:2115-2128) and the transition matrix."""
        M = self.M
        if M > 2:
            self.reinit_global_params(M - 1, b.trans_count, b.start_count)
        if M >= 2:
            for _ in range(4):
                self.transTheta, self.startTheta = self._calcThetaFull(b.trans_count, b.start_count, M)
                self.rho, self.omega = self.find_optimum_rhoOmega()
        self.trans_A = torch.as_tensor(_log_trans(self.transTheta, M))

    def _record(self, b, committed):
        """The beat's state, its row of the tables (forced: in every table, GPI_HDP.py:2168-2178) and the history."""
        M = self.M
        model = int(np.argmax(b.resp[-1].numpy())) if b.force is None else b.force
        if b.force is not None:
            _assign_newest(model, b.resp[-1].numpy(), b.respPair, b.q_chos, b.q_lat_chos)
        self.actual_state = model
        self._log("Main model chosen:", model + 1)
        if committed is not None:
            committed.finish_commit()
        if self.verbose:
            self.compute_q_elbo(b.resp[:, :M], b.respPair[:, :M, :M], self.weight_mean(b.q_chos)[:, :M], self.weight_mean(b.q_lat_chos)[:, :M],
                                self.gpmodels, self.M, snr='saved', post=False, one_sample=True)
        self.resp_assigned.append(torch.argmax(b.resp, dim=1))
        self.q.append(b.q_chos)


# ---------------------------------------------------------------------- small host-side pieces both loops use (offline_loop imports them)
def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)


def _log_trans(transTheta, M, eps=None):
    """log transition matrix of the leading M states from the Dirichlet pseudo-counts, rows normalised over M + 1 columns
    (GPI_HDP.py:1188 and its repeats).  quirk: some of the reference's copies add 1e-5 inside the logarithm and some do not -
    every caller passes its own (offline_loop.py, GPI_HDP.reload_model_from_labels, include_sample)."""
    tt = _np(transTheta)
    norm = np.sum(np.exp(_digamma(tt[:M, :M + 1])), axis=1)
    return _digamma(tt[:M, :M]) - np.log(norm if eps is None else norm + eps)[:, None]


def _by_size(resp):
    """Clusters largest first: (the permutation, the one-hot table resp with its columns permuted)."""
    order = torch.argsort(torch.sum(resp, dim=0), descending=True)
    return order, resp[:, order]


def _tables(labels, pairs, K):
    """One-hot host tables resp [N, K], respPair [N, K, K] of a hard assignment (labels [N], flat pair indexes [N]: host tensors
    or arrays) - where OfflineLoop._one_hot_tables and include_sample both end."""
    N = labels.shape[0]
    resp = torch.zeros((N, K), dtype=f64)
    resp[torch.arange(N), torch.as_tensor(labels)] = 1.0
    respPair = torch.zeros((N, K * K), dtype=f64)                             # the reference's table is float32: 0 / 1 either way
    respPair[torch.arange(N), torch.as_tensor(pairs)] = 1.0
    return resp, respPair.reshape(N, K, K)


def _assign_newest(model, resp_row, respPair=None, q=None, q_lat=None):
    """The forced assignment of include_sample: the newest row belongs to `model` (the caller's force_model, or the best existing
    cluster when the cap max_models forbids a birth), written into the tables given - resp_row: the newest row of resp (a view
    edits the table; a copy leaves it alone), respPair, and the score matrices q / q_lat, where the row's maximum goes to the
    forced cluster (GPI_HDP.py:2168-2178).  The reference itself raises on this path unless the beat opens a cluster
    (GPI_HDP.py:2187: `reorder` is bound only by the two self.reorder(...) calls, which the forced no-birth branch skips -
    UnboundLocalError); there the clusters keep their order, and that identity order is the definition (pinned by
    tests/golden/include_sample_r102_forced_mirror.npz)."""
    resp_row[:] = 0.0
    resp_row[model] = 1.0
    if q is not None:
        q[-1, model] = torch.max(q[-1])
        q_lat[-1, model] = torch.max(q_lat[-1])
        respPair[-1, model, :] = 0.0
        respPair[-1, :, model] = 0.0
        respPair[-1, model, model] = 1.0


# phase timing of include_sample (tools/time_online.py --phases): HGP_ONLINE_TIMING=1 synchronises at every phase boundary
TIMING = {}
_T_ON = ops.env_flag("HGP_ONLINE_TIMING")
_t_last = [0.0]


def _tick(name):
    if not _T_ON:
        return
    import time
    torch.cuda.synchronize()
    now = time.perf_counter()
    TIMING[name] = TIMING.get(name, 0.0) + now - _t_last[0]
    _t_last[0] = now
