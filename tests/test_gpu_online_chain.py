"""hdpgpc_amd/online_chain.py (BASELINE configs[4]): the online step's candidates and commits on persistent chains against the
one-by-one GPI_model methods (GPI_model.py:325-375,705-716,966-1115 restated call by call) on the same state.

The end-to-end gate is tests/test_gpu_include_sample.py (the reference's own traces); here the pool's pieces are held to the
one-by-one path directly: estimate_new's score, the candidate's latent-transition column, its MNIW parameter likelihood, and the
state a commit leaves behind, for clusters with one, two and several members, at T = 90 (riding inversions) and T = 144 / 256
(cooperative inversions with the workspace).  Below that, at T = 33: the slots' lifecycle - a model changed or
replaced behind its chain's back, the pool growing with a skipped update on record or a commit in flight, stacks that move -
and the one-by-one commit of a beat off the basis grid."""
import types

import numpy as np
import pytest
import torch

from conftest import golden, rel_err, relclose

pytestmark = pytest.mark.gpu


def _models(T, sizes, seed=3):
    """Clusters grown one beat at a time with the one-by-one methods (include_weighted_sample + bayesian_new_params, as the
    online commit does), from resampled beats of record 100."""
    import hdpgpc.GPI_HDP as hdpgp
    y90 = golden("mitbih100_lead0.npz")["y"][:64]
    tt = np.linspace(0, y90.shape[1] - 1, T)
    Y = np.stack([np.interp(tt, np.arange(y90.shape[1]), r) for r in y90])
    xb = np.arange(float(T))[:, None]
    std, std_dif = float(np.std(Y[:30], axis=0).mean()), float(np.std(np.diff(Y[:30], axis=0), axis=0).mean())
    sw = hdpgp.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif,
                       ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=(std * 1e-5, std * 2),
                       bound_gamma=(std_dif * 1e-5, std_dif * 2), bound_noise_warp=(std * 0.01, std * 0.02), verbose=False,
                       max_models=100, bayesian_params=True, free_deg_MNIV=20)
    sw.fixed_theta = (341.0, 1.2, 4.66)
    rng = np.random.default_rng(seed)
    x = torch.as_tensor(xb, device=sw.device)
    models, used = [], 0
    for n in sizes:
        g = sw.create_gp_default()
        for j in range(n):
            yy = torch.as_tensor(Y[used] + 0.05 * rng.standard_normal(T), device=sw.device).reshape(-1, 1)
            g.include_weighted_sample(used, x, x, yy, 1.0)
            g.bayesian_new_params(1.0)
            used += 1
        models.append(g)
    return sw, models, x, torch.as_tensor(Y[used], device=sw.device).reshape(-1, 1), used


def _one_by_one(sw, g, x, y, t_new, T_all):
    cand = sw.gpmodel_deepcopy(g)
    mean_, cov_, C_, Sigma_ = cand.smoother_weighted(x, y, 1.0)
    est = cand.log_sq_error(x, y, mean=mean_[-1], cov=cov_[-1], C=C_[-1], Sigma=Sigma_[-1], i=-1, first=len(cand.indexes) == 1)
    cand.include_weighted_sample(t_new, x, x, y, 1.0)
    cand.backwards_pair(1.0)
    cand.bayesian_new_params(1.0)
    return float(est), cand.compute_q_lat_all(torch.empty((T_all, 0))).cpu().numpy(), float(cand.lds_param_likelihood_value()), cand


@pytest.mark.parametrize("T", [90, 144, 256])
def test_candidates_and_commit_match_the_one_by_one_path(T):
    from hdpgpc_amd.online_chain import OnlinePool
    sizes = [1, 2, 5, 3] if T > 128 else [1, 2, 7, 3, 4, 2, 1, 6, 2]         # the second set grows the pool past its first capacity
    sw, models, x, y, t_new = _models(T, sizes)
    T_all = t_new + 1
    hist = torch.empty((T_all, 0))
    ref = [_one_by_one(sw, g, x, y, t_new, T_all) for g in models]
    pool = OnlinePool(T, sw.device, sw.annealing_def, cap=4)
    for g in models:
        assert pool.supports(g)
        pool.adopt(g)
    cols0 = torch.stack([g.compute_q_lat_all(hist) for g in models], dim=1).contiguous()
    before = [[t.clone() for t in (g.f_star_sm[-1], g.cov_f_sm[-1], g.A[-1], g.Sigma[-1], g.internal_params.scale)] for g in models]
    sc, info = pool.begin_beat(y[:, 0], models)
    assert int(info.abs().max()) == 0
    for c, g in enumerate(models):                 # the beat under every cluster's last state: log_sq_error(x, y, i=-1)
        want = float(g.log_sq_error(x, y, i=-1))
        assert abs(float(sc[c]) - want) <= 1e-9 * abs(want)
    est, cols, lds = pool.candidates(t_new, cols0)[:3]
    est, cols = est.cpu().numpy(), cols.cpu().numpy()
    for c, (e_ref, col_ref, lds_ref, _) in enumerate(ref):
        assert abs(est[c] - e_ref) <= 1e-9 * abs(e_ref), (c, est[c], e_ref)
        assert rel_err(cols[:, c][col_ref != 0], col_ref[col_ref != 0]) <= 1e-8 and np.array_equal(cols[:, c] == 0, col_ref == 0)
        assert abs(lds[c] - lds_ref) <= 1e-8 * abs(lds_ref)
    # a dry run leaves every cluster exactly as it was
    for g, b in zip(models, before):
        for now, was in zip((g.f_star_sm[-1], g.cov_f_sm[-1], g.A[-1], g.Sigma[-1], g.internal_params.scale), b):
            assert torch.equal(now, was)
    # commit: the cluster that takes the beat, against include_weighted_sample + bayesian_new_params on a copy
    for c in (0, 2):
        g = models[c]
        twin = sw.gpmodel_deepcopy(g)
        twin.include_weighted_sample(t_new, x, x, y, 1.0)
        twin.bayesian_new_params(1.0)
        pool.commit(g, t_new, x, y)
        pool.finish_commit()
        assert g.N == twin.N and g.indexes == twin.indexes and len(g.f_star) == len(twin.f_star)
        for name in ("f_star", "f_star_sm", "cov_f", "cov_f_sm", "A", "Gamma", "C", "Sigma"):
            a, b = torch.stack(list(getattr(g, name))).cpu().numpy(), torch.stack(list(getattr(twin, name))).cpu().numpy()
            assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b)), (name, c)
        assert g.internal_params.n0 == twin.internal_params.n0
        for a, b in ((g.internal_params.scale, twin.internal_params.scale), (g.observation_params.scale, twin.observation_params.scale),
                     (g.observation_params.m_mean, twin.observation_params.m_mean)):
            assert relclose(a.cpu().numpy(), b.cpu().numpy(), 1e-9)
        la, lb = g.compute_q_lat_all(hist).cpu().numpy(), twin.compute_q_lat_all(hist).cpu().numpy()
        assert rel_err(la[lb != 0], lb[lb != 0]) <= 1e-8
        assert abs(g.lds_param_likelihood_value() - twin.lds_param_likelihood_value()) <= 1e-8 * abs(twin.lds_param_likelihood_value())
    # and a second round of candidates on the grown chains (rows were appended, one slot was committed twice over its lists)
    y2 = (y * 0.97 + 0.3).contiguous()
    ref2 = [_one_by_one(sw, g, x, y2, t_new + 1, T_all + 1) for g in models]
    hist2 = torch.empty((T_all + 1, 0))
    cols1 = torch.stack([g.compute_q_lat_all(hist2) for g in models], dim=1).contiguous()
    pool.begin_beat(y2[:, 0], models)
    est2, cols2, lds2 = pool.candidates(t_new + 1, cols1)[:3]
    for c, (e_ref, col_ref, lds_ref, _) in enumerate(ref2):
        assert abs(float(est2[c]) - e_ref) <= 1e-9 * abs(e_ref)
        got = cols2[:, c].cpu().numpy()
        assert rel_err(got[col_ref != 0], col_ref[col_ref != 0]) <= 1e-8
        assert abs(lds2[c] - lds_ref) <= 1e-8 * abs(lds_ref)


# ---------------------------------------------------------------------- the pool's slot lifecycle (T = 33: no multiple of 16,
# riding inversions; what goes wrong here is host-side bookkeeping and does not depend on T)
_LISTS = ("f_star", "f_star_sm", "cov_f", "cov_f_sm", "A", "Gamma", "C", "Sigma")


def _twin_commit(twin, t, x, y):
    twin.include_weighted_sample(t, x, x, y, 1.0)
    twin.bayesian_new_params(1.0)


def _beats(y, n, seed=11):
    """n further beats: the beat y rescaled, shifted and with fresh noise."""
    rng = np.random.default_rng(seed)
    noise = torch.as_tensor(rng.standard_normal((n,) + tuple(y.shape)), device=y.device)
    return [(y * (1.0 - 0.02 * k) + 0.1 * k + 0.05 * noise[k]).contiguous() for k in range(n)]


def _assert_same_cluster(g, twin, T_all, tag):
    """The cluster g (on a pool's chain) against its one-by-one twin: members, the eight per-step lists and both MNIW
    distributions (1e-9), the latent-transition column and the parameter likelihood (1e-8)."""
    assert g.N == twin.N and g.indexes == twin.indexes and len(g.f_star) == len(twin.f_star), tag
    for name in _LISTS:
        assert len(getattr(g, name)) == len(getattr(twin, name)), (tag, name)
        a, b = torch.stack(list(getattr(g, name))).cpu().numpy(), torch.stack(list(getattr(twin, name))).cpu().numpy()
        assert np.max(np.abs(a - b)) <= 1e-9 * np.max(np.abs(b)), (tag, name, np.max(np.abs(a - b)) / np.max(np.abs(b)))
    eye = torch.eye(g.x_basis.shape[0], dtype=torch.float64, device=g.device)
    for par in ("internal_params", "observation_params"):
        a, b = getattr(g, par), getattr(twin, par)
        assert float(a.n0) == float(b.n0), (tag, par, float(a.n0), float(b.n0))
        for field in ("m_mean", "scale", "m_r_cov"):
            va, vb = (eye if getattr(p, field) is None else getattr(p, field) for p in (a, b))
            assert relclose(va.cpu().numpy(), vb.cpu().numpy(), 1e-9), (tag, par, field)
    hist = torch.empty((T_all, 0))
    la, lb = g.compute_q_lat_all(hist).cpu().numpy(), twin.compute_q_lat_all(hist).cpu().numpy()
    assert np.array_equal(la == 0, lb == 0) and rel_err(la[lb != 0], lb[lb != 0]) <= 1e-8, tag
    assert abs(g.lds_param_likelihood_value() - twin.lds_param_likelihood_value()) <= 1e-8 * abs(twin.lds_param_likelihood_value()), tag


def _assert_same_beat(sw, pool, models, twins, x, y, t_new):
    """One beat's scores and candidates (through the pool; pool None: through the one-by-one path of the online loop, which
    reads sw.gpmodels[0]) against the one-by-one methods on the twins, cluster by cluster in the order of `models`."""
    T_all = t_new + 1
    hist = torch.empty((T_all, 0))
    ref = [_one_by_one(sw, tw, x, y, t_new, T_all) for tw in twins]
    cols0 = torch.stack([g.compute_q_lat_all(hist) for g in models], dim=1).contiguous()
    if pool is not None:
        sc, info = pool.begin_beat(y[:, 0], models)
        assert int(info.abs().max()) == 0
        est, cols, lds = pool.candidates(t_new, cols0)[:3]
    else:
        assert sw.gpmodels[0] is models
        sc = sw._last_scores(x, y, 0)
        est, cols, lds = sw._eager_candidates(0, t_new, x, y, hist)[:3]
    assert sc.shape[0] == est.shape[0] == cols.shape[1] == len(lds) == len(models)
    sc, est, cols = sc.cpu().numpy(), est.cpu().numpy(), cols.cpu().numpy()
    for c, (tw, (e_ref, col_ref, lds_ref, _)) in enumerate(zip(twins, ref)):
        want = float(tw.log_sq_error(x, y, i=-1))
        assert abs(sc[c] - want) <= 1e-9 * abs(want), (c, sc[c], want)
        assert abs(est[c] - e_ref) <= 1e-9 * abs(e_ref), (c, est[c], e_ref)
        assert rel_err(cols[:, c][col_ref != 0], col_ref[col_ref != 0]) <= 1e-8 and np.array_equal(cols[:, c] == 0, col_ref == 0), c
        assert abs(lds[c] - lds_ref) <= 1e-8 * abs(lds_ref), (c, lds[c], lds_ref)


def _pool_commit(pool, g, twin, t, x, y, T_all, tag):
    _twin_commit(twin, t, x, y)
    pool.commit(g, t, x, y)
    pool.finish_commit()
    _assert_same_cluster(g, twin, T_all, tag)


def test_eager_commit_on_an_adopted_model_is_seen():
    """A beat off the basis grid is committed with include_weighted_sample + bayesian_new_params on a model whose lists are views
    of a slot's stacks (OnlineLoop._member_update without a pool): the lists turn into real lists and the cluster grows, the slot
    knows nothing of it.  The next time the loop asks for the pool, the slot must describe the cluster as it is now."""
    sw, models, x, y, t0 = _models(33, [1, 3, 2])
    twins = [sw.gpmodel_deepcopy(g) for g in models]
    sw.gpmodels[0] = models
    pool = sw._online_pool(0, x)
    assert pool is not None and all(pool.holds(g) for g in models)
    ys = _beats(y, 5)
    for g in (models[1], twins[1]):
        _twin_commit(g, t0, x, ys[0])
    pool = sw._online_pool(0, x)
    assert pool is not None and all(pool.holds(g) for g in models) and len(pool.slots) == len(models)
    _assert_same_beat(sw, pool, models, twins, x, ys[1], t0 + 1)
    for k, c in enumerate((1, 0, 2)):                        # the mutated cluster first
        _pool_commit(pool, models[c], twins[c], t0 + 1 + k, x, ys[2 + k], t0 + 2 + k, ("commit", c))
    assert sw._online_pool(0, x) is pool and len(pool.slots) == len(models)       # chain commits leave the slots valid


@pytest.mark.parametrize("how", ["permuted", "one_more"])
def test_replaced_model_list_gets_fresh_slots(how):
    """The model list of a lead is replaced by copies (as include_batch and reload_model_from_labels do) while a pool is
    alive: the copies carry no slot, the old slots describe models that are gone.  The pool the loop hands out next has one slot
    per model of the NEW list (or the loop takes the one-by-one path), and answers in the new list's order."""
    sw, built, x, y, t0 = _models(33, [2, 1, 3, 2])
    models, spare = built[:3], built[3]
    twins = [sw.gpmodel_deepcopy(g) for g in built]
    sw.gpmodels[0] = models
    ys = _beats(y, 4)
    pool = sw._online_pool(0, x)
    _assert_same_beat(sw, pool, models, twins[:3], x, ys[0], t0)           # one pooled beat, committed to cluster 0
    _pool_commit(pool, models[0], twins[0], t0, x, ys[0], t0 + 1, "first")
    order = [2, 0, 1] if how == "permuted" else [0, 1, 2, 3]
    new = [sw.gpmodel_deepcopy((models + [spare])[i]) for i in order]
    new_twins = [twins[i] for i in order]
    assert all(getattr(g, "_slot", None) is None for g in new)
    sw.gpmodels[0] = new
    pool = sw._online_pool(0, x)
    assert pool is None or (len(pool.slots) == len(new) and all(pool.holds(g) for g in new))
    _assert_same_beat(sw, pool, new, new_twins, x, ys[1], t0 + 1)
    if pool is not None:
        for k, c in enumerate((0, len(new) - 1)):
            _pool_commit(pool, new[c], new_twins[c], t0 + 1 + k, x, ys[2 + k], t0 + 2 + k, ("commit", c))


def _skipping(sw, g):
    """Make the cluster's MNIW update skip (GPI_model.py:1068-1071 keeps the previous distributions when a factorisation of
    the update fails): a right covariance of the internal distribution that is negative definite by far more than the 1e-2
    mean|diag(scale)| jitter of the update can repair.  Finite inputs; the filter step itself does not read it."""
    ip = g.internal_params
    jitter = 1e-2 * float(torch.mean(torch.diagonal(ip.scale).abs()))
    ip.m_r_cov = -(100.0 * jitter + 1.0) * torch.eye(ip.scale.shape[0], dtype=torch.float64, device=ip.scale.device)


def test_grow_keeps_the_skipped_update_count():
    """The host keeps, per slot, how many MNIW updates the device has skipped so far (finish_commit: `updated` = the device's
    count did not move).  Growing the pool gives every slot new status words: the count must survive it, or the host's n0 and the
    device's part ways at the next commit."""
    from hdpgpc_amd.online_chain import OnlinePool
    sw, models, x, y, t0 = _models(33, [2, 2, 2])
    _skipping(sw, models[0])
    twins = [sw.gpmodel_deepcopy(g) for g in models]
    ys = _beats(y, 4)
    # the yardstick itself skips: same distribution objects, same count, and still one more row in every list
    probe = sw.gpmodel_deepcopy(models[0])
    was = (probe.internal_params, probe.observation_params, float(probe.internal_params.n0), len(probe.A))
    _twin_commit(probe, t0, x, ys[0])
    assert probe.internal_params is was[0] and probe.observation_params is was[1]
    assert float(probe.internal_params.n0) == was[2] and len(probe.A) == was[3] + 1
    pool = OnlinePool(33, sw.device, sw.annealing_def, cap=2)
    for g in models[:2]:
        assert pool.supports(g)
        pool.adopt(g)
    n0 = float(models[0].internal_params.n0)
    _pool_commit(pool, models[0], twins[0], t0, x, ys[0], t0 + 1, "skipped, before the growth")
    assert float(models[0].internal_params.n0) == n0 and float(pool.slots[0].ch.n0) == n0
    pool.adopt(models[2])                                                   # past the capacity: the pool grows
    assert pool.cap == 4 and len(pool.slots) == 3
    _pool_commit(pool, models[0], twins[0], t0 + 1, x, ys[1], t0 + 2, "skipped, after the growth")
    assert float(models[0].internal_params.n0) == n0 and float(pool.slots[0].ch.n0) == n0
    _pool_commit(pool, models[1], twins[1], t0 + 2, x, ys[2], t0 + 3, "healthy, after the growth")
    assert float(pool.slots[1].ch.n0) == float(twins[1].internal_params.n0)
    _assert_same_beat(sw, pool, models, twins, x, ys[3], t0 + 3)


def test_commit_pending_across_grow():
    """commit() leaves its two status words to finish_commit(); adopting a cluster past the capacity in between replaces the
    status buffers.  The words finish_commit() reads must be the committed step's: here that step SKIPS its MNIW update, which
    only those words tell the host."""
    from hdpgpc_amd.online_chain import OnlinePool
    sw, models, x, y, t0 = _models(33, [2, 3, 1])
    _skipping(sw, models[0])
    twins = [sw.gpmodel_deepcopy(g) for g in models]
    ys = _beats(y, 3)
    pool = OnlinePool(33, sw.device, sw.annealing_def, cap=2)
    pool.adopt(models[0]), pool.adopt(models[1])
    n0 = float(models[0].internal_params.n0)
    _twin_commit(twins[0], t0, x, ys[0])
    assert float(twins[0].internal_params.n0) == n0                          # the yardstick skipped
    pool.commit(models[0], t0, x, ys[0])
    pool.adopt(models[2])                                                   # grows with the commit in flight
    assert pool.cap == 4
    pool.finish_commit()
    _assert_same_cluster(models[0], twins[0], t0 + 1, "pending across the growth")
    assert float(pool.slots[0].ch.n0) == n0
    # and a healthy commit in flight across the next adoption (no growth), then the whole pool for one beat
    _twin_commit(twins[1], t0 + 1, x, ys[1])
    pool.commit(models[1], t0 + 1, x, ys[1])
    pool.finish_commit()
    _assert_same_cluster(models[1], twins[1], t0 + 2, "healthy")
    _assert_same_beat(sw, pool, models, twins, x, ys[2], t0 + 2)


@pytest.mark.parametrize("T", [33, 144])
def test_more_rows_under_repeated_commits(T):
    """A slot starts with max(8, 2 L) rows; a one-member cluster that absorbs eight beats in a row outgrows them, and the stacks
    move (OnlinePool._more_rows) under the model's lists, the launch tables and the memoised latent-transition scores.
    T = 144 takes the cooperative inversions with the workspace."""
    from hdpgpc_amd.online_chain import OnlinePool
    sw, models, x, y, t0 = _models(T, [1, 2])
    twins = [sw.gpmodel_deepcopy(g) for g in models]
    ys = _beats(y, 9)
    pool = OnlinePool(T, sw.device, sw.annealing_def, cap=4)
    for g in models:
        pool.adopt(g)
    rows0 = pool.slots[0].rows
    models[0].compute_q_lat_all(torch.empty((t0, 0)))                        # the memo a commit carries forward
    for k in range(8):
        _pool_commit(pool, models[0], twins[0], t0 + k, x, ys[k], t0 + k + 1, ("commit", k))
    assert pool.slots[0].rows >= 2 * rows0 and models[0].N == 9
    _assert_same_beat(sw, pool, models, twins, x, ys[8], t0 + 8)


def _obs_update_ref(K, xb, xo, y, f_sm, m_mean, m_r_cov, n0, scale):
    """The one-step observation update for a member on the grid xo in plain numpy (GPI_model.py:1037-1041,1065,1300-1344 restated):
    the latent mean resampled on xo, both samples projected back onto the basis, zero covariance corrections."""
    T = xb.shape[0]
    eye = np.eye(T)
    f_off = K(xo, xb) @ np.linalg.solve(K(xb, xb) + 1e-4 * eye, f_sm)
    P = np.linalg.solve(K(xo, xo) + 1e-4 * eye, K(xo, xb)).T
    y1, y2 = P @ y, P @ f_off
    scale_inv = np.linalg.inv(0.5 * (m_r_cov + m_r_cov.T) + 1e-2 * np.mean(np.abs(np.diag(scale))) * eye)
    S__ = y2 @ y2.T + scale_inv
    S_ = y1 @ y2.T + m_mean @ scale_inv
    part = np.linalg.solve(0.5 * (S__ + S__.T) + 1e-8 * eye, S_.T).T
    e = y1 - y2
    return ((n0 - 2) * m_mean + part) / (n0 - 1), S__, ((n0 - 2) * scale + e @ e.T) / (n0 - 1)


def test_one_by_one_commit_off_the_grid_projects_the_observation_update():
    """The commit of a beat off the basis grid (include_weighted_sample + bayesian_new_params, OnlineLoop._member_update): the
    observation MNIW update reads the beat against the latent mean RESAMPLED on the beat's grid, both projected onto the basis
    (GPI_model.py:1037-1041,1065) - against the same update in plain numpy.  Bound: 1e-9 as for the states above, or 50 x what
    the numpy result itself moves under a 1e-15 relative perturbation of its inputs where that is more."""
    sw, models, x, y, t0 = _models(33, [2])
    g = models[0]
    xo = x + 0.3
    old = g.observation_params
    g.include_weighted_sample(t0, xo, xo, y, 1.0)
    g.bayesian_new_params(1.0)
    new = g.observation_params
    assert new is not old and float(new.n0) == float(old.n0) + 1
    n_ = lambda t: t.cpu().numpy().astype(np.float64)                              # noqa: E731
    K = lambda a, b: n_(g.gp.kernel(torch.as_tensor(a, device=g.device), torch.as_tensor(b, device=g.device)))   # noqa: E731
    args = [n_(y), n_(g.f_star_sm[-1]), n_(old.m_mean), n_(old.m_r_cov), float(old.n0), n_(old.scale)]
    ref = _obs_update_ref(K, n_(x), n_(xo), *args)
    rng = np.random.default_rng(0)
    pert = [a * (1.0 + 1e-15 * rng.standard_normal(a.shape)) if isinstance(a, np.ndarray) else a for a in args]
    ref_p = _obs_update_ref(K, n_(x), n_(xo), *pert)
    on_grid = old.posterior(1, g.y_train[-1], g.f_star_sm[-1])                     # what the shared-grid formula would give
    for name, got, want, want_p, plain in zip(("m_mean", "m_r_cov", "scale"), (new.m_mean, new.m_r_cov, new.scale), ref, ref_p,
                                              (on_grid.m_mean, on_grid.m_r_cov, on_grid.scale)):
        top = np.max(np.abs(want))
        tol = max(1e-9, 50 * np.max(np.abs(want - want_p)) / top)
        err = np.max(np.abs(n_(got) - want)) / top
        print(f"off-grid observation update, {name}: error {err:.2e}, bound {tol:.2e}, shared-grid formula off by {np.max(np.abs(n_(plain) - want)) / top:.2e}")
        assert err <= tol, name
        if name == "scale":                                                        # the projection is what is being tested
            assert np.max(np.abs(n_(plain) - want)) / top > 100 * tol
