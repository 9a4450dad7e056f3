"""hdpgpc/hdpgpc/util_plots.py: the result table the drivers print (util_plots.py:269-299).  Figures are presentation and
out of scope: every plot_* function computes and returns what its figure is drawn from and draws
nothing - plot_models / plot_models_plotly / plot_partial_models the cluster templates with their predictive bands on the
plotting grid (model_bands, model_evolution: one device call for all states, util_plots.py:335-476,755-772), plot_MDS /
plot_MDS_plotly the distance matrix (util_plots.py:598-688); mds_embedding adds the MDS embedding of that matrix (mds.smacof)."""
import numpy as np
import torch


def print_results(sw_gp, labels, N_0, error=False, purity=False):
    """Per cluster: histogram of the annotation labels of its members and the majority label; then the number of members
    whose label differs from their cluster's majority ("classification error")."""
    models = sw_gp.gpmodels[0]
    main_model = ["None"] * len(models)
    for i, gp in enumerate(models):
        vals, counts = np.unique([labels[j + N_0] for j in gp.indexes], return_counts=True)
        hist = "[" + ",".join(f"{v}-{c}" for v, c in zip(vals, counts)) + "]"
        mm = ""
        if len(counts) > 0:
            main_model[i] = vals[np.argmax(counts)]
            mm = ": MainModel: " + str(main_model[i])
        print('Model', (i + 1), mm, ':', hist)
    err = np.zeros(len(models))
    for m, gp in enumerate(models):
        err[m] = sum(1 for i in gp.indexes if labels[i + N_0] != main_model[m])
        if purity:
            print('Model', (m + 1), ': Purity: ', 1 - err[m] / len(gp.indexes))
    tot = int(err.sum())
    print(f"Classification error: {tot} / {sw_gp.T} -- {(tot / sw_gp.T):.5f}")
    if purity:
        print(f"Classification purity: {sw_gp.T - tot}/{sw_gp.T} -- {(1 - err.sum() / sw_gp.T):.5f}")
        return main_model, tot, sw_gp.T - tot
    if error:
        return main_model, tot
    return main_model


def _plot_grid(gp, step):
    """torch.arange(min(x_b), max(x_b), step) of util_plots.py:755-756, on the host."""
    x_b = gp.x_basis.reshape(-1).cpu()
    return x_b, torch.arange(float(x_b.min()), float(x_b.max()), step, dtype=torch.float64)


def model_bands(sw_gp, selected_gpmodels=None, lead=0, step=0.1, width=1.9):
    """What plot_models_plotly / plot_models draw for every selected cluster (util_plots.py:755-772), from ONE device call
    for all of them: per cluster a dict with `x` = arange(min x_b, max x_b, step), `mean` and `var` of observe_last on it,
    `lower` / `upper` = mean -/+ width sqrt(var), and the latent band on the basis grid: `x_basis`, `mean_latent` =
    f_star_sm[-1], `noise_latent` = width sqrt(diag Gamma[-1]).  Returns {cluster index: dict}, numpy arrays on the host."""
    from . import ops

    models = sw_gp.gpmodels[lead]
    sel = list(range(len(models))) if selected_gpmodels is None else [int(m) for m in selected_gpmodels]
    out = {}
    if not sel:
        return out
    gps = [models[m] for m in sel]
    grids = [_plot_grid(gp, step) for gp in gps]
    shared = all(g[0].shape == grids[0][0].shape and torch.equal(g[0], grids[0][0]) for g in grids)
    if shared and grids[0][1].numel() > 0:
        g0 = gps[0]
        dev = g0.device
        T = g0.x_basis.shape[0]
        theta = ops.to_dev(np.asarray([gp.gp.kernel.params() for gp in gps], dtype=np.float64), torch.float64, dev)
        mean = torch.cat([ops.gemm_batched(gp.C[-1], gp.f_star_sm[-1]).reshape(1, T) for gp in gps]).contiguous()
        Sig = torch.stack([gp.Sigma[-1] for gp in gps]).contiguous()
        mq, vq, _ = ops.pred_bands(g0.x_basis.reshape(-1).contiguous(), theta, mean, Sig, grids[0][1].to(dev), check=True)
        res = [(mq[i], vq[i]) for i in range(len(gps))]
    else:   # clusters on different basis grids: one call each
        res = [tuple(v[0] for v in gp.bands(g[1])) for gp, g in zip(gps, grids)]
    for m, gp, (x_b, x_), (mq, vq) in zip(sel, gps, grids, res):
        mean, var = mq.cpu().numpy(), vq.cpu().numpy()
        sd = np.sqrt(var)
        out[m] = {"x": x_.numpy(), "mean": mean, "var": var, "lower": mean - width * sd, "upper": mean + width * sd,
                  "x_basis": x_b.numpy(), "mean_latent": gp.f_star_sm[-1].reshape(-1).cpu().numpy(),
                  "noise_latent": width * np.sqrt(np.diag(gp.Gamma[-1].cpu().numpy()))}
    return out


def model_samples(sw_gp, selected_gpmodels=None, lead=0, num_samples=10, random_state=0):
    """Curves drawn from every selected cluster of a lead (default sw_gp.selected_gpmodels(), or all of them where the driver
    has no such method), each from its last smoothed state as observed - GPI_model.sample_last for all clusters from ONE
    device call (ops.sample_states), with the same normals for every cluster.  Returns a dict of host arrays: `x_basis` [T],
    `clusters` (their indices), `mean` [K,T] = C f_star_sm of the last state, `samples` [K,n,T].  Clusters on basis grids of
    different lengths go in one call per length; `x_basis`, `mean` and `samples` are then lists with one entry per cluster.
    Same distribution as the reference's sample_last, not the same numbers (IterativeGaussianProcess.sample_y)."""
    from . import ops

    models = sw_gp.gpmodels[lead]
    if selected_gpmodels is None:
        selected_gpmodels = sw_gp.selected_gpmodels() if hasattr(sw_gp, "selected_gpmodels") else range(len(models))
    sel = [int(m) for m in selected_gpmodels]
    gps = [models[m] for m in sel]
    n = int(num_samples)
    mean, samples = [None] * len(gps), [None] * len(gps)
    by_T = {}
    for k, gp in enumerate(gps):
        by_T.setdefault(int(gp.x_basis.shape[0]), []).append(k)
    for T, ks in by_T.items():
        g0 = gps[ks[0]]
        C = torch.stack([gps[k].C[-1] for k in ks]).contiguous()
        P = torch.stack([gps[k].cov_f_sm[-1] for k in ks]).contiguous()
        f = torch.stack([gps[k].f_star_sm[-1].reshape(T, 1) for k in ks]).contiguous()
        Sig = torch.stack([gps[k].Sigma[-1] for k in ks]).contiguous()
        mu = ops.gemm_batched(C, f).reshape(len(ks), T)
        cov = ops.gemm_batched(ops.gemm_batched(C, P), C, transB=True, add=Sig)
        out, _ = ops.sample_states(mu, cov, g0.gp.standard_normals([n, T], random_state))
        mu, out = mu.cpu().numpy(), out.cpu().numpy()
        for i, k in enumerate(ks):
            mean[k], samples[k] = mu[i], out[i]
    xb = [gp.x_basis.reshape(-1).cpu().numpy() for gp in gps]
    res = {"x_basis": xb, "clusters": np.asarray(sel, dtype=np.int64), "mean": mean, "samples": samples}
    if len(by_T) == 1:
        res.update(x_basis=xb[0], mean=np.stack(mean), samples=np.stack(samples))
    elif not gps:
        res.update(x_basis=np.zeros(0), mean=np.zeros((0, 0)), samples=np.zeros((0, n, 0)))
    return res


def model_evolution(sw_gp, m, lead=0, step=0.1, ts=None):
    """The bands of one cluster at every member step (ts=None: all of them) - observe(x, t) of plot_partial_models
    (util_plots.py:451-476) for the whole history in one device call.  Returns a dict: `x`, `mean` and `var` [n_steps, Q],
    `ts` and `indexes` (the member segment of each step)."""
    gp = sw_gp.gpmodels[lead][m]
    ts = list(range(len(gp.indexes))) if ts is None else [int(t) for t in ts]
    _, x_ = _plot_grid(gp, step)
    mq, vq = gp.bands(x_, ts)
    return {"x": x_.numpy(), "mean": mq.cpu().numpy(), "var": vq.cpu().numpy(), "ts": np.asarray(ts, dtype=np.int64),
            "indexes": np.asarray([gp.indexes[t] if 0 <= t < len(gp.indexes) else -1 for t in ts], dtype=np.int64)}


def _no_figure(name, save):
    print(f"{name}: figures are not part of the MI355X build" + (f" (nothing written to {save})" if save else ""))


def plot_models_plotly(sw_gp, selected_gpmodels, main_model=None, labels=None, N_0=0, save=None, lead=0, step=0.1,
                       plot_latent=False, ticks=False):
    """util_plots.py:725-794 without the figure: computes and returns what it is drawn from (model_bands)."""
    data = model_bands(sw_gp, selected_gpmodels, lead=lead, step=step)
    _no_figure("plot_models_plotly", save)
    return data


def plot_models(sw_gp, selected_gpmodels, main_model=None, labels=None, N_0=0, save=None, lead=0, step=0.1, plot_latent=False):
    """util_plots.py:301-419 without the figure: computes and returns what it is drawn from (model_bands)."""
    data = model_bands(sw_gp, selected_gpmodels, lead=lead, step=step)
    _no_figure("plot_models", save)
    return data


def plot_partial_models(sw_gp, selected_gpmodels, main_model=None, labels=None, N_0=0, time_instant=(-1,), save=None):
    """util_plots.py:421-520 without the figure: for every selected cluster the bands of observe(x, t) at the steps of
    `time_instant` (model_evolution on the reference's 0.1 grid).  Returns {cluster index: dict}."""
    data = {int(m): model_evolution(sw_gp, int(m), ts=list(time_instant)) for m in selected_gpmodels}
    _no_figure("plot_partial_models", save)
    return data


def _kl_blocks(sw_gp, lead, smoothed):
    """The blocks kl_distance_matrix places: (D on the device, segment index of each row, of each column), one device call each."""
    from . import ops

    x_bas = sw_gp.x_basis[0]
    models = [gp for gp in sw_gp.gpmodels[lead] if len(gp.indexes) > 0]
    if not models:
        return
    segs = [np.asarray([int(i) for i in gp.indexes]) for gp in models]
    rule = {gp._kl_static() for gp in models}
    if len(rule) == 1:
        mom = [gp._kl_moments_on(range(len(gp.indexes)), smoothed, x_bas, latent=rule == {True}) for gp in models]
        D = ops.kl_sym(torch.cat([m for m, _ in mom]).contiguous(), torch.cat([c for _, c in mom]).contiguous())
        seg = np.concatenate(segs)
        yield D, seg, seg
        return
    # static and dynamic clusters in one lead: the model that holds the smaller segment index decides what is compared
    # (GPI_model.py:918-921), so the blocks are computed model pair by model pair
    for g1, s1 in zip(models, segs):
        for g2, s2 in zip(models, segs):
            yield g1.kl_states(range(len(s1)), g2, range(len(s2)), smoothed=smoothed, x_bas=x_bas), s1, s2


def kl_distance_matrix(sw_gp, lead=0, smoothed=False):
    """The [sw_gp.T, sw_gp.T] matrix of symmetric Kullback-Leibler distances that plot_MDS / plot_MDS_plotly build
    (util_plots.py:600-616): entry (ind1, ind2) compares the observed Gaussians of the member states that included segments
    ind1 and ind2, over every cluster of `lead`, on the grid sw_gp.x_basis[0].  One device call for all pairs.  Rows and
    columns of segments that belong to no cluster stay zero, the diagonal is zero and the matrix is symmetric."""
    n_seg = int(sw_gp.T)
    KL = np.zeros((n_seg, n_seg))
    for D, seg1, seg2 in _kl_blocks(sw_gp, lead, smoothed):
        # the reference fills ind1 < ind2 and mirrors (util_plots.py:612-616)
        D = D.cpu().numpy()
        ii, jj = np.nonzero(seg1[:, None] < seg2[None, :])
        KL[seg1[ii], seg2[jj]] = D[ii, jj]
        KL[seg2[jj], seg1[ii]] = D[ii, jj]
    return KL


def kl_distance_matrix_device(sw_gp, lead=0, smoothed=False, device=None):
    """kl_distance_matrix, the same values, placed on the device and left there (an fp64 tensor): the matrix never crosses to
    the host.  `device` is only needed when no cluster of the lead has a member (default cuda:0)."""
    n_seg = int(sw_gp.T)
    KL = None
    for D, seg1, seg2 in _kl_blocks(sw_gp, lead, smoothed):
        if KL is None:
            KL = torch.zeros((n_seg, n_seg), dtype=torch.float64, device=D.device)
        ii, jj = np.nonzero(seg1[:, None] < seg2[None, :])
        if ii.size == 0:
            continue
        a, b = (torch.as_tensor(v, dtype=torch.int64, device=D.device) for v in (seg1[ii], seg2[jj]))
        vals = D[torch.as_tensor(ii, device=D.device), torch.as_tensor(jj, device=D.device)]
        KL[a, b] = vals
        KL[b, a] = vals
    if KL is None:
        KL = torch.zeros((n_seg, n_seg), dtype=torch.float64, device=device or "cuda:0")
    return KL


def mds_embedding(sw_gp, lead=0, smoothed=False, n_components=2, n_init=4, max_iter=300, eps=1e-6, random_state=None, KL=None):
    """The compute part of plot_MDS / plot_MDS_plotly (util_plots.py:600-620): the distance matrix of kl_distance_matrix (or
    `KL`, a host array or a device tensor) and its embedding MDS(dissimilarity='precomputed').fit_transform by mds.smacof; the
    matrix goes from the one device call to the other without crossing to the host.  Returns a dict of host arrays: `X`
    [sw_gp.T, n_components], `stress`, `n_iter` (of the best of n_init starts), `KL`, `cluster` [sw_gp.T] = the cluster of
    `lead` that holds each segment (-1: none) and `order` = the segment indices in time order, the line the figure draws
    through the points (util_plots.py:649-654)."""
    from . import mds

    n_seg = int(sw_gp.T)
    if KL is None:
        KL = kl_distance_matrix_device(sw_gp, lead=lead, smoothed=smoothed)
    X, stress, n_iter, _ = mds.smacof(KL, n_components=n_components, n_init=n_init, max_iter=max_iter, eps=eps, random_state=random_state)
    cluster = np.full(n_seg, -1, dtype=np.int64)
    for m, gp in enumerate(sw_gp.gpmodels[lead]):
        for i in gp.indexes:
            cluster[int(i)] = m
    return {"X": X, "stress": stress, "n_iter": n_iter, "KL": KL.cpu().numpy() if torch.is_tensor(KL) else np.asarray(KL, dtype=np.float64),
            "cluster": cluster, "order": np.arange(n_seg, dtype=np.int64)}


def plot_MDS(sw_gp, main_model, labels, N_0, lead=0, save=None):
    """util_plots.py:598-654 without the figure: computes and returns the distance matrix (mds_embedding: the embedding too)."""
    KL = kl_distance_matrix(sw_gp, lead=lead, smoothed=False)
    print("plot_MDS: figures are not part of the MI355X build (mds_embedding computes the embedding)" + (f" (nothing written to {save})" if save else ""))
    return KL


def plot_MDS_plotly(sw_gp, main_model, labels, N_0, lead=0, save=None):
    """util_plots.py:656-688 without the figure: computes and returns the distance matrix (mds_embedding: the embedding too)."""
    KL = kl_distance_matrix(sw_gp, lead=lead, smoothed=False)
    print("plot_MDS_plotly: figures are not part of the MI355X build (mds_embedding computes the embedding)" + (f" (nothing written to {save})" if save else ""))
    return KL
