"""hdpgpc/hdpgpc/util_plots.py: the result table the drivers print (util_plots.py:269-299).  Figures are presentation and
out of scope: plot_models_plotly is a no-op that says so; plot_MDS / plot_MDS_plotly compute and
return the distance matrix their figure is drawn from (util_plots.py:598-688) and draw nothing."""
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


def plot_models_plotly(*args, save=None, **kwargs):
    """util_plots.py:725-794 draws the clusters with plotly / matplotlib: presentation, not part of this build (SURVEY.md
    section 2, row 12).  Every reference driver ends with this call, so it returns quietly instead of raising."""
    print("plot_models_plotly: figures are not part of the MI355X build" + (f" (nothing written to {save})" if save else ""))
    return None


def kl_distance_matrix(sw_gp, lead=0, smoothed=False):
    """The [sw_gp.T, sw_gp.T] matrix of symmetric Kullback-Leibler distances that plot_MDS / plot_MDS_plotly build
    (util_plots.py:600-616): entry (ind1, ind2) compares the observed Gaussians of the member states that included segments
    ind1 and ind2, over every cluster of `lead`, on the grid sw_gp.x_basis[0].  One device call for all pairs.  Rows and
    columns of segments that belong to no cluster stay zero, the diagonal is zero and the matrix is symmetric."""
    from . import ops

    n_seg = int(sw_gp.T)
    KL = np.zeros((n_seg, n_seg))
    x_bas = sw_gp.x_basis[0]
    models = [gp for gp in sw_gp.gpmodels[lead] if len(gp.indexes) > 0]
    if not models:
        return KL

    def scatter(D, seg1, seg2):
        # the reference fills ind1 < ind2 and mirrors (util_plots.py:612-616)
        ii, jj = np.nonzero(seg1[:, None] < seg2[None, :])
        KL[seg1[ii], seg2[jj]] = D[ii, jj]
        KL[seg2[jj], seg1[ii]] = D[ii, jj]

    segs = [np.asarray([int(i) for i in gp.indexes]) for gp in models]
    rule = {gp._kl_static() for gp in models}
    if len(rule) == 1:
        mom = [gp._kl_moments_on(range(len(gp.indexes)), smoothed, x_bas, latent=rule == {True}) for gp in models]
        D = ops.kl_sym(torch.cat([m for m, _ in mom]).contiguous(), torch.cat([c for _, c in mom]).contiguous())
        seg = np.concatenate(segs)
        scatter(D.cpu().numpy(), seg, seg)
        return KL
    # static and dynamic clusters in one lead: the model that holds the smaller segment index decides what is compared
    # (GPI_model.py:918-921), so the blocks are computed model pair by model pair
    for g1, s1 in zip(models, segs):
        for g2, s2 in zip(models, segs):
            D = g1.kl_states(range(len(s1)), g2, range(len(s2)), smoothed=smoothed, x_bas=x_bas)
            scatter(D.cpu().numpy(), s1, s2)
    return KL


def plot_MDS(sw_gp, main_model, labels, N_0, lead=0, save=None):
    """util_plots.py:598-654 without the MDS embedding and the figure: computes and returns the distance matrix."""
    KL = kl_distance_matrix(sw_gp, lead=lead, smoothed=False)
    print("plot_MDS: figures are not part of the MI355X build" + (f" (nothing written to {save})" if save else ""))
    return KL


def plot_MDS_plotly(sw_gp, main_model, labels, N_0, lead=0, save=None):
    """util_plots.py:656-688 without the MDS embedding and the figure: computes and returns the distance matrix."""
    KL = kl_distance_matrix(sw_gp, lead=lead, smoothed=False)
    print("plot_MDS_plotly: figures are not part of the MI355X build" + (f" (nothing written to {save})" if save else ""))
    return KL
