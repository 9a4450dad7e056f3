"""Static cluster models (model_type='static') through every layer on the GPU: GPI_model.full_pass_weighted on the reference's
recorded chain (the fused filter chain against the eager methods and against tests/golden/chain_static_t30.npz), the replay of the
reference's static include_batch trace, the reload / classify / learn sequence with a mixed type list, and the consumers of a
trained static model (pickle, bands, draws, distance matrix).  Fixtures: tests/golden/make_golden_static.py.  The dynamic fixtures
are not run again here: the suite's own tests are the proof that nothing existing moved."""
import pickle

import numpy as np
import pytest
import torch

import static_trace
from conftest import golden, rel_err, relclose
from offline_trace import compare_trace, traced

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def chain_model(g):
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    m = GPI_model(RBFWhiteKernel(300.0, 3.0, float(g["noise_bounds"][0])), g["x_basis"][:, None], annealing=True, bayesian=True, free_deg_MNIV=5)
    cond = m.GPR_static(float(g["sigma"]))
    m.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    m.fixed_theta = tuple(float(v) for v in g["theta"])          # what the (out-of-scope) gpytorch fit left behind
    return m


def lists(m):
    out = {name: torch.stack(list(getattr(m, name))).cpu().numpy()[:, :, 0] for name in ("f_star", "f_star_sm")}
    out.update({name: torch.stack(list(getattr(m, name))).cpu().numpy() for name in ("cov_f", "cov_f_sm")})
    return out


def test_full_pass_weighted_reproduces_the_recorded_chain_fused_and_eager():
    g = golden("chain_static_t30.npz")
    y = g["y"]
    n, T = y.shape
    xs = np.repeat(g["x_basis"][None, :, None], n, axis=0)
    res = {}
    for fused in (True, False):
        m = chain_model(g)
        q, q_lat = m.full_pass_weighted(xs, y[:, :, None], np.ones(n), use_graphs=fused)
        assert getattr(m, "static_chain_calls", 0) == (1 if fused else 0)          # the route that was meant ran
        assert m.indexes == list(g["indexes"]) and m.N == n
        assert [len(getattr(m, k)) for k in ("A", "Gamma", "C", "Sigma")] == [1] * 4
        assert len(m.x_train) == len(m.y_train) == n
        assert not bool(torch.any(q_lat != 0)) and q_lat.shape == (n,)
        got = lists(m)
        for name, v in got.items():
            assert v.shape == g[name].shape and relclose(v, g[name], 1e-9), (fused, name)
        assert rel_err(q.cpu().numpy(), g["q"]) < 1e-9, fused
        for name, ref in (("A", "A0"), ("C", "C0"), ("Sigma", "Sigma0"), ("Gamma", "Gamma0")):
            assert np.array_equal(getattr(m, name)[0].cpu().numpy(), g[ref]), name
        res[fused] = (got, q.cpu().numpy())
    for name in res[True][0]:
        assert relclose(res[True][0][name], res[False][0][name], 1e-9), name
    assert rel_err(res[True][1], res[False][1]) < 1e-9


def test_fused_chain_continues_a_model_and_batches_chains_of_different_lengths():
    """Two passes over disjoint members = one pass over all of them (bit for bit: the same kernel, the same states), and
    chains of different lengths in one chain_batch.run = each alone."""
    from hdpgpc_amd import chain_batch
    g = golden("chain_static_t30.npz")
    y = g["y"]
    n, T = y.shape
    xs = np.repeat(g["x_basis"][None, :, None], n, axis=0)
    one = chain_model(g)
    one.full_pass_weighted(xs, y[:, :, None], np.ones(n))
    two = chain_model(g)
    r1, r2 = np.zeros(n), np.zeros(n)
    r1[:5], r2[5:] = 1.0, 1.0
    two.full_pass_weighted(xs, y[:, :, None], r1)
    two.full_pass_weighted(xs, y[:, :, None], r2)
    assert two.indexes == one.indexes and two.static_chain_calls == 2
    for name in ("f_star", "cov_f", "f_star_sm", "cov_f_sm"):
        assert torch.equal(torch.stack(list(getattr(one, name))), torch.stack(list(getattr(two, name)))), name
    ms = [chain_model(g) for _ in range(3)]
    resps = [r1, np.ones(n), r2]
    outs = chain_batch.run([chain_batch.Job(m, xs, y[:, :, None], r) for m, r in zip(ms, resps)])
    for m, r, out in zip(ms, resps, outs):
        alone = chain_model(g)
        q, _ = alone.full_pass_weighted(xs, y[:, :, None], r)
        assert torch.equal(out[0], q) and torch.equal(torch.stack(list(m.cov_f)), torch.stack(list(alone.cov_f)))


def test_include_batch_static_trace():
    """The reference's static include_batch on the first 60 beats of record 102, decision for decision: call sequence and every
    assignment identical, every number at 1e-9 (the record-102 trace gate); no event is skipped."""
    g = golden("include_batch_r102_n60_static.npz")
    sw, tr = static_trace.run_offline(g)
    assert len(tr["order"]) == len(g["order"]) == 359
    compare_trace(g, sw, tr, q_tol=1e-9)
    assert sw.M == 6 and [len(m.indexes) for m in sw.gpmodels[0]] == [28, 20, 6, 3, 2, 1]
    assert static_trace.static_lists_ok(sw)
    assert all(not e[2].any() for e in tr["em"])                         # Q_lat identically zero
    assert sum(getattr(m, "static_chain_calls", 0) for m in sw.gpmodels[0]) > 0
    # the consumers of a trained static model
    from hdpgpc_amd import util_plots
    T = len(g["x_basis"])
    back = pickle.loads(pickle.dumps(sw))
    assert back.model_type_def == 'static' and static_trace.static_lists_ok(back)
    for a, b in zip(sw.gpmodels[0], back.gpmodels[0]):
        assert a.indexes == b.indexes and torch.equal(a.f_star_sm[-1], b.f_star_sm[-1]) and torch.equal(a.Sigma[-1], b.Sigma[-1])
    bands = util_plots.model_bands(back)
    assert sorted(bands) == list(range(6))
    for d in bands.values():
        assert d["mean"].shape == d["var"].shape == d["x"].shape and np.isfinite(d["mean"]).all() and (d["var"] > 0).all()
        assert d["mean_latent"].shape == (T,) and not d["noise_latent"].any()          # Gamma = 0: no latent band
    draws = util_plots.model_samples(back, num_samples=4)
    assert draws["x_basis"].shape == (T,)
    assert all(np.isfinite(v).all() for k, v in draws.items() if isinstance(v, np.ndarray))
    KL = util_plots.kl_distance_matrix(back)
    assert KL.shape == (60, 60) and np.isfinite(KL).all() and (KL >= 0).all() and not np.diag(KL).any()
    ev = util_plots.model_evolution(back, 2)
    assert ev["mean"].shape[0] == len(back.gpmodels[0][2].indexes) and np.isfinite(ev["mean"]).all()          # one row per member step
    util_plots.print_results(back, np.zeros(60, dtype=np.int64), 0)
    back.keep_last_all()                                                 # first and last state; the member indexes stay
    for m in back.gpmodels[0]:
        assert [len(getattr(m, k)) for k in ("A", "Gamma", "C", "Sigma", "f_star", "f_star_sm", "cov_f", "cov_f_sm")] == [1] * 4 + [2] * 4
        assert not bool(torch.any(m.Gamma[-1] != 0))


def test_reload_classify_and_learn_with_a_mixed_type_list():
    """reload_model_from_labels, cluster_new_batch(learning=False) and cluster_new_batch(learning=True) with model_type
    alternating 'static', 'dynamic', ... over the label classes, against the reference's run: labels identical, q at 1e-7 (the
    gate of the reload tests).  As in the reference, the reload builds every class model from the default type - the first entry -
    so every cluster is static afterwards (the fixture records that)."""
    g = golden("reload_r102_n100_static_mixed.npz")
    data = np.asarray(g["y"], dtype=np.float64)
    n0, M0 = int(g["n0"]), int(g["M0"])
    types = [str(t) for t in g["model_type"]]
    sw, xb = static_trace.driver(g, data.shape[2], types, M=M0)
    assert [not bool(torch.any(m.Gamma[-1] != 0)) for m in sw.gpmodels[0]] == [t == 'static' for t in types]
    x_trains = np.array([xb] * data.shape[0])
    sw.reload_model_from_labels(x_trains[:n0], data[:n0], g["labels"], M0)
    assert [not bool(torch.any(m.Gamma[-1] != 0)) for m in sw.gpmodels[0]] == list(g["gamma_zero_after_reload"])
    assert relclose(sw.q[-1].cpu().numpy(), g["q_reload"], 1e-7)
    labels = sw.cluster_new_batch(x_trains[n0:], data[n0:], learning=False)
    assert np.array_equal(np.asarray(labels, dtype=np.int64), g["labels_frozen"])
    tr = traced(sw, lambda: sw.cluster_new_batch(x_trains[n0:], data[n0:], learning=True))
    compare_trace(g, sw, tr, q_tol=1e-7)          # with M, the cluster sizes, the last assignment, the bound and the last q matrices
