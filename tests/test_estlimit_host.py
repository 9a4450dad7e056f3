"""CPU tier of ``estimation_limit`` (a cluster stops re-estimating its LDS parameters once it has that many members): the host
logic of both drivers against the reference's own runs with a limit (tests/golden/make_golden_estlimit.py), through
tests/cpu_double.py, and the constructor / bookkeeping around the option.  The same traces run on the GPU in
tests/test_gpu_estlimit.py."""
import pickle

import numpy as np
import pytest
import torch
from scipy.special import digamma

from conftest import golden

import cpu_double
import estlimit_trace as et
from offline_trace import compare_trace
from online_trace import compare_online


def test_include_sample_trace_with_limit_cpu(monkeypatch):
    """The online step with estimation_limit = 4 against the reference's 40-beat run: two clusters grow past the limit, five are
    born after the first one reached it, and the decisions differ from the unlimited run from beat 7 on.  Gate: that of
    test_offline_loop_host.py::test_include_sample_trace_cpu."""
    cpu_double.install(monkeypatch)
    g = golden("include_sample_r102_n40_el4.npz")
    E = int(g["estimation_limit"])

    def each(sw, i):
        assert et.list_lengths_ok(sw), f"beat {i}: list lengths"
        assert all(m.estimation_limit == E for m in sw.gpmodels[0])         # clusters born later get the default limit

    sw, tr = et.run_online(g, each=each)
    compare_online(g, tr, 1e-9)
    assert sum(len(m.indexes) > E for m in sw.gpmodels[0]) >= 2


def test_include_batch_trace_with_limit_cpu(monkeypatch):
    """include_batch with estimation_limit = 6 against the reference's trace: one cluster ends far above the limit, one below.
    Gate: that of test_offline_loop_host.py::test_include_batch_trace_cpu."""
    cpu_double.install(monkeypatch)
    g = golden("include_batch_r102_n100_el6.npz")
    sw, tr = et.run_offline(g)
    compare_trace(g, sw, tr, q_tol=1e-8)
    assert et.list_lengths_ok(sw)
    sizes = [len(m.indexes) for m in sw.gpmodels[0]]
    assert max(sizes) > 6 > min(sizes) > 0


# ------------------------------------------------------------------------------------------ constructor and bookkeeping
T = 20


def _sw(**kw):
    import hdpgpc.GPI_HDP as hdpgp
    xb = np.arange(float(T))[:, None]
    sw = hdpgp.GPI_HDP(xb, ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=12.0, ini_sigma=9.0, ini_outputscale=300.0,
                       bound_sigma=(9e-5, 18.0), bound_gamma=(1e-4, 24.0), verbose=False, free_deg_MNIV=5, **kw)
    sw.fixed_theta = (341.0, 1.2, 4.66)
    return sw, xb


def _batch(N, seed=0):
    rng = np.random.default_rng(seed)
    base = 30.0 * np.sin(np.arange(T) / 3.0)
    return np.stack([base * (1.0 + 0.05 * rng.normal()) + rng.normal(size=T) for _ in range(N)])[:, :, None]


def test_constructor_scalar_list_and_default(monkeypatch):
    cpu_double.install(monkeypatch)
    sw, _ = _sw(M=2, estimation_limit=5)
    assert [m.estimation_limit for m in sw.gpmodels[0]] == [5, 5] and sw.estimation_limit_def == 5
    sw, _ = _sw(M=3, estimation_limit=[3, 7, 9])
    assert [m.estimation_limit for m in sw.gpmodels[0]] == [3, 7, 9] and sw.estimation_limit_def == 3
    assert sw.create_gp_default().estimation_limit == 3 and sw.create_gp_default(i=2).estimation_limit == 3
    sw, _ = _sw(M=2, estimation_limit=np.array([4, 6]))
    assert [m.estimation_limit for m in sw.gpmodels[0]] == [4, 6]
    sw, _ = _sw(M=2)
    assert all(m.estimation_limit == np.inf for m in sw.gpmodels[0]) and sw.estimation_limit_def is None
    assert sw.create_gp_default().estimation_limit == np.inf
    with pytest.raises(ValueError):
        _sw(M=2, estimation_limit=[3, 4, 5])


def test_inducing_points_still_raise(monkeypatch):
    cpu_double.install(monkeypatch)
    with pytest.raises(NotImplementedError, match="inducing"):
        _sw(inducing_points=True)
    with pytest.raises(NotImplementedError, match="inducing"):
        _sw(inducing_points=True, estimation_limit=30)
    _sw(inducing_points=False, estimation_limit=30)


def _lens(m):
    return [len(getattr(m, k)) for k in ("A", "Gamma", "C", "Sigma", "f_star", "f_star_sm", "cov_f", "cov_f_sm")]


def test_copy_pickle_and_keep_last_preserve_a_limited_model(monkeypatch):
    cpu_double.install(monkeypatch)
    E, N = 3, 7
    sw, xb = _sw(M=1, estimation_limit=E)
    y = _batch(N)
    m = sw.gpmodels[0][0]
    m.full_pass_weighted(np.array([xb] * N), y, torch.ones(N))
    assert m.N == N and _lens(m) == [E] * 4 + [N + 1] * 4
    c = sw.gpmodel_deepcopy(m)
    assert c.estimation_limit == E and _lens(c) == _lens(m) and c.N == N
    c.include_weighted_sample(N, xb, xb, y[0], 1.0)                   # the copy goes on as a limited model: nothing is appended
    c.backwards_pair(1.0)
    c.bayesian_new_params(1.0)
    assert _lens(c) == [E] * 4 + [N + 2] * 4 and _lens(m) == [E] * 4 + [N + 1] * 4
    assert c.internal_params is m.internal_params
    back = pickle.loads(pickle.dumps(sw))
    b = back.gpmodels[0][0]
    assert back.estimation_limit_def == E and b.estimation_limit == E and _lens(b) == _lens(m)
    for k in ("A", "Sigma", "f_star_sm"):
        assert all(torch.equal(u, v) for u, v in zip(getattr(b, k), getattr(m, k)))
    assert back.create_gp_default().estimation_limit == E
    sw.keep_last_all()
    assert m.estimation_limit == E and _lens(m) == [1] * 4 + [2] * 4


@pytest.mark.parametrize("E,N", [(4, 12), (30, 12), (None, 12)])
def test_redefine_default_uses_the_limited_window(monkeypatch, E, N):
    """GPI_HDP.py:1870-1874: n_f = min(E_def, N - 1) with a limit, N - 1 without."""
    cpu_double.install(monkeypatch)
    sw, xb = _sw(M=1, estimation_limit=E)
    y = torch.as_tensor(_batch(N, seed=3))
    n_f = N - 1 if E is None else min(E, N - 1)
    a, b = y[:n_f, :10, 0].T, y[1:n_f + 1, :10, 0].T
    var_y = torch.median(torch.sum((a - torch.mean(a, dim=1, keepdim=True)) ** 2, dim=1) / n_f)
    var_d = torch.median(torch.sum((b - a) ** 2, dim=1) / n_f)
    sw.redefine_default(None, y)
    assert sw.ini_sigma_def == pytest.approx(float(var_y) * 0.02, rel=1e-14)
    assert sw.ini_gamma_def == pytest.approx(float(var_d) * 0.025, rel=1e-14)
    assert sw.gpmodels[0][0].estimation_limit == (np.inf if E is None else E)


def test_compute_Pi(monkeypatch):
    cpu_double.install(monkeypatch)
    sw, _ = _sw(M=3, estimation_limit=30)
    sw.transTheta = np.array([[5.0, 1.2, 0.3, 0.1], [0.7, 9.0, 2.0, 0.2], [0.1, 0.4, 3.0, 0.6], [0.2, 0.2, 0.2, 0.2]])
    Pi = sw.compute_Pi()
    dg = digamma(sw.transTheta)
    ref = np.exp(dg - np.log(np.sum(np.exp(dg), axis=1))[:, None])
    assert Pi.shape == (4, 4) and np.allclose(Pi.numpy(), ref, rtol=1e-14, atol=0)
    assert np.all(Pi.numpy().sum(axis=1) <= 1.0 + 1e-14) and np.all(Pi.numpy() > 0)
