"""``estimation_limit`` on the HIP kernels: offline chains that cross the limit (chain_batch: the full step up to it, the frozen
step behind it), the online pool with a frozen slot, and both drivers against the reference's own runs with a limit
(tests/golden/make_golden_estlimit.py; the CPU tier replays the same traces in tests/test_estlimit_host.py)."""
import types

import numpy as np
import pytest
import torch

from conftest import golden

import estlimit_trace as et
from offline_trace import compare_trace
from online_trace import compare_online

pytestmark = pytest.mark.gpu

LISTS = ("f_star", "f_star_sm", "cov_f", "cov_f_sm", "A", "Gamma", "C", "Sigma")
INF = float("inf")


def _beats(T, n):
    y90 = golden("mitbih100_lead0.npz")["y"][:n]
    t = np.linspace(0, y90.shape[1] - 1, T)
    return np.stack([np.interp(t, np.arange(y90.shape[1]), r) for r in y90])


def _model(T, E, sigma=9.0, gamma=12.0):
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    m = GPI_model(RBFWhiteKernel(300.0, 3.0, sigma * 1e-5), np.arange(float(T))[:, None], annealing=True, bayesian=True,
                  estimation_limit=None if E == INF else E, free_deg_MNIV=5)
    cond = m.GPR_dynamic(gamma, sigma)
    m.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    m.fixed_theta, m.noise_bounds = (341.0, 1.2, 4.66), (sigma * 1e-5, sigma * 2.0)
    return m


def _copy(m):
    import hdpgpc_amd.GPI_HDP as H
    return H.GPI_HDP.gpmodel_deepcopy(types.SimpleNamespace(verbose=False), m)


def _resp(N, members):
    r = torch.zeros(N)
    r[list(members)] = 1.0
    return r


def _state(m):
    return {k: torch.stack(list(getattr(m, k))).cpu().numpy() for k in LISTS}


def _close(a, b, tol=1e-9):
    return a.shape == b.shape and bool(np.allclose(a, b, rtol=tol, atol=tol * max(float(np.abs(b).max()), 1e-300)))


def _lengths_ok(m):
    n = m.N + 1
    return all(len(getattr(m, k)) == n for k in LISTS[:4]) and all(len(getattr(m, k)) == min(n, m.estimation_limit) for k in LISTS[4:])


# ------------------------------------------------------------------------------------------------------- offline chains
def test_chains_across_the_limit_side_by_side(monkeypatch):
    """Three jobs at T = 20: (a) no limit, 9 members; (b) E = 3 on a fresh model, 9 members: it crosses the limit during the
    run; (c) E = 3 on a model that already has 5 members: frozen from its first step.  Against _full_pass_eager on deep copies:
    every per-step list and both score vectors within 1e-9, list lengths exact; (a) and (b) bit-identical to running them alone.
    No job may take the eager path, and the runs of (b) and (c) replay hipGraphs: side by side the groups here are too short
    for chain_batch to capture anything (it captures a lock-step phase only from 2 UNROLL remaining steps on), so the replays are
    counted on the runs of (b) and (c) alone, which are the same two runs over the same lists."""
    from hdpgpc_amd import chain_batch, member_step
    from hdpgpc_amd.GPI_model import GPI_model
    T, N = 20, 30
    y = _beats(T, N)[:, :, None]
    x = np.repeat(np.arange(float(T))[None, :, None], N, axis=0)
    mem_a, mem_b, pre_c, mem_c = range(0, 27, 3), range(1, 28, 3), (0, 2, 5, 6, 8), range(10, 28, 2)
    assert len(mem_a) == len(mem_b) == len(mem_c) == 9

    def fresh():
        a, b, c = _model(T, INF), _model(T, 3), _model(T, 3)
        c.full_pass_weighted(x, y, _resp(N, pre_c), use_graphs=False)
        assert c.N == 5 and _lengths_ok(c)
        return [a, b, c]

    resps = [_resp(N, mem_a), _resp(N, mem_b), _resp(N, mem_c)]
    ms = fresh()
    eager = [_copy(m) for m in ms]
    assert [e.estimation_limit for e in eager] == [INF, 3, 3]
    ref = [e.full_pass_weighted(x, y, r, use_graphs=False) for e, r in zip(eager, resps)]

    frozen_steps, eager_calls = [], []
    real_step, real_eager = member_step.member_step, GPI_model._full_pass_eager
    monkeypatch.setattr(chain_batch, "member_step", lambda *a, **k: (frozen_steps.append(bool(k.get("frozen"))), real_step(*a, **k))[1])
    monkeypatch.setattr(GPI_model, "_full_pass_eager", lambda self, *a: (eager_calls.append(self), real_eager(self, *a))[1])
    out = chain_batch.run([chain_batch.Job(m, x, y, r) for m, r in zip(ms, resps)])
    assert not eager_calls and True in frozen_steps and False in frozen_steps
    for m, e, (q, ql), (qr, qlr) in zip(ms, eager, out, ref):
        assert m.N == e.N and m.indexes == e.indexes and _lengths_ok(m) and _lengths_ok(e)
        assert float(m.internal_params.n0) == float(e.internal_params.n0)
        sm, se = _state(m), _state(e)
        for k in LISTS:
            print(k, float(np.abs(sm[k] - se[k]).max() / np.abs(se[k]).max()))
            assert _close(sm[k], se[k]), k
        assert _close(q.cpu().numpy(), qr.cpu().numpy()) and _close(ql.cpu().numpy(), qlr.cpu().numpy())
    assert [len(m.A) for m in ms] == [10, 3, 3] and [len(m.f_star) for m in ms] == [10, 10, 15]
    # alone: the same runs as groups of one
    alone = fresh()
    del eager_calls[:]                                   # (fresh() grew model (c) with the eager methods)
    for i, (m, r) in enumerate(zip(alone, resps)):
        q, ql = chain_batch.run([chain_batch.Job(m, x, y, r)])[0]
        if i < 2:
            assert torch.equal(q, out[i][0]) and torch.equal(ql, out[i][1])
            for k in LISTS:
                assert torch.equal(torch.stack(list(getattr(m, k))), torch.stack(list(getattr(ms[i], k)))), (i, k)
        if i > 0:
            assert getattr(m, "graph_replays", 0) > 0
    assert not eager_calls


def test_frozen_lock_step_group_is_captured():
    """Two chains with E = 3 and 22 members each: their frozen runs advance in lock-step for 20 steps, enough for chain_batch to
    capture the frozen step of a group (2 UNROLL remaining steps) and replay it.  Against the eager methods on deep copies."""
    from hdpgpc_amd import chain_batch
    T, N = 20, 30
    y = _beats(T, N)[:, :, None]
    x = np.repeat(np.arange(float(T))[None, :, None], N, axis=0)
    resps = [_resp(N, [i for i in range(N) if i % 4 != 1][:22]), _resp(N, [i for i in range(N) if i % 4 != 2][:22])]
    ms = [_model(T, 3), _model(T, 3)]
    eager = [_copy(m) for m in ms]
    ref = [e.full_pass_weighted(x, y, r, use_graphs=False) for e, r in zip(eager, resps)]
    out = chain_batch.run([chain_batch.Job(m, x, y, r) for m, r in zip(ms, resps)])
    for m, e, (q, ql), (qr, qlr) in zip(ms, eager, out, ref):
        assert m.graph_replays > 0 and m.N == e.N == 22 and _lengths_ok(m) and len(m.A) == 3
        sm, se = _state(m), _state(e)
        for k in LISTS:
            assert _close(sm[k], se[k]), k
        assert _close(q.cpu().numpy(), qr.cpu().numpy()) and _close(ql.cpu().numpy(), qlr.cpu().numpy())


def test_single_chain_t144_across_the_limit():
    """128 < T <= 256 (cooperative inversions, LV_RHS levels; the frozen run has no second one): one chain with E = 3."""
    T, N = 144, 12
    y = _beats(T, N)[:, :, None]
    x = np.repeat(np.arange(float(T))[None, :, None], N, axis=0)
    resp = _resp(N, [i for i in range(N) if i != 4])
    m = _model(T, 3)
    e = _copy(m)
    q, ql = m.full_pass_weighted(x, y, resp)
    qr, qlr = e.full_pass_weighted(x, y, resp, use_graphs=False)
    assert m.graph_replays > 0 and m.N == e.N == 11 and _lengths_ok(m) and len(m.A) == 3
    sm, se = _state(m), _state(e)
    for k in LISTS:
        assert _close(sm[k], se[k]), k
    assert _close(q.cpu().numpy(), qr.cpu().numpy()) and _close(ql.cpu().numpy(), qlr.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------- online pool
def test_pool_keeps_a_frozen_cluster():
    """T = 20, E = 3: eight beats committed to one cluster (it freezes at the second) while a second cluster stays below the
    limit.  Every beat: candidates of both clusters and the commit against the one-by-one path on deep copies (1e-9); the frozen
    cluster stays on the pool; parameter list lengths exact."""
    import hdpgpc.GPI_HDP as hdpgp
    from hdpgpc_amd.online_chain import OnlinePool
    T, E = 20, 3
    Y = _beats(T, 16)
    xb = np.arange(float(T))[:, None]
    std, std_dif = float(np.std(Y, axis=0).mean()), float(np.std(np.diff(Y, axis=0), axis=0).mean())
    sw = hdpgp.GPI_HDP(xb, x_basis_warp=xb[::2], n_outputs=1, ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=std_dif,
                       ini_sigma=std, ini_outputscale=300.0, noise_warp=std * 0.1, bound_sigma=(std * 1e-5, std * 2),
                       bound_gamma=(std_dif * 1e-5, std_dif * 2), bound_noise_warp=(std * 0.01, std * 0.02), verbose=False,
                       max_models=100, bayesian_params=True, estimation_limit=E, free_deg_MNIV=20)
    sw.fixed_theta = (341.0, 1.2, 4.66)
    x = torch.as_tensor(xb, device=sw.device)
    beat = lambda i: torch.as_tensor(Y[i], device=sw.device).reshape(-1, 1)           # noqa: E731
    models, used = [], 0
    for n in (1, 1):
        g = sw.create_gp_default()
        assert g.estimation_limit == E
        for _ in range(n):
            g.include_weighted_sample(used, x, x, beat(used), 1.0)
            g.bayesian_new_params(1.0)
            used += 1
        models.append(g)
    pool = OnlinePool(T, sw.device, sw.annealing_def, cap=4)
    for g in models:
        assert pool.supports(g)
        pool.adopt(g)
    g0 = models[0]
    worst = 0.0
    rel = lambda a, b: float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(np.asarray(b))))       # noqa: E731
    for k in range(8):
        t_new, y = used + k, beat(used + k)
        hist = torch.empty((t_new + 1, 0))
        cols0 = torch.stack([g.compute_q_lat_all(hist) for g in models], dim=1).contiguous()
        pool.begin_beat(y[:, 0], models)
        est, cols, lds = pool.candidates(t_new, cols0)[:3]
        for c, g in enumerate(models):
            cand = sw.gpmodel_deepcopy(g)
            mean_, cov_, C_, Sigma_ = cand.smoother_weighted(x, y, 1.0)
            e_ref = float(cand.log_sq_error(x, y, mean=mean_[-1], cov=cov_[-1], C=C_[-1], Sigma=Sigma_[-1], i=-1, first=len(cand.indexes) == 1))
            cand.include_weighted_sample(t_new, x, x, y, 1.0)
            cand.backwards_pair(1.0)
            cand.bayesian_new_params(1.0)
            col_ref = cand.compute_q_lat_all(hist).cpu().numpy()
            got = cols[:, c].cpu().numpy()
            assert np.array_equal(got == 0, col_ref == 0)
            errs = (abs(float(est[c]) - e_ref) / abs(e_ref), rel(got[col_ref != 0], col_ref[col_ref != 0]),
                    abs(lds[c] - cand.lds_param_likelihood_value()) / abs(cand.lds_param_likelihood_value()))
            worst = max(worst, *errs)
            assert max(errs) <= 1e-9, (k, c, errs)
        twin = sw.gpmodel_deepcopy(g0)
        twin.include_weighted_sample(t_new, x, x, y, 1.0)
        twin.bayesian_new_params(1.0)
        pool.commit(g0, t_new, x, y)
        pool.finish_commit()
        assert pool.holds(g0) and pool.holds(models[1]), f"beat {k}: a cluster fell off the pool"
        assert g0.N == twin.N == k + 2 and g0.indexes == twin.indexes
        assert [len(getattr(g0, n_)) for n_ in LISTS] == [k + 3] * 4 + [min(k + 3, E)] * 4 == [len(getattr(twin, n_)) for n_ in LISTS]
        for n_ in LISTS:
            a, b = torch.stack(list(getattr(g0, n_))).cpu().numpy(), torch.stack(list(getattr(twin, n_))).cpu().numpy()
            worst = max(worst, rel(a, b))
            assert rel(a, b) <= 1e-9, (k, n_)
        assert g0.internal_params.n0 == twin.internal_params.n0
        for a, b in ((g0.internal_params.scale, twin.internal_params.scale), (g0.observation_params.m_mean, twin.observation_params.m_mean)):
            assert rel(a.cpu().numpy(), b.cpu().numpy()) <= 1e-9
        la, lb = g0.compute_q_lat_all(hist).cpu().numpy(), twin.compute_q_lat_all(hist).cpu().numpy()
        assert rel(la[lb != 0], lb[lb != 0]) <= 1e-9
    assert len(models[1].A) == 2 and len(g0.A) == E and len(g0.f_star) == 10
    print(f"pool with a frozen slot: worst relative error {worst:.2e}")


# -------------------------------------------------------------------------------------------------------------- drivers
def test_include_sample_with_limit(monkeypatch):
    """The online step with estimation_limit = 4 against the reference's trace.  Every cluster is adopted by the pool once, at
    the beat after its birth, and never again: a cluster that fell off its chain (the one-by-one path) would be adopted anew."""
    from hdpgpc_amd.online_chain import OnlinePool
    g = golden("include_sample_r102_n40_el4.npz")
    adopted, real = [], OnlinePool.adopt
    monkeypatch.setattr(OnlinePool, "adopt", lambda self, m: (adopted.append(id(m)), real(self, m))[1])

    def each(sw, i):
        assert et.list_lengths_ok(sw), f"beat {i}: list lengths"
        assert i == 0 or sw._pools.get(0) is not None, f"beat {i}: the step left the pool"

    sw, tr = et.run_online(g, each=each)
    worst = compare_online(g, tr, 1e-8)
    assert sum(len(m.indexes) > int(g["estimation_limit"]) for m in sw.gpmodels[0]) >= 2
    assert len(adopted) == len(set(adopted)) and all(id(m) in adopted for m in sw.gpmodels[0] if m.N > 1)
    print(f"include_sample with estimation_limit = 4: worst {worst:.2e}")


def test_include_batch_with_limit_and_readers_behind_it():
    """include_batch with estimation_limit = 6 against the reference's trace, then the readers of steps t >= E on the finished
    model (they take C[-1] / Sigma[-1] there): the KL distance matrix, the bands and draws of every member state."""
    g = golden("include_batch_r102_n100_el6.npz")
    sw, tr = et.run_offline(g)
    worst = compare_trace(g, sw, tr, q_tol=1e-8)
    assert et.list_lengths_ok(sw)
    print(f"include_batch with estimation_limit = 6: {len(tr['order'])} traced calls, worst relative error {worst:.2e}")
    m = max(sw.gpmodels[0], key=lambda m_: len(m_.indexes))
    n = len(m.indexes)
    assert n > m.estimation_limit == 6 and len(m.C) == 6
    ts = list(range(n))
    from hdpgpc_amd.util_plots import kl_distance_matrix
    KL = kl_distance_matrix(sw)
    states = sum(len(m_.f_star) - 1 for m_ in sw.gpmodels[0])
    assert len(KL) == states == 100 and KL.shape == (states, states) and np.all(np.isfinite(KL)) and np.all(KL[~np.eye(states, dtype=bool)] > 0)
    mean, var = m.bands(m.x_basis.reshape(-1)[::2] + 0.5, ts)
    assert mean.shape == var.shape == (n, (m.x_basis.shape[0] + 1) // 2) and bool(torch.isfinite(mean).all()) and bool((var > 0).all())
    draws = m.sample_states(ts, num_samples=2)
    assert draws.shape == (n, 2, m.x_basis.shape[0]) and bool(torch.isfinite(draws).all())
