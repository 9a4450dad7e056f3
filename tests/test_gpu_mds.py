"""a15 on the device: hgp_smacof_steps_f64 through ops.smacof_steps, mds.smacof on top of it and util_plots.mds_embedding.

Gates.  The kernel is compared with tests/mds_ref.py (the NumPy restatement of scikit-learn's _smacof_single that
tests/test_mds_host.py holds against scikit-learn itself) at the project's parity gate: 1e-9 relative to max|X|, the same
relative to the stress, and equal n_iter.  Wherever a count of iterations is compared, the test first asserts on the restatement
that its stop criterion is further from eps than rounding can move it, so that the count cannot flip.  Batch position, batch
size, the split of the passes over calls and the row stride of delta are bit for bit.

The kernel's row tile is 4 rows (one per wave) and its column chunk 256: n = 5 and n = 257 are one more than each.
"""
import types

import numpy as np
import pytest
import torch

import conftest
import kl_ref
import mds_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 1e-9
ROW_TILE, COL_CHUNK = 4, 256
COUNTS = (1, 2, 20, 100)
NOISE = 1e-12     # a stop criterion this close to zero is rounding noise: (S' - S) / N with S, S' equal to ~1e-15 S


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def run(D, X0, n_steps, eps, max_iter, carry=None):
    """ops.smacof_steps from the beginning (or from `carry`, the tuple a previous call returned), n_steps passes in one call.
    D: a device tensor (used as it is) or a host array; X0 [B,n,p].  Returns (X, state, status, stress, n_iter) on the device."""
    from hdpgpc_amd import _ffi, ops
    Dd = D if torch.is_tensor(D) else dev(D)
    if carry is None:
        B = X0.shape[0]
        carry = (dev(X0), torch.zeros((B, _ffi.MDS_STATE_DOUBLES), dtype=torch.float64, device=DEV),
                 torch.zeros(B, dtype=torch.int32, device=DEV), torch.full((B,), -7.0, dtype=torch.float64, device=DEV),
                 torch.full((B,), -7, dtype=torch.int32, device=DEV))
    X, state, status, stress, n_iter = carry
    ops.smacof_steps(Dd, X, state, status, stress, n_iter, n_steps, eps=eps, max_iter=max_iter)
    return carry


def host(carry):
    return tuple(t.cpu().numpy() for t in carry)


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
    conftest._note(err)
    print(f"{what}: err {err:.3e}")
    assert got.shape == ref.shape and np.all(np.isfinite(got)) and err <= GATE, (what, err)


def starts(n, p, B, seed):
    rs = np.random.RandomState(seed)
    return np.stack([rs.uniform(size=n * p).reshape(n, p) for _ in range(B)])


def criteria(D, X0, count):
    """(the restatement's stop criterion of iterations 1 .. count - 1 with no stop rule, {k: (X_k, stress of X_k)} for k in COUNTS)"""
    X, out, crit, old = np.array(X0), {}, [], None
    for it in range(count):
        X = mds_ref.guttman(X, D)
        s, nrm = mds_ref.stress_norm(X, D)
        if old is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                crit.append((old - s) / nrm)
        old = s
        if it + 1 in COUNTS:
            out[it + 1] = (X.copy(), s)
    return np.array(crit), out


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("n", [2, ROW_TILE + 1, 97, COL_CHUNK + 1])
def test_fixed_count_parity(n, p):
    """X and stress after exactly 1, 2, 20 and 100 iterations.  eps = 0 where the restatement's criterion stays clear of zero
    for the whole run; where it does not (n = 2 is exact after one iteration, p = 1 reaches a fixed point in a few), the
    criterion is rounding noise around zero and eps = 0 would let rounding decide the count, so those runs take eps = -1,
    which the C entry accepts and no criterion falls below: the count is max_iter on both sides either way, and asserted."""
    _, D = mds_ref.drifting_groups(n, seed=3)
    X0 = starts(n, p, 1, 10 * n + p)
    crit, ref = criteria(D, X0[0], max(COUNTS))
    for M in COUNTS:
        c = crit[:M - 1]
        assert np.all(np.isfinite(c))
        eps = 0.0 if np.all(c > NOISE) else -1.0
        Xr, sr, nr = mds_ref.smacof_single(D, X0[0], max_iter=M, eps=eps)
        assert nr == M and np.array_equal(Xr, ref[M][0])
        X, _, status, stress, n_iter = host(run(D, X0, M + 1, eps, M))
        assert status[0] == 2 and n_iter[0] == M, (n, p, M, eps, status, n_iter)
        close(X[0], Xr, f"n={n} p={p} M={M} eps={eps} X")
        if sr > 1e-20 * float(np.sum(D ** 2)):          # an exact embedding (n = 2): the stress is rounding, compared with |delta|^2
            close(stress[0], sr, f"n={n} p={p} M={M} eps={eps} stress")
        else:
            assert abs(stress[0] - sr) <= GATE * float(np.sum(D ** 2)) / 2


def stop_case(n, kind, p, seed):
    _, D = mds_ref.drifting_groups(n, seed=3)
    if kind == "sq":
        D = D ** 2 / 2
    return D, starts(n, p, 2, seed)


@pytest.mark.parametrize("n,kind,p", [(97, "euclid", 2), (COL_CHUNK + 1, "sq", 2), (48, "sq", 3)])
def test_stop_rule_parity(n, kind, p):
    eps = 1e-6
    D, X0 = stop_case(n, kind, p, n + p)
    refs = []
    for b in range(2):
        tr = []
        Xr, sr, nr = mds_ref.smacof_single(D, X0[b], max_iter=300, eps=eps, trace=tr)
        assert 2 < nr < 300 and len(tr) == nr - 1
        # the criterion of the stopping iteration and of the one before, clear of eps: rounding cannot flip the count
        assert all(abs(c - eps) > 1e-6 * eps for c in tr[-2:]), tr[-2:]
        assert tr[-1] < eps <= min(tr[:-1])
        refs.append((Xr, sr, nr))
    X, _, status, stress, n_iter = host(run(D, X0, max(r[2] for r in refs) + 3, eps, 300))
    for b, (Xr, sr, nr) in enumerate(refs):
        assert status[b] == 1 and n_iter[b] == nr, (b, status, n_iter, nr)
        close(X[b], Xr, f"n={n} {kind} start {b} X")
        close(stress[b], sr, f"n={n} {kind} start {b} stress")
    # a budget smaller than that count: status 2, n_iter = max_iter
    M = min(r[2] for r in refs) - 5
    assert M >= 2
    X, _, status, stress, n_iter = host(run(D, X0, M + 1, eps, M))
    for b in range(2):
        Xr, sr, nr = mds_ref.smacof_single(D, X0[b], max_iter=M, eps=eps)
        assert nr == M and status[b] == 2 and n_iter[b] == M
        close(X[b], Xr, f"n={n} {kind} start {b} budget X")
        close(stress[b], sr, f"n={n} {kind} start {b} budget stress")


def same(a, b):
    """bit for bit, tuple of device tensors against tuple of device tensors"""
    return all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
               for x, y in zip(a, b))


@pytest.mark.parametrize("n,p", [(97, 2), (COL_CHUNK + 1, 3), (ROW_TILE + 1, 1)])
def test_bitwise_batch_split_and_stride(n, p):
    _, D = mds_ref.drifting_groups(n, seed=3)
    Dd = dev(D)
    X0 = starts(n, p, 4, 1000 + n)
    for eps, max_iter in ((0.0, 300), (1e-3, 300), (1e-6, 12)):   # nobody ends / the starts end at different passes / the budget ends them
        batch = run(Dd, X0, 20, eps, max_iter)
        for b in range(4):
            alone = run(Dd, X0[b:b + 1], 20, eps, max_iter)
            assert same(alone, tuple(t[b:b + 1] for t in batch)), (n, p, eps, b)
        moved = run(Dd, X0[[2, 0, 3, 1, 2]], 20, eps, max_iter)      # other positions, B = 5 (a second group of slots)
        assert same(tuple(t[[2, 0, 3, 1, 2]] for t in batch), moved)
        split = run(Dd, None, 13, eps, max_iter, carry=run(Dd, X0, 7, eps, max_iter))
        assert same(split, batch)
        wide = torch.full((n, n + 3), float("nan"), dtype=torch.float64, device=DEV)   # ld > n; what lies beyond n is never read
        wide[:, :n] = Dd
        assert same(run(wide[:, :n], X0, 20, eps, max_iter), batch)
    assert np.all(host(batch)[2] != 0)


def test_ended_start_is_frozen():
    n = 97
    _, D = mds_ref.drifting_groups(n, seed=3)
    X0 = starts(n, 2, 3, 5)
    c = run(D, X0, 40, 1e-2, 25)
    status = c[2].cpu().numpy()
    assert np.all(status != 0) and np.any(status == 1)
    before = tuple(t.clone() for t in c)
    run(D, None, 9, 1e-2, 25, carry=c)
    assert same(c, before)


def test_zero_rows_and_identical_start_rows():
    """Segments in no cluster (zero rows and columns of delta) and two identical rows of X_0 (d == 0 -> 1e-5 off the diagonal)."""
    n = 41
    _, D = mds_ref.drifting_groups(n, seed=3)
    for s in (0, 7, 8, 40):
        D[s, :] = 0.0
        D[:, s] = 0.0
    X0 = starts(n, 2, 2, 77)
    X0[0, 5] = X0[0, 4]            # delta[4, 5] != 0: ratio delta / 1e-5 times a zero difference
    X0[1, 7] = X0[1, 8]            # delta[7, 8] == 0
    X0[1, 20] = X0[1, 3]
    assert D[4, 5] > 0 and D[7, 8] == 0
    for M in (1, 2, 20):
        X, _, status, stress, n_iter = host(run(D, X0, M + 1, -1.0, M))
        for b in range(2):
            Xr, sr, nr = mds_ref.smacof_single(D, X0[b], max_iter=M, eps=-1.0)
            assert nr == M and status[b] == 2 and n_iter[b] == M
            close(X[b], Xr, f"zero rows, start {b}, M={M} X")
            close(stress[b], sr, f"zero rows, start {b}, M={M} stress")


def test_single_point():
    X, state, status, stress, n_iter = host(run(np.zeros((1, 1)), np.array([[[0.3, 0.7]]]), 4, 1e-6, 3))
    assert status[0] == 2 and n_iter[0] == 3 and stress[0] == 0.0 and np.all(X == 0.0)


def test_non_finite_inputs():
    n = 33
    _, D = mds_ref.drifting_groups(n, seed=3)
    X0 = starts(n, 2, 3, 9)
    bad = D.copy()
    bad[n - 1, 2] = bad[2, n - 1] = np.nan
    X, _, status, stress, n_iter = host(run(bad, X0, 5, 1e-6, 300))
    assert np.all(status == -2) and np.array_equal(X, X0)           # every start fails; X as it was
    Xn = X0.copy()
    Xn[1, 6, 1] = np.nan
    got = run(D, Xn, 5, 1e-6, 300)
    X, _, status, _, _ = host(got)
    assert list(status) == [0, -2, 0]
    assert np.array_equal(X[1], Xn[1], equal_nan=True)              # that start only, X as it was
    for b in (0, 2):
        alone = run(D, X0[b:b + 1], 5, 1e-6, 300)
        assert same(alone, tuple(t[b:b + 1] for t in got))


def test_smacof_best_of_four():
    from hdpgpc_amd import mds
    n, seed, eps = 48, 11, 1e-6
    _, D = mds_ref.drifting_groups(n, seed=3)
    X0 = mds.initial_configurations(n, 2, 4, seed)
    runs = []
    for b in range(4):
        tr = []
        runs.append(mds_ref.smacof_single(D, X0[b], max_iter=300, eps=eps, trace=tr))
        assert runs[-1][2] < 300 and all(abs(c - eps) > 1e-6 * eps for c in tr[-2:])
    Xr, sr, nr, best, _ = mds_ref.smacof(D, X0, max_iter=300, eps=eps)
    order = sorted(r[1] for r in runs)
    assert order[1] - order[0] > GATE * order[0]          # the best start is the best by more than the gate
    X, stress, n_iter, info = mds.smacof(D, n_components=2, n_init=4, max_iter=300, eps=eps, random_state=seed, chunk=16)
    assert info["best"] == best and n_iter == nr
    close(X, Xr, "best X")
    close(stress, sr, "best stress")
    assert list(info["n_iter"]) == [r[2] for r in runs] and list(info["status"]) == [1] * 4
    for b in range(4):
        close(info["X"][b], runs[b][0], f"start {b} X")
    # two equal starts: the first of equals wins
    X2, s2, _, info2 = mds.smacof(dev(D), init=X0[[(best + 1) % 4, best, best]], max_iter=300, eps=eps)
    assert info2["best"] == 1 and info2["stress"][1] == info2["stress"][2] and np.array_equal(X2, info["X"][best]) and s2 == stress
    asym = D.copy()
    asym[3, 9] += 1.0
    with pytest.raises(ValueError):
        mds.smacof(asym, random_state=0)
    with pytest.raises(ValueError):
        mds.smacof(D[:, :-1], random_state=0)
    bad = D.copy()
    bad[1, 2] = bad[2, 1] = np.inf
    with pytest.raises(FloatingPointError):
        mds.smacof(bad, random_state=0)


def _golden_model(c):
    """A GPI_model rebuilt from one cluster's stacks of kl_states.npz (as tests/test_gpu_kl.py builds it)."""
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    gm = GPI_model(RBFWhiteKernel(*[float(v) for v in c["theta"]], device=DEV), c["x_basis"])
    T = len(c["x_basis"])
    gm.load_state(c["f_star"], c["Sigma"], c["C"], c["indexes"], f_star_sm=c["f_star_sm"], cov_f_sm=c["cov_f_sm"],
                  A=np.eye(T)[None], Gamma=c["Gamma_last"][None], cov_f=c["cov_f"])
    return gm


def test_mds_embedding_on_the_golden_model(capsys):
    import hdpgpc.util_plots as up
    from hdpgpc_amd import mds
    from hdpgpc_amd import util_plots as upa
    z = conftest.golden("kl_states.npz")
    gL, gS = _golden_model(kl_ref.cluster(z, "L_")), _golden_model(kl_ref.cluster(z, "S_"))
    n_seg = int(z["n_seg"])
    sw = types.SimpleNamespace(T=n_seg, M=2, gpmodels=[[gL, gS]], x_basis=[z["L_x_basis"]],
                               cond_to_torch=lambda x: torch.as_tensor(x, dtype=torch.float64, device=DEV))
    KL = upa.kl_distance_matrix(sw)
    KLd = upa.kl_distance_matrix_device(sw)
    assert torch.is_tensor(KLd) and KLd.is_cuda and np.array_equal(KLd.cpu().numpy(), KL)
    out = upa.mds_embedding(sw, random_state=4)
    assert set(out) == {"X", "stress", "n_iter", "KL", "cluster", "order"}
    assert np.array_equal(out["KL"], KL)
    X, stress, n_iter, _ = mds.smacof(KL, n_components=2, n_init=4, max_iter=300, eps=1e-6, random_state=4)
    assert out["X"].shape == (n_seg, 2) and np.array_equal(out["X"], X) and out["stress"] == stress and out["n_iter"] == n_iter
    cluster = np.full(n_seg, -1)
    cluster[[int(i) for i in z["L_indexes"]]] = 0
    cluster[[int(i) for i in z["S_indexes"]]] = 1
    assert np.array_equal(out["cluster"], cluster) and out["cluster"][0] == -1 and np.all(KL[0] == 0.0)
    assert np.array_equal(out["order"], np.arange(n_seg))
    # the matrix handed in, host or device, and other parameters
    again = upa.mds_embedding(sw, random_state=4, KL=KLd)
    assert np.array_equal(again["X"], X) and np.array_equal(again["KL"], KL)
    three = upa.mds_embedding(sw, n_components=3, n_init=2, max_iter=30, random_state=1, KL=KL)
    assert three["X"].shape == (n_seg, 3) and three["n_iter"] <= 30
    for fn in (up.plot_MDS, up.plot_MDS_plotly):
        assert np.array_equal(fn(sw, None, None, 0), KL)
    assert "figures are not part of" in capsys.readouterr().out


@pytest.mark.parametrize("p", [1, 2, 3])
def test_direct_call_stays_inside_the_reported_workspace(p):
    """hgp_smacof_steps_f64 on exactly hgp_smacof_ws_bytes(B, n, p) bytes between two guard pads: the pads keep their bits and
    X, state, status, stress and n_iter are the wrapper's, bit for bit."""
    import ws_guard
    from hdpgpc_amd import _ffi, ops
    B, n, n_steps, eps, max_iter = 2, 5, 4, 1e-6, 300
    _, D = mds_ref.drifting_groups(n, seed=3)
    X0, Dd = starts(n, p, B, seed=p), dev(D)
    want = run(Dd, X0, n_steps, eps, max_iter)
    X, state = dev(X0), torch.zeros((B, _ffi.MDS_STATE_DOUBLES), dtype=torch.float64, device=DEV)
    status, n_iter = torch.zeros(B, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    stress = torch.full((B,), -7.0, dtype=torch.float64, device=DEV)
    need = _ffi.lib.hgp_smacof_ws_bytes(B, n, p)
    buf, ws = ws_guard.guarded(need, DEV)
    P = ops._ptr
    assert _ffi.lib.hgp_smacof_steps_f64(P(Dd), n, n, p, B, P(X), eps, n_steps, max_iter, P(state), P(status), P(stress), P(n_iter), ws,
                                         need, ops._stream()) == 0
    torch.cuda.synchronize()
    ws_guard.assert_pads_untouched(buf)
    for got, ref in zip((X, state, status, stress, n_iter), want):
        ws_guard.assert_same_bits(got, ref)
