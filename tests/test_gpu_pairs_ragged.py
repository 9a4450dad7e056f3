"""Ragged pair batches (hgp_loglik_pairs_ragged_f64, PairsPlan.loglik(lengths=...)): segments of different lengths in one call.

The contract is that a length only says where a row ends: row n of a ragged call has, BIT FOR BIT, the outputs of the
rectangular call on the same plan for the one segment x[n, :len], y[n, :len].  Everything else follows from it and is checked on
its own: parity with the oracle per segment (rtol 1e-8, the per-pair gate of tests/test_gpu_parity.py), padding that is never
read (NaN in every test; 0 and 1e300 give the same bits), equivariance under permutations and sub-ranges including the chunk
boundary of the fall-back list, bad lengths, and the layers above (compute_sq_err_all, frozen_scores, cluster_new_batch).

Cases (plan padded size; T, ld; lengths, each at least twice; grids): K = 3 clusters, length-scales 1.2 / 2.0 / 1.2, the third
with an iso-diagonal Sigma, the dense Sigmas from state_t30.npz (leading 20 x 20), state_t90.npz, pairs_ill.npz (T = 128) or,
at T = 200, an SPD draw of synthetic_batch's kind.  Grids: "span" = sorted, the segment's points spread over the basis interval
with jitter; "unit" = sorted and unit-spaced with jitter (the band kernel's pattern at full length); "mixed" = unit grids
permuted (even rows) or compressed to half spacing (odd rows): not block-tridiagonal, through the fall-back list.
The oracle scores every case and every length here (length 1 is a 1 x 1 covariance): none had to be dropped."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, rel_err
from oracle import hdpgpc_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

DEV = "cuda"
RT_PAIR = 1e-8
FB_CAP = 65536                     # PAIRS_FB_CAP of csrc/hgp_internal.hpp: segments per band / generic launch pair
L96 = (1, 16, 17, 45, 80, 81, 89, 90, 95, 96)
L128 = (1, 64, 112, 113, 127, 128)
CASES = {
    "p32": dict(T=20, ld=30, lens=(1, 2, 15, 16, 17, 29, 30), grid="span"),
    "p96_band": dict(T=90, ld=96, lens=L96, grid="unit"),
    "p96_list": dict(T=90, ld=96, lens=L96, grid="mixed"),
    "p128_band": dict(T=128, ld=128, lens=L128, grid="unit"),
    "p128_list": dict(T=128, ld=128, lens=L128, grid="mixed"),
    "p192": dict(T=90, ld=150, lens=(1, 90, 128, 129, 144, 145, 150), grid="span"),
    "p256": dict(T=200, ld=256, lens=(17, 200, 241, 256), grid="span", K=2),
}
NAMES = list(CASES)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def idev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


def same_bits(a, b):
    """Equal as bit patterns (NaN equals the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return bool(torch.equal(a, b))


def grid(kind, L, T, n, rng):
    if kind == "span":
        step = (T - 1.0) / max(L - 1.0, 1.0)
        return (np.arange(L) if L > 1 else np.array([0.37 * T])) * step + rng.uniform(-0.3, 0.3, L) * min(step, 1.0)
    x = np.arange(L, dtype=np.float64) + rng.uniform(-0.3, 0.3, L)
    if kind == "mixed":
        x = rng.permutation(x) if n % 2 == 0 else 0.5 * x
    return x


def dense_sigmas(T, rng):
    if T == 20:
        S = golden("state_t30.npz")["st_Sigma"]
        return [S[-1][:20, :20], S[-2][:20, :20]]
    if T == 90:
        S = golden("state_t90.npz")["st_Sigma"]
        return [S[-1], S[-2]]
    if T == 128:
        S = golden("pairs_ill.npz")["c4_Sigma"]
        return [S[0], S[1]]
    out = []
    for _ in range(2):
        v = rng.normal(size=T)
        out.append(rng.uniform(0.5, 5.0) * (np.eye(T) + 0.1 * np.outer(v, v)))
    return out


def case_host(name):
    """The case's host arrays (NumPy only)."""
    spec = CASES[name]
    T, ld, K = spec["T"], spec["ld"], spec.get("K", 3)
    rng = np.random.default_rng(sum(map(ord, name)))
    lens = np.array(list(spec["lens"]) + list(spec["lens"])[::-1], dtype=np.int32)      # every length twice
    N = lens.size
    sb = orc.synthetic_batch(N, K, T, seed=11 + T)
    xb, mean = sb["xb"], sb["mean"]
    S2 = dense_sigmas(T, rng)
    if K == 3:
        theta = np.array([[341.0, 1.2, 0.9], [358.0, 2.0, 0.9], [375.0, 1.2, 0.9]])
        Sigma = np.stack([S2[0], S2[1], 1.7 * np.eye(T)])
    else:
        theta = np.array([[341.0, 1.2, 0.9], [358.0, 2.0, 0.9]])
        Sigma = np.stack([S2[0], 1.7 * np.eye(T)])
    xs, ys = [], []
    for n, L in enumerate(lens):
        x = grid(spec["grid"], int(L), T, n, rng)
        xs.append(x)
        ys.append(np.interp(x, xb, mean[sb["labels"][n]]) + rng.normal(0.0, 3.0, int(L)))
    X = np.full((N, ld), np.nan)
    Y = np.full((N, ld), np.nan)
    for n, L in enumerate(lens):
        X[n, :L], Y[n, :L] = xs[n], ys[n]
    return dict(name=name, T=T, ld=ld, K=K, N=N, lens=lens, xs=xs, ys=ys, xb=xb, theta=theta, mean=mean, Sigma=Sigma, Xh=X, Yh=Y,
                fn_h=rng.uniform(0.0, 2.0, (N, K)), sel=rng.integers(0, K, N).astype(np.int32))


def oracle_rows(c):
    """[N, K, (score, quad, logdet)] of the oracle, segment by segment on x[n, :len]."""
    return np.array([[orc.log_sq_error_state(c["xs"][n], c["ys"][n], c["xb"], c["mean"][k], c["Sigma"][k], tuple(c["theta"][k]))
                      for k in range(c["K"])] for n in range(c["N"])])


_CASE = {}


def case(name):
    """The case with its NaN-padded device batch and plan (default routing), built once per session and left unchanged."""
    if name not in _CASE:
        c = case_host(name)
        c.update(X=dev(c["Xh"]), Y=dev(c["Yh"]), lens_d=idev(c["lens"]), fn=dev(c["fn_h"]))
        c["plan"] = new_plan(c)
        _CASE[name] = c
    return _CASE[name]


def new_plan(c, acc_tol=1e-9):
    plan = ops.PairsPlan(c["T"], c["ld"], c["theta"], acc_tol=acc_tol).update(dev(c["xb"]), dev(c["mean"]), dev(c["Sigma"]))
    assert int(plan.info.abs().max()) == 0
    return plan


def ragged(plan, c, fn=None, sel=None, X=None, Y=None):
    """(quad, logdet, info, score) of one ragged call each for the quadratic form and for the score output."""
    X, Y = (c["X"] if X is None else X), (c["Y"] if Y is None else Y)
    q, l, i = plan.loglik(X, Y, first_noise=fn, sel=sel, lengths=c["lens_d"])
    s, i2 = plan.score(X, Y, first_noise=fn, sel=sel, lengths=c["lens_d"])
    assert same_bits(i, i2)
    return q, l, i, s


def rows_rectangular(plan, c, fn=None, sel=None):
    """The same four outputs from one rectangular call per segment on x[n, :len], y[n, :len]."""
    out = [[], [], [], []]
    for n, L in enumerate(c["lens"]):
        x, y = c["X"][n:n + 1, :L].contiguous(), c["Y"][n:n + 1, :L].contiguous()
        f = None if fn is None else fn[n:n + 1].contiguous()
        s_ = None if sel is None else sel[n:n + 1]
        q, l, i = plan.loglik(x, y, first_noise=f, sel=s_)
        s, _ = plan.score(x, y, first_noise=f, sel=s_)
        for o, v in zip(out, (q, l, i, s)):
            o.append(v)
    return [torch.cat(o) for o in out]


_DEFAULT = {}


def ragged_default(name):
    if name not in _DEFAULT:
        c = case(name)
        _DEFAULT[name] = ragged(c["plan"], c)
    return _DEFAULT[name]


# ---------------------------------------------------------------------------------------------- 1. same bits as the rectangular call
@pytest.mark.parametrize("mode", ["default", "first_noise", "sel", "explicit", "solve"])
@pytest.mark.parametrize("name", NAMES)
def test_ragged_rows_have_the_bits_of_the_rectangular_call(name, mode):
    c = case(name)
    plan = c["plan"]
    if mode == "explicit":
        plan = new_plan(c, acc_tol=-1.0)
        assert not plan.solve_based().any()
    if mode == "solve":
        plan = new_plan(c, acc_tol=0.0)
        assert plan.solve_based().all()
    fn = c["fn"] if mode == "first_noise" else (c["fn"][torch.arange(c["N"]), torch.as_tensor(c["sel"]).long()].contiguous() if mode == "sel" else None)
    sel = c["sel"] if mode == "sel" else None
    got = ragged_default(name) if mode == "default" else ragged(plan, c, fn, sel)
    ref = rows_rectangular(plan, c, fn, sel)
    for what, g, r in zip(("quad", "logdet", "info", "score"), got, ref):
        assert same_bits(g, r), (name, mode, what)
    assert int(got[2].abs().max()) == 0
    assert bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all() and torch.isfinite(got[3]).all())


# ---------------------------------------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize("name", NAMES)
def test_ragged_against_the_oracle_per_segment(name):
    c = case(name)
    q, l, info, s = (t.cpu().numpy() for t in ragged_default(name))
    assert not info.any()
    ref = oracle_rows(c)
    assert np.isfinite(ref).all()                                               # the oracle scores every length of the case
    errs = [rel_err(s, ref[:, :, 0]), rel_err(q, ref[:, :, 1]), rel_err(l, ref[:, :, 2])]
    print(f"{name}: max rel err vs the oracle: score {errs[0]:.2e} quad {errs[1]:.2e} logdet {errs[2]:.2e}")
    assert max(errs) < RT_PAIR


def test_ragged_ill_conditioned_default_routing_against_the_oracle():
    """ell = 3.0 on T = 90 (pairs_ill.npz, case 3): every cluster goes to the solve-based kernel by the plan's own routing."""
    g = golden("pairs_ill.npz")
    x, y, xb, th, mean, Sig = (g[f"c3_{k}"] for k in ("x", "y", "xb", "theta", "mean", "Sigma"))
    assert float(th[0, 1]) == 3.0
    lens = np.array([1, 17, 45, 89, 90], dtype=np.int32)
    X, Y = x.copy(), y.copy()
    for n, L in enumerate(lens):
        X[n, L:], Y[n, L:] = np.nan, np.nan
    plan = ops.PairsPlan(90, 90, th).update(dev(xb), dev(mean), dev(Sig))
    assert plan.solve_based().all()
    q, l, info = plan.loglik(dev(X), dev(Y), lengths=lens)
    assert int(info.abs().max()) == 0
    ref = np.array([[orc.log_sq_error_state(x[n, :L], y[n, :L], xb, mean[k], Sig[k], tuple(th[k]))[1:] for k in range(3)]
                    for n, L in enumerate(lens)])
    assert np.isfinite(ref).all()
    eq, el = rel_err(q.cpu().numpy(), ref[:, :, 0]), rel_err(l.cpu().numpy(), ref[:, :, 1])
    print(f"ill-conditioned ragged: max rel err quad {eq:.2e} logdet {el:.2e}")
    assert max(eq, el) < RT_PAIR


# ---------------------------------------------------------------------------------------------- 3. padding is never read
@pytest.mark.parametrize("name", NAMES)
def test_padding_is_never_read(name):
    c = case(name)
    ref = ragged_default(name)
    assert np.isnan(c["Xh"][0, c["lens"][0]:]).all() and np.isnan(c["Yh"][0, c["lens"][0]:]).all()      # the default IS NaN padding
    for fill in (0.0, 1e300):
        X, Y = c["Xh"].copy(), c["Yh"].copy()
        X[np.isnan(X)] = fill
        Y[np.isnan(Y)] = fill
        got = ragged(c["plan"], c, X=dev(X), Y=dev(Y))
        for what, g, r in zip(("quad", "logdet", "info", "score"), got, ref):
            assert same_bits(g, r), (name, fill, what)


# ---------------------------------------------------------------------------------------------- 4. equivariance
@pytest.mark.parametrize("name", NAMES)
def test_permutation_and_sub_range(name):
    c = case(name)
    ref = ragged_default(name)
    plan = c["plan"]
    perm = torch.as_tensor(np.random.default_rng(1).permutation(c["N"]), device=DEV)
    q, l, i = plan.loglik(c["X"][perm].contiguous(), c["Y"][perm].contiguous(), lengths=c["lens_d"][perm])
    assert same_bits(q, ref[0][perm]) and same_bits(l, ref[1][perm]) and same_bits(i, ref[2][perm])
    lo, hi = 3, c["N"] - 2
    q, l, i = plan.loglik(c["X"][lo:hi].contiguous(), c["Y"][lo:hi].contiguous(), lengths=c["lens"][lo:hi])      # host lengths
    assert same_bits(q, ref[0][lo:hi]) and same_bits(l, ref[1][lo:hi]) and same_bits(i, ref[2][lo:hi])


def test_more_segments_than_the_fall_back_list_holds():
    """PAIRS_FB_CAP + 5 segments (T = 90, ld = 96, one cluster, sorted unit grids, lengths cycling through the list): the second
    launch pair starts at segment 65 536 and must read ITS lengths; rows on both sides of the boundary against the same rows alone."""
    T, ld, N = 90, 96, FB_CAP + 5
    rng = np.random.default_rng(9)
    sb = orc.synthetic_batch(4, 1, T, seed=2)
    base = 40
    lens_b = np.array([L96[n % len(L96)] for n in range(base)], dtype=np.int32)
    Xb, Yb = np.full((base, ld), np.nan), np.full((base, ld), np.nan)
    for n, L in enumerate(lens_b):
        Xb[n, :L] = np.arange(L) + rng.uniform(-0.3, 0.3, L)
        Yb[n, :L] = np.interp(Xb[n, :L], sb["xb"], sb["mean"][0]) + rng.normal(0.0, 3.0, L)
    reps = N // base + 1
    X, Y, lens = dev(np.tile(Xb, (reps, 1))[:N]), dev(np.tile(Yb, (reps, 1))[:N]), idev(np.tile(lens_b, reps)[:N])
    assert FB_CAP % base != 0                      # the lengths' cycle is out of step with the chunk: an unshifted pointer shows
    plan = ops.PairsPlan(T, ld, sb["theta"][:1]).update(dev(sb["xb"]), dev(sb["mean"][:1]), dev(sb["Sigma"][:1]))
    q, l, i = plan.loglik(X, Y, lengths=lens)
    assert int(i.abs().max()) == 0
    for lo, hi in ((0, 12), (FB_CAP - 7, FB_CAP), (FB_CAP, N), (FB_CAP - 3, FB_CAP + 3)):
        qa, la, ia = plan.loglik(X[lo:hi].contiguous(), Y[lo:hi].contiguous(), lengths=lens[lo:hi].contiguous())
        assert same_bits(qa, q[lo:hi]) and same_bits(la, l[lo:hi]) and same_bits(ia, i[lo:hi]), (lo, hi)
    s, _ = plan.score(X[FB_CAP - 3:].contiguous(), Y[FB_CAP - 3:].contiguous(), lengths=lens[FB_CAP - 3:].contiguous())
    sa, _ = plan.score(X, Y, lengths=lens)
    assert same_bits(sa[FB_CAP - 3:], s)


# ---------------------------------------------------------------------------------------------- 5. bad lengths
def test_host_lengths_out_of_range_raise():
    c = case("p96_band")
    for bad in (0, c["ld"] + 1):
        lens = c["lens"].copy()
        lens[4] = bad
        with pytest.raises(ValueError):
            c["plan"].loglik(c["X"], c["Y"], lengths=lens)
        with pytest.raises(ValueError):
            c["plan"].score(c["X"], c["Y"], lengths=torch.as_tensor(lens))          # a CPU tensor is a host array
    with pytest.raises(ValueError):
        c["plan"].loglik(c["X"], c["Y"], lengths=c["lens"][:-1])


@pytest.mark.parametrize("mode", ["default", "sel", "explicit", "solve"])
@pytest.mark.parametrize("name", ["p32", "p96_band", "p96_list", "p192", "p256"])
def test_device_lengths_out_of_range_give_nan_rows_only(name, mode):
    c = case(name)
    plan = c["plan"] if mode in ("default", "sel") else new_plan(c, acc_tol=-1.0 if mode == "explicit" else 0.0)
    sel = idev(c["sel"]) if mode == "sel" else None
    lens = c["lens"].copy()
    b0, b1 = 2, c["N"] - 3
    lens[b0], lens[b1] = 0, c["ld"] + 1
    good = np.array([n for n in range(c["N"]) if n not in (b0, b1)])
    gd = torch.as_tensor(good, device=DEV)
    q, l, i = plan.loglik(c["X"], c["Y"], sel=sel, lengths=idev(lens))
    s, i2 = plan.score(c["X"], c["Y"], sel=sel, lengths=idev(lens))
    for b in (b0, b1):
        assert bool(torch.isnan(q[b]).all() and torch.isnan(l[b]).all() and torch.isnan(s[b]).all())
        assert bool((i[b] == -1).all() and (i2[b] == -1).all())
    qg, lg, ig = plan.loglik(c["X"][gd].contiguous(), c["Y"][gd].contiguous(), sel=None if sel is None else sel[gd].contiguous(),
                             lengths=idev(lens[good]))
    sg, _ = plan.score(c["X"][gd].contiguous(), c["Y"][gd].contiguous(), sel=None if sel is None else sel[gd].contiguous(),
                       lengths=idev(lens[good]))
    assert same_bits(q[gd], qg) and same_bits(l[gd], lg) and same_bits(i[gd], ig) and same_bits(s[gd], sg)
    assert int(ig.abs().max()) == 0 and bool(torch.isfinite(qg).all())


def test_c_entry_argument_checks_come_before_any_launch():
    c = case("p96_band")
    fn = _ffi.lib.hgp_loglik_pairs_ragged_f64
    x, y, ln = (ctypes.c_void_p(t.data_ptr()) for t in (c["X"], c["Y"], c["lens_d"]))
    out = torch.full((c["N"], c["K"]), 7.0, dtype=torch.float64, device=DEV)
    o = ctypes.c_void_p(out.data_ptr())
    h = c["plan"]._h
    assert fn(h, x, y, c["N"], c["ld"], None, None, None, o, None, None, None) == -1          # seg_len == NULL
    assert fn(h, x, y, c["N"], 0, ln, None, None, o, None, None, None) == -1
    assert fn(h, x, None, c["N"], c["ld"], ln, None, None, o, None, None, None) == -1
    assert fn(h, x, y, c["N"], 97, ln, None, None, o, None, None, None) == -2                 # above the plan's padded size (96)
    assert fn(h, x, y, c["N"], 257, ln, None, None, o, None, None, None) == -2                # above HGP_MAX_T_COOP
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                                                           # nothing was launched


# ---------------------------------------------------------------------------------------------- 6. upper layers
def _model_t90():
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    g = golden("state_t90.npz")
    cc, ell, noise = (float(v) for v in g["st_theta"])
    m = GPI_model(RBFWhiteKernel(cc, ell, noise), g["st_x_basis"][:, None], bayesian=True)
    m.load_state(g["st_f_star"], g["st_Sigma"], g["st_C"], g["st_indexes"], f_star_sm=g["st_f_star_sm"], cov_f_sm=g["st_cov_f_sm"],
                 A=g["st_A"], Gamma=g["st_Gamma"], A_def=g["st_A_def"], Gamma_def=g["st_Gamma_def"], C_def=g["st_C_def"],
                 Sigma_def=g["st_Sigma_def"], n0=float(g["st_n0"]))
    return m, g


def test_compute_sq_err_all_with_lengths():
    m, g = _model_t90()
    y, x = g["y"], g["x_irr"]
    n, T = y.shape
    lens = np.array([60, 64, 71, 77, 80, 85, 89, 90], dtype=np.int32)
    X, Y = x.copy(), y.copy()
    for j, L in enumerate(lens):
        X[j, L:], Y[j, L:] = np.nan, np.nan
    got = m.compute_sq_err_all(X, Y, lengths=lens).cpu().numpy()
    st = orc.ClusterState(g["st_x_basis"], g["st_theta"], list(g["st_f_star"]), list(g["st_Sigma"]), list(g["st_C"]), list(g["st_indexes"]))
    i_vals, first = orc.step_of_segments(st.indexes, n)
    ini = 1e-2 * float(np.mean(np.diag(st.Sigma[0])))
    ref = np.array([orc.log_sq_error_state(x[j, :L], y[j, :L], st.x_basis, *orc.observe_select(st, int(i_vals[j]))[:2], st.theta,
                                           ini if first[j] else 0.0)[0] for j, L in enumerate(lens)])
    assert np.isfinite(ref).all() and rel_err(got, ref) < RT_PAIR
    # lists of per-segment arrays are padded inside: the same bits
    as_list = m.compute_sq_err_all([x[j, :L] for j, L in enumerate(lens)], [y[j, :L] for j, L in enumerate(lens)])
    assert same_bits(as_list, m.compute_sq_err_all(X, Y, lengths=lens))
    # every row at full length: the call without lengths, on irregular grids (general path) and on the basis (shared-grid path)
    full = np.full(n, T, dtype=np.int32)
    assert same_bits(m.compute_sq_err_all(x, y, lengths=full), m.compute_sq_err_all(x, y))
    xs = np.repeat(g["st_x_basis"][None, :], n, 0)
    assert same_bits(m.compute_sq_err_all(xs, y, lengths=idev(full)), m.compute_sq_err_all(xs, y))
    with pytest.raises(ValueError):
        m.compute_sq_err_all(X, Y, lengths=np.array([60, 64, 71, 77, 80, 85, 89, 91]))


def _frozen_r102():
    from test_gpu_dropin import _driver
    g = golden("reload_r102.npz")
    sw, x_trains, data = _driver(g)
    n = 120
    lab = np.searchsorted(np.unique(g["labels"][:n]), g["labels"][:n])
    sw.reload_model_from_labels(x_trains[:n], data[:n], lab, int(lab.max()) + 1)
    return sw, x_trains, data


def test_frozen_scores_and_cluster_new_batch_with_lengths():
    """Beats of record 102 cut to 60 / 75 / 90 points (not beyond the basis length: the per-length plans then share the ragged
    plan's padded size, 96), on the basis' own points or on jittered ones; the full-length beats on the basis take the shared
    covariance as they do today."""
    sw, x_trains, data = _frozen_r102()
    T, N = 90, 24
    rng = np.random.default_rng(4)
    lens = np.array([(60, 75, 90)[n % 3] for n in range(N)], dtype=np.int32)
    x = x_trains[200:200 + N, :, 0].copy()
    y = data[200:200 + N].copy()                                    # [N, 90, 1]
    x[::2] += rng.uniform(-0.3, 0.3, x[::2].shape)                  # every other beat on a grid of its own
    X, Y = x.copy(), y.copy()
    for n, L in enumerate(lens):
        X[n, L:], Y[n, L:] = np.nan, np.nan
    Xd, Yd = sw.cond_to_torch(X), sw.cond_to_torch(Y)
    q = sw.frozen_scores(Xd, Yd, lengths=lens)
    assert q.shape == (N, sw.M, 1) and bool(torch.isfinite(q).all())
    q_ref = torch.empty_like(q)
    for L in np.unique(lens):
        rows = np.nonzero(lens == L)[0]
        q_ref[torch.as_tensor(rows, device=q.device)] = sw.frozen_scores(sw.cond_to_torch(x[rows, :L]), sw.cond_to_torch(y[rows, :L]))
    assert same_bits(q, q_ref)
    assert same_bits(sw.frozen_scores(Xd, Yd, lengths=idev(lens)), q)                        # device lengths
    labels = sw.cluster_new_batch(X, Y, lengths=lens)
    unpatched = sw.frozen_scores
    try:
        sw.frozen_scores = lambda *a, **k: q_ref
        labels_ref = sw.cluster_new_batch(X, Y, lengths=lens)
    finally:
        sw.frozen_scores = unpatched
    assert labels.shape == (N,) and torch.equal(labels, labels_ref)
    # lists of per-segment arrays
    xl, yl = [x[n, :L] for n, L in enumerate(lens)], [y[n, :L] for n, L in enumerate(lens)]
    assert same_bits(sw.frozen_scores(xl, yl), q)
    assert torch.equal(sw.cluster_new_batch(xl, yl), labels)
    with pytest.raises(ValueError):
        sw.frozen_scores(Xd, Yd, lengths=np.where(np.arange(N) == 5, 91, lens))
    with pytest.raises(NotImplementedError):
        sw.cluster_new_batch(X, Y, learning=True, lengths=lens)


def test_two_leads_with_snr_refuse_ragged_input():
    from test_gpu_dropin import _driver
    sw, x_trains, data = _driver(golden("reload_r102_2leads.npz"))
    assert sw.n_outputs == 2 and sw.use_snr
    lens = np.array([80, 90, 70], dtype=np.int32)
    with pytest.raises(NotImplementedError):
        sw.cluster_new_batch(x_trains[:3, :, 0], data[:3], lengths=lens)
    with pytest.raises(NotImplementedError):
        sw.cluster_new_batch([x_trains[n, :L, 0] for n, L in enumerate(lens)], [data[n, :L] for n, L in enumerate(lens)])


def test_emission_scores_passes_the_lengths_on():
    from hdpgpc_amd import batch
    c = case("p96_list")
    q = batch.emission_scores(c["plan"], c["X"], c["Y"], lengths=c["lens_d"])
    assert same_bits(q, ragged_default("p96_list")[3])


def test_pad_ragged_on_the_device():
    c = case("p32")
    X, Y, lens = ops.pad_ragged(c["xs"], c["ys"], device=DEV)
    assert X.is_cuda and same_bits(X, c["X"]) and same_bits(Y, c["Y"]) and same_bits(lens, c["lens_d"])
