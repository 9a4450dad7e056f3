"""Projection of segments of different lengths onto the basis grid in one call (hgp_project_ragged_f64, ops.project_ragged,
IterativeGaussianProcess.project_y, GPI_HDP.project_batch).

Parity is per segment against tests/project_ref.py (the reference's project_y restated; it reproduces the reference's recorded
outputs exactly, tests/test_project_host.py), the error relative to the segment's max |y_p|.  Gates: 1e-10 at length-scale 1.2
(the wave-kernel tier; cond(K~) <= 6e3), 1e-8 at 2.5 and 3.0 (the per-pair tier; cond(K~) ~ 2e7, where the float64 reference itself
sits ~1e-10 from a longdouble solve).  Grids are unit-spaced, as the beats the operator is for: sorted with jitter, reversed,
permuted, shifted by 0.3, and with pairs of points 1e-3 apart; values are smooth beat-like curves, 17 leads of which the calls
with fewer leads take the first.  Everything else is bit for bit at a fixed row stride: a row's result does not depend on the
batch around it, on how the lengths arrive, on the padding or on the number of leads."""
import ctypes

import numpy as np
import pytest
import torch

import project_ref
from conftest import golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

DEV = "cuda"
C_OUT = 300.0
LENS128 = (1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 90, 127, 128)
LENS256 = (129, 144, 200, 255, 256)
KINDS = ("jitter", "reversed", "permuted", "shift", "close")
NLEAD = 17


def gate(ell):
    return 1e-10 if ell < 2.0 else 1e-8


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def same_bits(a, b):
    """Equal as bit patterns (NaN equals the same NaN)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return bool(torch.equal(a, b))


def grid(kind, L, rng):
    base = np.arange(L, dtype=np.float64) + rng.uniform(-0.3, 0.3, L)
    if kind == "jitter":
        return base
    if kind == "reversed":
        return base[::-1].copy()
    if kind == "permuted":
        return rng.permutation(base)
    if kind == "shift":
        return np.arange(L, dtype=np.float64) + 0.3
    x = np.arange(L, dtype=np.float64)             # "close": points 2k and 2k + 1 sit 1e-3 apart
    x[1::2] = x[0:-1:2][:len(x[1::2])] + 1e-3
    return x


def curves(x, span, nlead=NLEAD):
    """[L, nlead]: smooth beat-like values on x (two bumps on a slow wave, another shape per lead)."""
    u = np.asarray(x, dtype=np.float64)[:, None] / max(span, 1.0)
    k = np.arange(nlead, dtype=np.float64)[None, :]
    return (150.0 * np.exp(-0.5 * ((u - 0.40 - 0.01 * k) / 0.06) ** 2) - (40.0 + 3.0 * k) * np.exp(-0.5 * ((u - 0.55) / 0.04) ** 2)
            + (20.0 + k) * np.sin(2.0 * np.pi * u * (1.0 + 0.1 * k)))


def ragged(lens, ld, seed, kinds=KINDS, fill=np.nan):
    """One row per (length, grid kind): X [N, ld], Y [N, ld, NLEAD] padded with `fill`, lengths, and the per-row arrays."""
    rng = np.random.default_rng(seed)
    rows = [(L, kind) for L in lens for kind in kinds]
    X = np.full((len(rows), ld), fill)
    Y = np.full((len(rows), ld, NLEAD), fill)
    xs, ys = [], []
    for n, (L, kind) in enumerate(rows):
        x = grid(kind, L, rng)
        y = curves(x, ld)
        X[n, :L], Y[n, :L] = x, y
        xs.append(x)
        ys.append(y)
    return X, Y, np.array([L for L, _ in rows], dtype=np.int32), xs, ys, rows


_REF = {}


def reference(tag, xs, ys, xb, ell):
    """Per-row restatement results [N, T, NLEAD], computed once per case and shared (read only)."""
    key = (tag, len(xb), ell)
    if key not in _REF:
        out = np.stack([project_ref.project_y_ref(x, y, None, None, xb, C_OUT, ell)[0] for x, y in zip(xs, ys)])
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


def worst_by_kind(got, want, rows):
    worst = {}
    for n, (L, kind) in enumerate(rows):
        e = project_ref.rel_err(got[n], want[n])
        if e >= worst.get(kind, (-1.0, 0))[0]:
            worst[kind] = (e, L)
    return worst


# ------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("ell", [1.2, 2.5, 3.0])
@pytest.mark.parametrize("T", [20, 90, 128])
def test_parity_with_the_restatement_up_to_128(T, ell):
    X, Y, lens, xs, ys, rows = ragged(LENS128, 128, seed=11)
    xb = np.arange(T, dtype=np.float64)
    want = reference("w", xs, ys, xb, ell)
    for D in (1, 2, 3, 17):
        yp, info = ops.project_ragged(dev(X), dev(Y[:, :, :D]), lens, dev(xb), C_OUT, ell)
        assert yp.shape == (len(rows), T, D) and info.dtype == torch.int32 and not bool(info.any())
        worst = worst_by_kind(yp.cpu().numpy(), want[:, :, :D], rows)
        print(f"T {T} ell {ell} D {D}: " + ", ".join(f"{k} {e:.2e} (L {L})" for k, (e, L) in worst.items()))
        for kind, (e, L) in worst.items():
            assert e <= gate(ell), (T, ell, D, kind, L, e)


@pytest.mark.parametrize("ell", [1.2, 3.0])
@pytest.mark.parametrize("T", [150, 256])
def test_parity_with_the_restatement_above_128(T, ell):
    X, Y, lens, xs, ys, rows = ragged(LENS256, 256, seed=12)
    xb = np.arange(T, dtype=np.float64)
    want = reference("c", xs, ys, xb, ell)[:, :, :2]
    yp, info = ops.project_ragged(dev(X), dev(Y[:, :, :2]), lens, dev(xb), C_OUT, ell)
    assert yp.shape == (len(rows), T, 2) and not bool(info.any())
    worst = worst_by_kind(yp.cpu().numpy(), want, rows)
    print(f"T {T} ell {ell} D 2 (ld 256): " + ", ".join(f"{k} {e:.2e} (L {L})" for k, (e, L) in worst.items()))
    for kind, (e, L) in worst.items():
        assert e <= gate(ell), (T, ell, kind, L, e)


# ------------------------------------------------------------------------------------------------------------ bit for bit
BIT_CASES = {"wave": dict(lens=(1, 17, 64, 90, 128), ld=128, T=90), "coop": dict(lens=(129, 200, 256), ld=256, T=150)}


@pytest.fixture(scope="module", params=list(BIT_CASES))
def bits(request):
    c = BIT_CASES[request.param]
    X, Y, lens, xs, ys, rows = ragged(c["lens"], c["ld"], seed=13, kinds=("jitter", "permuted", "close"))
    xb = dev(np.arange(c["T"], dtype=np.float64))
    yp, info = ops.project_ragged(dev(X), dev(Y[:, :, :3]), lens, xb, C_OUT, 3.0)
    assert not bool(info.any())
    return dict(X=X, Y=Y, lens=lens, xs=xs, ys=ys, xb=xb, yp=yp, info=info, T=c["T"], ld=c["ld"])


def test_a_row_alone_and_anywhere_in_a_batch_has_the_same_bits(bits):
    b = bits
    N = len(b["lens"])
    for n in (0, N // 2, N - 1):
        alone, info = ops.project_ragged(dev(b["X"][n:n + 1]), dev(b["Y"][n:n + 1, :, :3]), b["lens"][n:n + 1], b["xb"], C_OUT, 3.0)
        assert same_bits(alone[0], b["yp"][n]) and int(info[0]) == 0
    perm = np.random.default_rng(3).permutation(N)
    yp, _ = ops.project_ragged(dev(b["X"][perm]), dev(b["Y"][perm][:, :, :3]), b["lens"][perm], b["xb"], C_OUT, 3.0)
    assert same_bits(yp, b["yp"][torch.as_tensor(perm, device=DEV)])


def test_host_lengths_device_lengths_and_lists_agree(bits):
    b = bits
    X, Y = dev(b["X"]), dev(b["Y"][:, :, :3])
    yp_d, info_d = ops.project_ragged(X, Y, torch.as_tensor(b["lens"], device=DEV), b["xb"], C_OUT, 3.0)
    assert same_bits(yp_d, b["yp"]) and same_bits(info_d, b["info"])
    Xl, Yl, ll = ops.pad_ragged(b["xs"], [y[:, :3] for y in b["ys"]], DEV)
    assert Xl.shape[1] == b["ld"]
    yp_l, _ = ops.project_ragged(Xl, Yl, ll, b["xb"], C_OUT, 3.0)
    assert same_bits(yp_l, b["yp"])
    full = b["lens"] == b["ld"]                      # lengths=None: every row has ld points
    yp_n, _ = ops.project_ragged(X[full], Y[full], None, b["xb"], C_OUT, 3.0)
    assert int(full.sum()) >= 2 and same_bits(yp_n, b["yp"][torch.as_tensor(full, device=DEV)])
    with pytest.raises(ValueError):
        ops.project_ragged(X, Y, np.where(np.arange(len(b["lens"])) == 1, b["ld"] + 1, b["lens"]), b["xb"], C_OUT, 3.0)
    with pytest.raises(ValueError):
        ops.project_ragged(X, Y, b["lens"][:-1], b["xb"], C_OUT, 3.0)


def test_the_padding_is_never_read(bits):
    b = bits
    for fill in (0.0, 1e300):
        X, Y = np.nan_to_num(b["X"], nan=fill), np.nan_to_num(b["Y"][:, :, :3], nan=fill)
        yp, info = ops.project_ragged(dev(X), dev(Y), b["lens"], b["xb"], C_OUT, 3.0)
        assert same_bits(yp, b["yp"]) and same_bits(info, b["info"])


def test_a_lead_has_the_bits_of_the_one_lead_call(bits):
    b = bits
    X = dev(b["X"])
    yp17, _ = ops.project_ragged(X, dev(b["Y"]), b["lens"], b["xb"], C_OUT, 3.0)
    for d in (0, 2, 15, 16):
        one, _ = ops.project_ragged(X, dev(b["Y"][:, :, d]), b["lens"], b["xb"], C_OUT, 3.0)     # [N, ld] -> [N, T]
        assert one.shape == b["yp"].shape[:2]
        assert same_bits(one, yp17[:, :, d].contiguous())
        if d < 3:
            assert same_bits(one, b["yp"][:, :, d].contiguous())


def test_guard_words_behind_the_outputs_are_untouched(bits):
    b = bits
    N, T, D, ld = len(b["lens"]), b["T"], 3, b["ld"]
    G = 64
    out = torch.full((N * T * D + G,), -7.25, dtype=torch.float64, device=DEV)
    inf = torch.full((N + G,), 77, dtype=torch.int32, device=DEV)
    X, Y, lens = dev(b["X"]), dev(b["Y"][:, :, :3]), torch.as_tensor(b["lens"], device=DEV)
    need = int(_ffi.lib.hgp_project_ragged_ws_bytes(N, ld, T, D))
    ws = torch.full((need // 8 + G,), -7.25, dtype=torch.float64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _ffi.lib.hgp_project_ragged_f64(p(X), p(Y), p(lens), N, ld, D, p(b["xb"]), T, C_OUT, 3.0, 1e-4, p(out), p(inf), p(ws), need,
                                         ops._stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert same_bits(out[:N * T * D].reshape(N, T, D), b["yp"]) and same_bits(inf[:N], b["info"])
    assert bool((out[N * T * D:] == -7.25).all()) and bool((inf[N:] == 77).all()) and bool((ws[need // 8:] == -7.25).all())


# ------------------------------------------------------------------------------------------------------------ special rows
@pytest.mark.parametrize("ld", [128, 256])
def test_on_basis_rows_in_a_mixed_batch_are_copied(ld):
    T = 90 if ld == 128 else 150
    X, Y, lens, xs, ys, rows = ragged((60, T, ld), ld, seed=14, kinds=("jitter", "shift"))
    xb = np.arange(T, dtype=np.float64)
    on = [n for n, (L, kind) in enumerate(rows) if L == T and kind == "jitter"]
    assert len(on) == 1
    n = on[0]
    X[n, :T] = xb                                   # this row sits on the basis; the shifted row of T points does not
    Y[n, :T] = curves(xb, ld) + 1e-3 * np.random.default_rng(5).standard_normal((T, NLEAD))
    yp, info = ops.project_ragged(dev(X), dev(Y[:, :, :3]), lens, dev(xb), C_OUT, 3.0)
    assert not bool(info.any())
    assert same_bits(yp[n], dev(Y[n, :T, :3]))
    for m in range(len(rows)):
        if m != n:
            want = project_ref.project_y_ref(xs[m], ys[m][:, :3], None, None, xb, C_OUT, 3.0)[0]
            assert project_ref.rel_err(yp[m].cpu().numpy(), want) <= gate(3.0)
            assert not same_bits(yp[m], dev(Y[m, :T, :3]))


def test_a_bad_row_is_contained(bits):
    b = bits
    N = len(b["lens"])
    n = N // 2
    X = b["X"].copy()
    X[n, b["lens"][n] // 2] = np.nan                 # inside the row's length
    yp, info = ops.project_ragged(dev(X), dev(b["Y"][:, :, :3]), b["lens"], b["xb"], C_OUT, 3.0)
    assert int(info[n]) > 0 and bool(torch.isnan(yp[n]).all())
    keep = torch.as_tensor(np.arange(N) != n, device=DEV)
    assert same_bits(yp[keep], b["yp"][keep]) and not bool(info[keep].any())
    with pytest.raises(torch.linalg.LinAlgError):
        ops.raise_on_info(info, "project_ragged")
    lens = torch.as_tensor(b["lens"], device=DEV).clone()      # a device length out of range: refused on the device
    lens[n] = b["ld"] + 1
    lens[0] = 0
    yp, info = ops.project_ragged(dev(b["X"]), dev(b["Y"][:, :, :3]), lens, b["xb"], C_OUT, 3.0)
    assert int(info[n]) == -1 and int(info[0]) == -1 and bool(torch.isnan(yp[n]).all()) and bool(torch.isnan(yp[0]).all())
    keep[0] = False
    assert same_bits(yp[keep], b["yp"][keep]) and not bool(info[keep].any())


def test_an_empty_batch():
    yp, info = ops.project_ragged(torch.empty((0, 64), dtype=torch.float64, device=DEV), torch.empty((0, 64, 2), dtype=torch.float64, device=DEV),
                                  None, dev(np.arange(30.0)), C_OUT, 1.2)
    assert yp.shape == (0, 30, 2) and info.shape == (0,)


# ------------------------------------------------------------------------------------------------------------ mirror
def test_mirror_project_y_against_the_recorded_reference():
    from hdpgpc_amd.GPI import IterativeGaussianProcess, RBFWhiteKernel
    g = golden("project_y.npz")
    worst = {}
    for k in range(int(g["n_cases"])):
        p = f"c{k}_"
        c, ell = (float(v) for v in g[p + "theta"])
        xb, x, y, want = g[p + "xb"], g[p + "x"], g[p + "y"], g[p + "yp"]
        T = len(xb)
        C = g[p + "C"] if p + "C" in g.files else np.eye(T)
        gp = IterativeGaussianProcess(RBFWhiteKernel(c, ell, 1.0, device=DEV), xb[:, None])
        Sigma = dev(2.0 * np.eye(T))
        y_p, S_p = gp.project_y(x[:, None], y, None, C, Sigma)
        assert S_p is Sigma and y_p.shape == (T, y.shape[1])
        if np.array_equal(x, xb):
            assert same_bits(y_p, dev(y))            # the short-circuit
            continue
        e = project_ref.rel_err(y_p.cpu().numpy(), want)
        worst[ell] = max(worst.get(ell, 0.0), e)
        assert e <= gate(ell), (k, e)
        # ... and against the mirror's own projection matrix (five launches and a [T, T*] matrix per segment)
        P = gp.projection_matrix(xb[:, None], x[:, None])
        alt = (dev(C) @ P @ dev(y)).cpu().numpy()
        assert project_ref.rel_err(y_p.cpu().numpy(), alt) <= 1e-8, (k,)
    print("mirror project_y vs recorded reference: " + ", ".join(f"ell {k} {v:.2e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------ drop-in
def test_project_batch_feeds_the_training_entry_points():
    from test_gpu_dropin import _driver
    g = golden("reload_r102.npz")
    sw_gp, x_trains, data = _driver(g)
    T, NB = data.shape[1], 24
    assert T == 90
    xb = np.arange(T, dtype=np.float64)
    first = 200                                      # beats the frozen models are rebuilt from; the 24 after them are re-cut
    labels, M = g["labels"][:first], int(g["M"])
    assert np.all(np.bincount(labels, minlength=M) > 0)
    sw_gp.reload_model_from_labels(x_trains[:first], data[:first], labels, M)
    beats = data[first:first + NB]
    xs, ys, lens = [], [], []
    for n in range(NB):
        L = T if n % 3 == 0 else (60 if n % 3 == 1 else 75)
        x = xb if L == T else np.linspace(0.0, T - 1.0, L)
        xs.append(x)
        ys.append(beats[n] if L == T else np.stack([np.interp(x, xb, beats[n, :, d]) for d in range(beats.shape[2])], axis=1))
        lens.append(L)
    x_b, y_b = sw_gp.project_batch(xs, ys)
    D = beats.shape[2]
    assert x_b.shape == (NB, T, 1) and y_b.shape == (NB, T, D) and bool(torch.equal(x_b[:, :, 0], dev(xb).expand(NB, T)))
    ell, worst = float(sw_gp.ini_lengthscale), 0.0
    assert (sw_gp.ini_outputscale_def, ell) == (300.0, 3.0)
    for n in range(NB):
        if lens[n] == T:
            assert same_bits(y_b[n], dev(beats[n]))
        else:
            want = project_ref.project_y_ref(xs[n], ys[n], None, None, xb, 300.0, ell)[0]
            worst = max(worst, project_ref.rel_err(y_b[n].cpu().numpy(), want))
    print(f"project_batch vs restatement: worst {worst:.2e}")
    assert worst <= gate(ell)
    # rectangular input with lengths gives the same bits as the lists
    Xr, Yr, lr = ops.pad_ragged(xs, ys, DEV)
    _, y_r = sw_gp.project_batch(Xr, Yr, lengths=lr)
    assert same_bits(y_r, y_b)
    new_labels = sw_gp.cluster_new_batch(x_b, y_b)
    assert new_labels.shape == (NB,) and bool(((new_labels >= 0) & (new_labels < M)).all())
    with pytest.raises(NotImplementedError):         # the training drivers themselves still want one grid
        sw_gp.cluster_new_batch(Xr, Yr, learning=True, lengths=lr)
    fresh, _, _ = _driver(g)
    fresh.include_batch(x_b, y_b)
    assert bool(torch.isfinite(fresh.q_last).all()) and fresh.q_last.shape[0] == NB
