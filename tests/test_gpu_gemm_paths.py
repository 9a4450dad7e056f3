"""The batched tile GEMM (hgp_gemm.hip) and the list GEMM (hgp_chain.hip, which kept it when the inverses moved to hgp_inverse.hip) on the paths the product's shapes never take: the
one-wave-per-32x32-block kernel k_gemm22, batches beyond one grid (chunks of 65535), beta != 0 reading C, operands with
lda > cols and batch strides larger than a matrix (or zero), both transposes at once, every side of the dispatch's Kd boundaries,
and each launch form of ops.GemmList on its own.

Reference: np.longdouble products.  Every comparison is element-wise against the bound that holds for ANY order of summation
(the standard gamma_K bound, Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):
    |C - ref| <= (Kd + 4) eps (|alpha| (|op A| |op B|) + |beta| |D|)
(Kd products and Kd - 1 sums of the dot product, the product with alpha, the product with beta, the sum of the two, one to
spare).  float64 NumPy is held to the same bound on the same inputs before the device is; where a large batch is compared with
float64 NumPy instead, both sides are within the bound of the exact result, so they are within twice the bound of each other.
Operands and results are views inside NaN-filled parents: a kernel that reads padding returns NaN, one that writes outside the
M x N views leaves a number where a NaN was.
"""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import conftest

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


class Padded:
    """[batch, rows, cols] numbers with leading dimension ld > cols and batch stride > rows * ld inside a NaN parent (stride 0: one
    matrix shared by the batch)."""

    def __init__(self, rng, batch, rows, cols, ld_extra=3, stride_extra=5, shared=False, fill=True):
        self.ld = cols + ld_extra
        self.n = 1 if shared else batch
        self.step = rows * self.ld + stride_extra
        self.stride = 0 if shared else self.step
        self.lead = 7
        self.parent = np.full(self.lead + self.n * self.step + 4, np.nan)
        self.mask = np.zeros(self.parent.size, dtype=bool)
        strides = (self.step * 8, self.ld * 8, 8)
        self.v = np.lib.stride_tricks.as_strided(self.parent[self.lead:], shape=(self.n, rows, cols), strides=strides)
        np.lib.stride_tricks.as_strided(self.mask[self.lead:], shape=(self.n, rows, cols), strides=(self.step, self.ld, 1))[...] = True
        if fill:
            self.v[...] = rng.normal(size=self.v.shape)
        self.dev = None

    def up(self):
        self.dev = torch.from_numpy(self.parent).cuda()
        return self

    @property
    def ptr(self):
        return ctypes.c_void_p(self.dev.data_ptr() + 8 * self.lead)

    def down(self):
        """(the views [batch, rows, cols] of the device parent, True if the parent is still NaN everywhere outside them)."""
        torch.cuda.synchronize()
        p = self.dev.cpu().numpy()
        v = np.lib.stride_tricks.as_strided(p[self.lead:], shape=self.v.shape, strides=self.v.strides).copy()
        return v, bool(np.isnan(p[~self.mask]).all())


def op(X, t):
    return X.transpose(0, 2, 1) if t else X


def reference(A, B, tA, tB, alpha, beta=0.0, D=None, items=None, dtype=LD):
    """(alpha op(A) op(B) + beta D, the bound) for the items `items` of the batch (operands with one matrix are shared)."""
    batch = max(A.shape[0], B.shape[0], 1 if D is None else D.shape[0])
    items = range(batch) if items is None else items
    pick = lambda X: np.stack([X[i if X.shape[0] > 1 else 0] for i in items])      # noqa: E731
    a, b = op(pick(A), tA), op(pick(B), tB)
    Kd = a.shape[2]
    ref = alpha * np.matmul(a.astype(dtype), b.astype(dtype))
    mag = abs(alpha) * np.matmul(np.abs(a), np.abs(b))
    if D is not None and beta != 0.0:
        d = pick(D)
        ref = ref + beta * d.astype(dtype)
        mag = mag + abs(beta) * np.abs(d)
    return ref, (Kd + 4) * EPS * mag


def ratio(C, ref, bound, what):
    """max |C - ref| / bound, noted like the other parity figures; C must be finite."""
    assert np.isfinite(C).all(), f"{what}: non-finite result (padding read?)"
    r = float(np.max(np.abs(C.astype(LD) - ref) / np.maximum(bound, 1e-300)))
    conftest._note(r)
    return r


def check(C, A, B, tA, tB, alpha, beta=0.0, D=None, items=None, what=""):
    """C (the device's items `items`) against longdouble within the bound - and float64 NumPy within the same bound first."""
    ref, bound = reference(A, B, tA, tB, alpha, beta, D, items)
    f64, _ = reference(A, B, tA, tB, alpha, beta, D, items, dtype=np.float64)
    assert ratio(f64, ref, bound, what + " (NumPy float64)") <= 1.0
    r = ratio(C, ref, bound, what)
    assert r <= 1.0, f"{what}: {r:.3f} x the bound"
    return r


def gemm(tA, tB, M, N, Kd, alpha, A, B, C, batch, beta=0.0, D=None):
    st = ops._stream()
    if D is None:
        rc = _ffi.lib.hgp_gemm_batched_f64(int(tA), int(tB), M, N, Kd, alpha, A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, beta,
                                           C.ptr, C.ld, C.stride, batch, st)
    else:
        rc = _ffi.lib.hgp_gemm_add_batched_f64(int(tA), int(tB), M, N, Kd, alpha, A.ptr, A.ld, A.stride, B.ptr, B.ld, B.stride, beta,
                                               D.ptr, D.ld, D.stride, C.ptr, C.ld, C.stride, batch, st)
    assert rc == 0


# ---------------------------------------------------------------------------------------------------- shapes and layout
KDS = [1, 3, 4, 5, 32, 33, 96, 97, 128, 129, 130]          # every side of the dispatch's Kd <= 32 / <= 96 / <= 128 boundaries
_MN = list(itertools.product([1, 15, 16, 17, 33], [1, 16, 17]))
SHAPES = [_MN[(4 * j + t) % len(_MN)] + (kd,) for j, kd in enumerate(KDS) for t in range(4)]     # 44 of the 165, every M, N, Kd


def run_layout_case(M, N, Kd, tA, tB, variant):
    rng = np.random.default_rng(1000 * M + 100 * N + Kd + 7 * tA + 13 * tB)
    batch, alpha = 3, -0.75
    A = Padded(rng, batch, *((Kd, M) if tA else (M, Kd)), shared=variant == "strideA0").up()
    B = Padded(rng, batch, *((N, Kd) if tB else (Kd, N)), shared=variant == "strideB0").up()
    C = Padded(rng, batch, M, N, ld_extra=5, fill=False).up()
    D, beta = None, 0.0
    if variant == "add":
        D, beta = Padded(rng, batch, M, N, ld_extra=1).up(), 1.5
    gemm(tA, tB, M, N, Kd, alpha, A, B, C, batch, beta=beta, D=D)
    got, clean = C.down()
    what = f"{M}x{N}x{Kd} tA={int(tA)} tB={int(tB)} {variant}"
    r = check(got, A.v, B.v, tA, tB, alpha, beta, None if D is None else D.v, what=what)
    assert clean, f"{what}: written outside the M x N views"
    return r


@pytest.mark.parametrize("M,N,Kd", SHAPES)
def test_gemm_padded_operands_all_transposes(M, N, Kd):
    """batch 3, ld = cols + 3 and a batch stride larger than the matrix for A and B, ldc = N + 5 for C, all inside NaN parents: the
    masked tail of every tile neither reads padding nor writes outside M x N."""
    assert set(KDS) == {s[2] for s in SHAPES} and len(SHAPES) == 44
    worst = max(run_layout_case(M, N, Kd, tA, tB, "plain") for tA in (False, True) for tB in (False, True))
    print(f"gemm {M}x{N}x{Kd}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("Kd", KDS)
@pytest.mark.parametrize("variant", ["strideA0", "strideB0", "add"])
def test_gemm_shared_operands_and_addend(Kd, variant):
    """One row of the shapes (M, N = 33, 17, every Kd) with A shared by the batch (strideA = 0), with B shared, and through
    hgp_gemm_add_batched_f64 with the addend at ldd = N + 1."""
    worst = max(run_layout_case(33, 17, Kd, tA, tB, variant) for tA in (False, True) for tB in (False, True))
    print(f"gemm 33x17x{Kd} {variant}: worst error / bound = {worst:.3f}")


# --------------------------------------------------------------------------------------------------------------- k_gemm22
def test_gemm22_block_kernel_and_its_threshold():
    """M = N = 64, Kd = 160, no transposes: 4 blocks of 32 x 32 per item, so a batch of 512 is 2048 blocks - the first that takes
    k_gemm22 - and a batch of 511 still takes k_gemm.  A shared by the batch; B and C per item."""
    rng = np.random.default_rng(22)
    M = N = 64
    Kd, batch, alpha = 160, 512, 1.25
    sub = [0, 1, 255, 510, 511]                          # the longdouble subset; every item against float64 NumPy
    A = Padded(rng, batch, M, Kd, shared=True).up()
    B = Padded(rng, batch, Kd, N).up()
    f64 = alpha * np.matmul(A.v, B.v)
    _, bound = reference(A.v, B.v, False, False, alpha, dtype=np.float64)

    def run(n, beta=0.0, D=None, prefill=None):
        C = Padded(rng, batch, M, N, ld_extra=5, fill=False)
        if prefill is not None:
            C.v[...] = prefill
        gemm(False, False, M, N, Kd, alpha, A, B, C.up(), n, beta=beta, D=D)
        got, clean = C.down()
        assert clean
        return got

    c512 = run(512)
    check(c512[sub], A.v, B.v, False, False, alpha, items=sub, what="k_gemm22 batch 512")
    assert np.all(np.abs(c512 - f64) <= 2 * bound)
    conftest._note(float(np.max(np.abs(c512 - f64) / (2 * bound))))
    c511 = run(511)
    sub511 = [i for i in sub if i < 511]
    check(c511[sub511], A.v, B.v, False, False, alpha, items=sub511, what="k_gemm batch 511")
    assert np.isnan(c511[511]).all()                                       # the item behind the batch: not touched
    assert np.all(np.abs(c511[:511] - c512[:511]) <= 2 * bound[:511])      # both kernels within the bound of the exact product
    # the addend D shared by the batch (stride 0), beta = 2
    D = Padded(rng, batch, M, N, ld_extra=1, shared=True).up()
    cadd = run(512, beta=2.0, D=D)
    check(cadd[sub], A.v, B.v, False, False, alpha, 2.0, D.v, items=sub, what="k_gemm22 + 2 D")
    full = f64 + 2.0 * D.v
    assert np.all(np.abs(cadd - full) <= 2 * (bound + (Kd + 4) * EPS * 2.0 * np.abs(D.v)))
    # beta = -0.5 reading C itself (hgp_gemm_batched_f64 accumulating into a pre-filled C)
    C0 = rng.normal(size=(batch, M, N))
    cacc = run(512, beta=-0.5, prefill=C0)
    check(cacc[sub], A.v, B.v, False, False, alpha, -0.5, C0, items=sub, what="k_gemm22 - 0.5 C")
    assert np.all(np.abs(cacc - (f64 - 0.5 * C0)) <= 2 * (bound + (Kd + 4) * EPS * 0.5 * np.abs(C0)))


# ---------------------------------------------------------------------------------------------------------- batch chunking
def test_gemm_batch_beyond_one_grid():
    """batch = 65535 + 3: two launches, the second starting at item 65535 (boff).  Every item against float64 NumPy, the first,
    the last and the items around the chunk boundary against longdouble."""
    rng = np.random.default_rng(65535)
    M, N, Kd, batch, alpha = 3, 2, 5, 65535 + 3, 0.5
    A, B = Padded(rng, batch, M, Kd).up(), Padded(rng, batch, Kd, N).up()
    C = Padded(rng, batch, M, N, ld_extra=5, fill=False).up()
    gemm(False, False, M, N, Kd, alpha, A, B, C, batch)
    got, clean = C.down()
    assert clean
    sub = [0, 32768, 65534, 65535, 65536, batch - 1]
    check(got[sub], A.v, B.v, False, False, alpha, items=sub, what="chunked batch")
    _, bound = reference(A.v, B.v, False, False, alpha, dtype=np.float64)
    f64 = alpha * np.matmul(A.v, B.v)
    assert np.isfinite(got).all() and np.all(np.abs(got - f64) <= 2 * bound)


# --------------------------------------------------------------------------------------------------------------- GEMM list
def _nan_view(rows, cols, pad=3):
    """A [rows, cols] view with row stride cols + pad (cols = None: a contiguous vector) inside a NaN-filled device parent."""
    if cols is None:
        parent = torch.full((rows + 9,), np.nan, dtype=torch.float64, device="cuda")
        return parent, parent[4:4 + rows]
    ld = cols + pad
    parent = torch.full((5 + rows * ld + 6,), np.nan, dtype=torch.float64, device="cuda")
    return parent, parent[5:5 + rows * ld].view(rows, ld)[:, :cols]


def _filled(rng, rows, cols):
    parent, v = _nan_view(rows, cols)
    h = rng.normal(size=(rows,) if cols is None else (rows, cols))
    v.copy_(torch.from_numpy(h))
    return v, h


class ListCase:
    """One item of a GemmList with padded operands and outputs, and what it must compute."""

    def __init__(self, gl, rng, M, N, K, tA, tB, alpha, beta, with_D, eye, with_out2):
        vec = N == 1
        self.A, a = _filled(rng, *((K, M) if tA else (M, K)))
        if vec:                                                    # vectors are 1-D (read as columns)
            self.B, b = _filled(rng, K, None)
            b = b[None, :] if tB else b[:, None]
        else:
            self.B, b = _filled(rng, *((N, K) if tB else (K, N)))
        self.D, d = _filled(rng, M, None if vec else N) if with_D else (None, None)
        self.outs = [_nan_view(M, None if vec else N, pad=4) for _ in range(2 if with_out2 else 1)]
        gl.add(self.A, self.B, self.outs[0][1], D=self.D, transA=tA, transB=tB, alpha=alpha, beta=beta, add_eye=eye,
               out2=self.outs[1][1] if with_out2 else None)
        a, b = (a.T if tA else a), (b.T if tB else b)
        self.ref = alpha * (a.astype(LD) @ b.astype(LD))
        mag = abs(alpha) * (np.abs(a) @ np.abs(b))
        if with_D:
            self.ref = self.ref + beta * d.reshape(M, N).astype(LD)
            mag = mag + abs(beta) * np.abs(d.reshape(M, N))
        if eye:
            self.ref = self.ref + eye * np.eye(M, dtype=LD)
            mag = mag + abs(eye) * np.eye(M)
        self.bound = (K + 4) * EPS * mag
        self.what = f"list item {M}x{N}x{K} tA={int(tA)} tB={int(tB)}"

    def clear(self):
        for parent, _ in self.outs:
            parent.fill_(np.nan)

    def check(self, ran):
        """ran: the launch covered this item - outputs within the bound, both copies the same bits, nothing outside the views;
        otherwise everything is still NaN."""
        got = []
        for parent, v in self.outs:
            g = v.cpu().numpy().reshape(self.ref.shape)
            if not ran:
                assert torch.isnan(parent).all(), f"{self.what}: written by a launch that does not cover it"
                continue
            assert ratio(g, self.ref, self.bound, self.what) <= 1.0, self.what
            assert int(torch.isnan(parent).sum()) == parent.numel() - v.numel(), f"{self.what}: written outside its view"
            got.append(g)
        assert len(got) < 2 or np.array_equal(got[0], got[1])


def _list_cases(gl, rng):
    spec = [  # M, N, K, tA, tB, alpha, beta, D, add_eye, out2
        (17, 33, 5, False, False, 1.0, 1.0, False, 0.0, False),
        (33, 33, 97, True, False, -1.0, 2.0, True, 1.0, True),
        (16, 16, 16, False, True, 0.5, -1.0, True, 0.0, False),
        (45, 1, 45, False, False, 1.0, 1.0, True, 0.0, True),
        (90, 90, 130, True, True, 1.0, 1.0, False, -0.25, False),
        (1, 7, 100, False, True, 2.0, 1.0, True, 0.0, False),
    ]
    return [ListCase(gl, rng, *s) for s in spec]


def _launch_and_check(cases, launch, covered):
    for c in cases:
        c.clear()
    launch()
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        c.check(i in covered)


def test_gemm_list_launch_forms_with_padded_items():
    """Operands, addend and both outputs of every item with stride(0) > shape[1] inside NaN parents; each launch form starts from
    NaN outputs and is checked on its own: the mapped launch, its replay, a walked sub-range, a mapped prefix."""
    gl = ops.GemmList("cuda")
    cases = _list_cases(gl, np.random.default_rng(31))
    n = len(cases)
    _launch_and_check(cases, gl.run, range(n))
    _launch_and_check(cases, gl.run, range(n))                                  # replay
    _launch_and_check(cases, lambda: gl.run_range(2, 3), range(2, 5))           # walked, un-mapped (hgp_gemm_list_f64)
    _launch_and_check(cases, lambda: gl.run_range(0, 2), range(0, 2))           # prefix of the tile map
    assert gl._map is not None


def test_gemm_list_of_one_item_walks():
    """A one-item list has no tile map: run() and run_range() both go through hgp_gemm_list_f64."""
    gl = ops.GemmList("cuda")
    case = [ListCase(gl, np.random.default_rng(33), 33, 33, 97, True, False, -1.0, 2.0, True, 1.0, True)]
    assert gl.finalize()._map is None
    _launch_and_check(case, gl.run, [0])
    _launch_and_check(case, lambda: gl.run_range(0, 1), [0])
