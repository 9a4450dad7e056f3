"""CPU-side checks of the MDS embedding (hdpgpc_amd/mds.py, include/hdpgpc_hip_mds.h): the NumPy restatement the kernel is
compared with (tests/mds_ref.py) against scikit-learn's public smacof and seeded MDS, the start configurations against
scikit-learn's draws, and the C entry's argument validation, which happens before any HIP call.

Gate: the project's parity gate, 1e-9 relative to max|X| (and relative to the stress), and equal n_iter.  Inputs are separated
points (mds_ref.drifting_groups): scikit-learn forms distances in the expanded form, which loses digits where embedded points
nearly coincide, so parity with scikit-learn is asserted on such inputs only and only through the restatement."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import mds_ref

sk_mds = pytest.importorskip("sklearn.manifold")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
MDS_HEADER = os.path.join(ROOT, "include", "hdpgpc_hip_mds.h")
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
GATE = 1e-9

i32, f64, vp, sz = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
PINNED = {"hgp_smacof_ws_bytes": (sz, [i32, i32, i32]),
          "hgp_smacof_steps_f64": (i32, [vp, i32, i32, i32, i32, vp, f64, i32, i32, vp, vp, vp, vp, vp, sz, vp])}
# hgp_smacof_ws_bytes(B, n, p) as the header's workspace macro gave it (doubles, times 8) before the library reported its
# workspace itself: a caller that sized its buffer by the macro stays correct
WS_BYTES = {(4, 97, 3): 15520, (1, 1, 1): 24}


def inputs(n, kind):
    _, D = mds_ref.drifting_groups(n, seed=3)     # a seed at which scikit-learn's stress still falls at iteration 100 (asserted below)
    if kind == "sq":
        D = D ** 2 / 2          # not a metric: the triangle inequality fails
    X0 = np.random.RandomState(n).uniform(size=n * 2).reshape(n, 2)
    return D, X0


def close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print(f"{what}: {err:.3e}")
    assert got.shape == ref.shape and err <= GATE, (what, err)


@pytest.mark.parametrize("n", [48, 97])
@pytest.mark.parametrize("kind", ["euclid", "sq"])
def test_restatement_matches_sklearn_smacof(n, kind):
    D, X0 = inputs(n, kind)
    for max_iter, eps in ((1, 0.0), (20, 0.0), (100, 0.0), (300, 1e-6)):
        Xs, ss, ns = sk_mds.smacof(D, init=X0.copy(), n_init=1, max_iter=max_iter, eps=eps, normalized_stress=False, return_n_iter=True)
        if eps == 0.0:
            assert ns == max_iter          # both sides ran the same count
        Xr, sr, nr = mds_ref.smacof_single(D, X0, max_iter=max_iter, eps=eps)
        assert nr == ns, (max_iter, eps, nr, ns)
        close(Xr, Xs, f"n={n} {kind} max_iter={max_iter} eps={eps} X")
        close(sr, ss, f"n={n} {kind} max_iter={max_iter} eps={eps} stress")


@pytest.mark.parametrize("seed", [0, 7])
def test_starts_and_seeded_mds_parity(seed):
    from hdpgpc_amd import mds
    n = 48
    _, D = mds_ref.drifting_groups(n, seed=3)
    starts = mds.initial_configurations(n, 2, 4, seed)
    assert starts.shape == (4, n, 2)
    rs = np.random.RandomState(seed)
    assert np.array_equal(starts, np.stack([rs.uniform(size=n * 2).reshape(n, 2) for _ in range(4)]))
    assert np.array_equal(mds.initial_configurations(n, 2, 4, np.random.RandomState(seed)), starts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = sk_mds.MDS(n_components=2, dissimilarity="precomputed", n_init=4, max_iter=300, eps=1e-6, random_state=seed,
                       normalized_stress=False)
        emb = m.fit_transform(D)
    X, stress, n_iter, best, runs = mds_ref.smacof(D, starts, max_iter=300, eps=1e-6)
    assert n_iter == m.n_iter_
    close(X, emb, "embedding_")
    close(stress, m.stress_, "stress_")
    assert all(r[1] >= stress for r in runs)


def test_mds_header_parses_to_the_pinned_binding():
    from hdpgpc_amd import _cheader
    with open(MDS_HEADER) as f:
        funcs, structs, defines = _cheader.parse_header(f.read())
    assert funcs == PINNED and structs == {} and defines == {"HGP_MDS_STATE_DOUBLES": 8}


@needs_lib
def test_mds_table_is_separate_from_the_main_headers():
    from hdpgpc_amd import _cheader, _ffi, ops
    assert _ffi.MDS_EXPORTS == sorted(PINNED) and _ffi.MDS_STATE_DOUBLES == 8
    assert not set(PINNED) & set(_ffi.EXPORTS) and not set(PINNED) & set(_ffi.FIT_EXPORTS)
    with open(os.path.join(ROOT, "include", "hdpgpc_hip.h")) as f:
        assert _ffi.EXPORTS == sorted(_cheader.parse_header(f.read())[0])
    for name, sig in PINNED.items():
        fn = getattr(_ffi.lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name
    assert ops.smacof_ws_doubles(4, 97, 3) == 4 * 97 * 5


@needs_lib
def test_workspace_bytes_are_pinned():
    from hdpgpc_amd import _ffi, ops
    size_fn = _ffi.lib.hgp_smacof_ws_bytes
    assert {shape: size_fn(*shape) for shape in WS_BYTES} == WS_BYTES
    assert {shape: 8 * ops.smacof_ws_doubles(*shape) for shape in WS_BYTES} == WS_BYTES
    assert size_fn(0, 5, 2) == size_fn(2, 0, 2) == size_fn(2, 5, 0) == size_fn(2, -5, 2) == 0


@needs_lib
def test_bad_arguments_return_before_any_hip_call():
    from hdpgpc_amd import _ffi
    fn = _ffi.lib.hgp_smacof_steps_f64
    buf = (ctypes.c_double * 64)()             # never dereferenced: every call below returns before a launch
    q = ctypes.cast(buf, vp)

    def call(n=4, p=2, B=1, ld=None, n_steps=1, ws_bytes=1 << 40, **ptr):
        a = {k: ptr.get(k, q) for k in ("delta", "X", "state", "status", "stress", "n_iter", "ws")}
        return fn(a["delta"], n if ld is None else ld, n, p, B, a["X"], 1e-6, n_steps, 10, a["state"], a["status"], a["stress"],
                  a["n_iter"], a["ws"], ws_bytes, None)

    assert call(n=0) == -1 and call(n=-2) == -1
    assert call(p=0) == -1 and call(p=4) == -1
    assert call(B=0) == -1 and call(B=-1) == -1
    assert call(n_steps=-1) == -1
    assert call(ld=3) == -1
    for k in ("delta", "X", "state", "status", "stress", "n_iter", "ws"):
        assert call(**{k: None}) == -1, k
    need = _ffi.lib.hgp_smacof_ws_bytes(2, 5, 2)   # one byte short, everything else valid: refused (no GPU here: before any HIP call)
    assert need > 0 and call(n=5, p=2, B=2, ws_bytes=need - 1) == -1
