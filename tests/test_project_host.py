"""CPU-side checks of the projection of ragged batches onto the basis grid: the restatement of the reference's project_y
(tests/project_ref.py) against the reference's own recorded outputs (tests/golden/project_y.npz, written by
tests/golden/make_golden_project.py) and against a longdouble solve, and the boundary of include/hdpgpc_hip_project.h - the header
parses with the one parser, its binding sits in a table of its own, the library exports both symbols, the main header's table and
the ABI version are untouched, and the argument checks happen before any HIP call.

Observed when the fixture was written: the restatement reproduces the reference's twelve recorded outputs exactly (0.0 relative
to max |y_p|; the gate is 1e-12).  The reference's float64 numbers themselves sit up to 8.2e-13 (length-scale 1.2) and 2.6e-10
(length-scale 3.0, 45 points on a basis of 30) from the longdouble solve."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import project_ref
from hdpgpc_amd import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
HEADER = os.path.join(ROOT, "include", "hdpgpc_hip.h")
PROJECT_HEADER = os.path.join(ROOT, "include", "hdpgpc_hip_project.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "project_y.npz")
CLANG = "/opt/rocm/llvm/bin/clang"

i32, vp, f64, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_size_t
WS, CALL = "hgp_project_ragged_ws_bytes", "hgp_project_ragged_f64"
PINNED = {WS: (sz, [i32, i32, i32, i32]),
          CALL: (i32, [vp, vp, vp, i32, i32, i32, vp, i32, f64, f64, f64, vp, vp, vp, sz, vp])}


def parsed(path):
    with open(path) as f:
        return _cheader.parse_header(f.read())


def cases():
    g = np.load(GOLDEN)
    for k in range(int(g["n_cases"])):
        p = f"c{k}_"
        yield k, {n[len(p):]: g[n] for n in g.files if n.startswith(p)}


def test_restatement_reproduces_the_references_outputs():
    worst, shortcut = 0.0, 0
    for k, c in cases():
        got, _ = project_ref.project_y_ref(c["x"], c["y"], c.get("C"), None, c["xb"], *c["theta"])
        if c["x"].shape == c["xb"].shape and np.array_equal(c["x"], c["xb"]):
            assert got is not None and np.array_equal(got, c["y"]) and np.array_equal(c["yp"], c["y"])   # the short-circuit
            shortcut += 1
        err = project_ref.rel_err(got, c["yp"])
        worst = max(worst, err)
        assert err <= 1e-12, (k, err)
    assert shortcut == 2
    print(f"restatement vs recorded reference: worst {worst:.3e}")


def test_recorded_outputs_sit_where_float64_can_against_longdouble():
    """The reference's own numbers against the longdouble solve: the distance the GPU gates (1e-10 at length-scale 1.2, 1e-8 at
    3.0) leave room for."""
    for k, c in cases():
        if "C" in c or np.array_equal(c["x"], c["xb"]):
            continue
        ell = float(c["theta"][1])
        err = project_ref.rel_err(c["yp"], project_ref.project_y_longdouble(c["x"], c["y"], c["xb"], *c["theta"]))
        print(f"case {k} ell {ell} L {len(c['x'])} T {len(c['xb'])}: reference vs longdouble {err:.3e}")
        assert err <= (1e-11 if ell < 2.0 else 1e-9), (k, err)


def test_project_header_parses_to_the_pinned_binding():
    funcs, structs, defines = parsed(PROJECT_HEADER)
    assert funcs == PINNED
    assert structs == {} and defines == {}


def test_project_header_compiles_as_c_alone_and_next_to_the_main_header(tmp_path):
    for k, inc in enumerate(('#include "hdpgpc_hip_project.h"', '#include "hdpgpc_hip.h"\n#include "hdpgpc_hip_project.h"',
                             '#include "hdpgpc_hip_project.h"\n#include "hdpgpc_hip.h"')):
        src = tmp_path / f"probe{k}.c"
        src.write_text(f"{inc}\nint main(void) {{ return {CALL}(0, 0, 0, 1, 1, 1, 0, 1, 1.0, 1.0, 0.0, 0, 0, 0, {WS}(1, 1, 1, 1), 0) == 0; }}\n")
        subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], check=True)


def test_library_exports_both_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert {WS, CALL} <= set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))


def test_project_table_is_separate_from_the_main_headers():
    from hdpgpc_amd import _ffi
    assert _ffi.PROJECT_EXPORTS == sorted(PINNED)
    assert _ffi.EXPORTS == sorted(parsed(HEADER)[0])
    for name in PINNED:
        assert all(name not in t for t in (_ffi.EXPORTS, _ffi.FIT_EXPORTS, _ffi.MDS_EXPORTS, _ffi.RAGGED_EXPORTS))
        fn = getattr(_ffi.lib, name)
        assert (fn.restype, list(fn.argtypes)) == PINNED[name]
    assert _ffi.ABI_VERSION == 7


def test_workspace_size():
    from hdpgpc_amd import _ffi
    ws = getattr(_ffi.lib, WS)
    assert ws(0, 256, 256, 2) == 0 and ws(0, 90, 90, 1) == 0
    assert ws(7, 128, 256, 3) == 0                           # the one-wave range needs none
    assert ws(7, 129, 90, 3) == 2 * 7 * 129 * 129 * 8
    assert ws(5, 256, 256, 17) == 2 * 5 * 256 * 256 * 8      # the leads do not enter


def test_bad_arguments_return_before_any_hip_call():
    from hdpgpc_amd import _ffi
    fn = getattr(_ffi.lib, CALL)
    buf = (ctypes.c_double * 64)()             # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, vp)

    def call(x=p, y=p, lengths=p, N=3, ld=8, D=2, xb=p, T=8, c=300.0, ell=1.2, jitter=1e-4, yp=p, info=p, ws=None, ws_bytes=0):
        return fn(x, y, lengths, N, ld, D, xb, T, c, ell, jitter, yp, info, ws, ws_bytes, None)

    assert call(N=0) == 0 and call(N=0, x=None, yp=None) == 0            # an empty batch is a no-op
    assert call(N=-1) == -1
    for bad in (dict(x=None), dict(y=None), dict(xb=None), dict(yp=None), dict(info=None), dict(ld=0), dict(D=0), dict(T=0),
                dict(ell=0.0), dict(ell=-1.0), dict(ell=float("nan")), dict(c=0.0), dict(c=float("nan")), dict(jitter=-1e-4),
                dict(jitter=float("nan"))):
        assert call(**bad) == -1, bad
    assert call(ld=257) == -2 and call(T=257) == -2                      # beyond the build
    assert call(ld=200) == -2                                            # needs a workspace: none given
    assert call(ld=200, ws=p, ws_bytes=2 * 3 * 200 * 200 * 8 - 1) == -2  # ... or one that is too small


def test_host_tensors_are_refused():
    """ops.project_ragged takes device tensors only (its length checks are looked at on the GPU tier)."""
    import torch
    from hdpgpc_amd import ops
    with pytest.raises(TypeError):
        ops.project_ragged(torch.zeros(2, 4, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.float64), None,
                           torch.zeros(4, dtype=torch.float64), 300.0, 1.2)
