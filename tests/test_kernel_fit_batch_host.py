"""CPU-side checks of the batched kernel fit's boundary (include/hdpgpc_hip_fit.h): the second header parses with the same
parser, its binding is the pinned one, the library exports the symbol, the main header's table is untouched, argument
validation happens before any HIP call, and the workspace size is the pinned one."""
import ctypes
import os
import re
import subprocess

import pytest

from hdpgpc_amd import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
HEADER = os.path.join(ROOT, "include", "hdpgpc_hip.h")
FIT_HEADER = os.path.join(ROOT, "include", "hdpgpc_hip_fit.h")
CLANG = "/opt/rocm/llvm/bin/clang"

i32, i64, f64, vp, sz = ctypes.c_int, ctypes.c_long, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
PINNED = {"hgp_kernel_fit_ws_bytes": (sz, [i32, i32]),
          "hgp_kernel_fit_steps_f64": (i32, [vp, i64, vp, i32, i32, vp, f64, i32, i32, i32, vp, vp, vp, i32, vp, sz, vp])}
# hgp_kernel_fit_ws_bytes(B, T) as the header's workspace macro gave it (doubles, times 8) before the library reported its
# workspace itself: a caller that sized its buffer by the macro stays correct
WS_BYTES = {(1, 1): 24, (7, 128): 1835064, (7, 129): 1863848, (3, 256): 3145752}
needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")


def parsed(path):
    with open(path) as f:
        return _cheader.parse_header(f.read())


def test_fit_header_parses_to_the_pinned_binding():
    funcs, structs, defines = parsed(FIT_HEADER)
    assert funcs == PINNED
    assert structs == {}
    assert defines == {"HGP_FIT_STATE_DOUBLES": 32}


@needs_lib
def test_library_exports_the_fit_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert set(PINNED) <= set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))


@needs_lib
def test_fit_table_is_separate_from_the_main_headers():
    from hdpgpc_amd import _ffi
    assert _ffi.FIT_EXPORTS == sorted(PINNED)
    assert _ffi.EXPORTS == sorted(parsed(HEADER)[0])
    assert not set(PINNED) & set(_ffi.EXPORTS)
    assert _ffi.FIT_STATE_DOUBLES == 32 and _ffi.ABI_VERSION == 7
    for name, sig in PINNED.items():
        fn = getattr(_ffi.lib, name)
        assert (fn.restype, list(fn.argtypes)) == sig, name


@needs_lib
def test_bad_arguments_return_before_any_hip_call():
    from hdpgpc_amd import _ffi
    fn = _ffi.lib.hgp_kernel_fit_steps_f64
    buf = (ctypes.c_double * 64)()             # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, vp)

    def call(T=4, B=1, Y=p, state=p, x=p, n_steps=1, x_stride=0, ws_bytes=1 << 40):
        return fn(x, x_stride, Y, T, B, p, 0.1, n_steps, 10, 20, state, p, None, 0, p, ws_bytes, None)

    assert call(T=0) == -1 and call(T=-3) == -1
    assert call(B=0) == -1 and call(B=-1) == -1
    assert call(Y=None) == -1 and call(state=None) == -1 and call(x=None) == -1
    assert call(n_steps=-1) == -1 and call(x_stride=-4) == -1
    assert call(T=257) == -2
    assert call(T=257, Y=None) == -1           # a bad argument is reported first
    assert call(T=257, ws_bytes=0) == -2       # and an unsupported size before a workspace that is too small
    for T in (16, 129):                        # one byte short, everything else valid: refused (no GPU here: before any HIP call)
        need = _ffi.lib.hgp_kernel_fit_ws_bytes(2, T)
        assert need > 0 and call(T=T, B=2, ws_bytes=need - 1) == -1


@pytest.fixture(scope="module")
def c_probe(tmp_path_factory):
    probes = [("state", "HGP_FIT_STATE_DOUBLES")]
    d = tmp_path_factory.mktemp("c_probe_fit")
    body = "\n".join(f'  printf("{k}=%zu\\n", (size_t)({expr}));' for k, expr in probes)
    (d / "probe.c").write_text(f'#include <stdio.h>\n#include "hdpgpc_hip_fit.h"\nint main(void) {{\n{body}\n  return 0;\n}}\n')
    subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(FIT_HEADER), "-o", str(d / "probe"), str(d / "probe.c")],
                   check=True)
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (line.split("=") for line in out.splitlines())}


@needs_lib
def test_state_size_matches_the_header_macro_and_workspace_bytes_are_pinned(c_probe):
    from hdpgpc_amd import _ffi, ops
    assert c_probe["state"] == _ffi.FIT_STATE_DOUBLES == 32
    size_fn = _ffi.lib.hgp_kernel_fit_ws_bytes
    assert {shape: size_fn(*shape) for shape in WS_BYTES} == WS_BYTES
    assert {shape: 8 * ops.kernel_fit_ws_doubles(*shape) for shape in WS_BYTES} == WS_BYTES
    assert size_fn(0, 16) == size_fn(2, 0) == size_fn(-1, 16) == 0
