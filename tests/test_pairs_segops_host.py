"""CPU-side checks of the segment-operator entries' boundary (include/hdpgpc_hip_segops.h): the header parses with the one parser
to the pinned binding and sits in a table of its own, it compiles as C alone and next to the other headers, the library exports
the symbols, the main header's table and the ABI version are untouched, and what can be decided without a plan is decided
before any HIP call.  (A plan needs a device buffer, so the byte counts per plan size - 0 outside padded sizes 96 and 128,
record size x groups x N inside - are checked on the GPU tier, tests/test_gpu_pairs_segops.py::test_sizes_and_argument_errors.)"""
import ctypes
import os
import re
import subprocess

from hdpgpc_amd import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
INCLUDE = os.path.join(ROOT, "include")
CLANG = "/opt/rocm/llvm/bin/clang"

i32, vp, sz = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t
BYTES, ENTRY = "hgp_pairs_segops_bytes", "hgp_loglik_pairs_segops_f64"
PINNED = {BYTES: (sz, [vp, i32, i32]), ENTRY: (i32, [vp, vp, sz, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp])}


def parsed(name):
    with open(os.path.join(INCLUDE, name)) as f:
        return _cheader.parse_header(f.read())


def test_segops_header_parses_to_the_pinned_binding():
    funcs, structs, defines = parsed("hdpgpc_hip_segops.h")
    assert funcs == PINNED
    assert structs == {} and defines == {}


def test_segops_header_compiles_as_c_alone_and_next_to_the_other_headers(tmp_path):
    call = f"{ENTRY}(0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0) == 0 && {BYTES}(0, 1, 1) == 0"
    for k, inc in enumerate(('#include "hdpgpc_hip_segops.h"',
                             '#include "hdpgpc_hip.h"\n#include "hdpgpc_hip_ragged.h"\n#include "hdpgpc_hip_segops.h"',
                             '#include "hdpgpc_hip_segops.h"\n#include "hdpgpc_hip_ragged.h"\n#include "hdpgpc_hip.h"')):
        src = tmp_path / f"probe{k}.c"
        src.write_text(f"{inc}\nint main(void) {{ return {call}; }}\n")
        subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)], check=True)


def test_library_exports_the_segops_symbols():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert set(PINNED) <= set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))


def test_segops_table_is_separate_from_the_other_headers():
    from hdpgpc_amd import _ffi
    assert _ffi.SEGOPS_EXPORTS == sorted(PINNED)
    assert _ffi.EXPORTS == sorted(parsed("hdpgpc_hip.h")[0]) and _ffi.ABI_VERSION == 7
    for name in PINNED:
        assert all(name not in t for t in (_ffi.EXPORTS, _ffi.FIT_EXPORTS, _ffi.MDS_EXPORTS, _ffi.RAGGED_EXPORTS, _ffi.PROJECT_EXPORTS))
        fn = getattr(_ffi.lib, name)
        assert (fn.restype, list(fn.argtypes)) == PINNED[name]


def test_bytes_and_bad_arguments_without_a_gpu():
    from hdpgpc_amd import _ffi
    lib = _ffi.lib
    assert lib.hgp_pairs_segops_bytes(None, 8, 128) == 0      # no plan: no band kernel serves it
    buf = (ctypes.c_double * 64)()                            # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, vp)
    entry = lib.hgp_loglik_pairs_segops_f64
    assert entry(None, p, 512, p, p, 3, 8, None, None, None, p, None, None, None) == -1     # no plan
    assert entry(None, p, 512, p, p, 3, 8, p, None, None, p, None, None, None) == -1        # no plan, ragged
    assert entry(None, None, 0, p, p, -1, 8, None, None, None, p, None, None, None) == -1   # N < 0
    assert entry(None, p, 512, p, p, 0, 8, None, None, None, p, None, None, None) == 0      # an empty batch is a no-op
