"""CPU-side checks of the ragged pair call's boundary (include/hdpgpc_hip_ragged.h): the header parses with the one parser, its
binding is the pinned one and sits in a table of its own, the library exports the symbol, the main header's table and the ABI
version are untouched, and the argument checks that need no plan happen before any HIP call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from hdpgpc_amd import _cheader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
HEADER = os.path.join(ROOT, "include", "hdpgpc_hip.h")
RAGGED_HEADER = os.path.join(ROOT, "include", "hdpgpc_hip_ragged.h")
CLANG = "/opt/rocm/llvm/bin/clang"

i32, vp = ctypes.c_int, ctypes.c_void_p
NAME = "hgp_loglik_pairs_ragged_f64"
PINNED = {NAME: (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp])}


def parsed(path):
    with open(path) as f:
        return _cheader.parse_header(f.read())


def test_ragged_header_parses_to_the_pinned_binding():
    funcs, structs, defines = parsed(RAGGED_HEADER)
    assert funcs == PINNED
    assert structs == {} and defines == {}


def test_ragged_header_compiles_as_c_alone_and_next_to_the_main_header(tmp_path):
    for k, inc in enumerate(('#include "hdpgpc_hip_ragged.h"', '#include "hdpgpc_hip.h"\n#include "hdpgpc_hip_ragged.h"',
                             '#include "hdpgpc_hip_ragged.h"\n#include "hdpgpc_hip.h"')):
        src = tmp_path / f"probe{k}.c"
        src.write_text(f"{inc}\nint main(void) {{ return {NAME}(0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0) == 0; }}\n")
        subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], check=True)


def test_library_exports_the_ragged_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert NAME in set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))


def test_ragged_table_is_separate_from_the_main_headers():
    from hdpgpc_amd import _ffi
    assert _ffi.RAGGED_EXPORTS == [NAME]
    assert _ffi.EXPORTS == sorted(parsed(HEADER)[0])
    assert NAME not in _ffi.EXPORTS and NAME not in _ffi.FIT_EXPORTS and NAME not in _ffi.MDS_EXPORTS
    assert _ffi.ABI_VERSION == 7
    fn = getattr(_ffi.lib, NAME)
    assert (fn.restype, list(fn.argtypes)) == PINNED[NAME]


def test_bad_arguments_return_before_any_hip_call():
    from hdpgpc_amd import _ffi
    fn = getattr(_ffi.lib, NAME)
    buf = (ctypes.c_double * 64)()             # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, vp)
    assert fn(None, p, p, 3, 8, p, None, None, p, None, None, None) == -1       # no plan
    assert fn(None, p, p, 3, 8, None, None, None, p, None, None, None) == -1    # no plan, no lengths
    assert fn(None, p, p, 0, 8, p, None, None, p, None, None, None) == 0        # an empty batch is a no-op, as in the rectangular call


def test_pad_ragged_argument_checks():
    """ops.pad_ragged's host logic (the padded tensors themselves are looked at on the GPU tier)."""
    from hdpgpc_amd import ops
    with pytest.raises(ValueError):
        ops.pad_ragged([], [], device="cpu")
    with pytest.raises(ValueError):
        ops.pad_ragged([np.arange(3.0)], [np.arange(4.0)], device="cpu")
    with pytest.raises(ValueError):
        ops.pad_ragged([np.arange(3.0), np.arange(0.0)], [np.arange(3.0), np.arange(0.0)], device="cpu")
    X, Y, lens = ops.pad_ragged([np.arange(3.0), np.arange(5.0)[:, None]], [np.ones(3), 2.0 * np.ones(5)], device="cpu")
    assert X.shape == (2, 5) and Y.shape == (2, 5) and lens.tolist() == [3, 5] and str(lens.dtype) == "torch.int32"
    assert np.array_equal(np.isnan(X.numpy()), np.array([[0, 0, 0, 1, 1], [0] * 5], dtype=bool))
    assert np.array_equal(np.isnan(Y.numpy()), np.isnan(X.numpy())) and float(Y[1, 4]) == 2.0
    X, Y, lens = ops.pad_ragged([np.arange(2.0), np.arange(3.0)], [np.ones((2, 2)), np.ones((3, 2))], device="cpu")
    assert Y.shape == (2, 3, 2) and bool(np.isnan(Y.numpy()[0, 2]).all())
