"""CPU-side checks of the boundary: the shared library loads and exports every symbol the header declares."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "hdpgpc_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(hgp_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_path():
    syms = header_symbols()
    for s in ("hgp_gram_rbf_f64", "hgp_potrf_batched_f64", "hgp_score_groups_f64", "hgp_loglik_pairs_f64",
              "hgp_pairs_plan_create", "hgp_pairs_plan_update"):
        assert s in syms


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_library_exports_every_declared_symbol():
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))
    missing = [s for s in header_symbols() if s not in exported]
    assert not missing, missing


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_ctypes_binding_loads_without_a_gpu():
    from hdpgpc_amd import _ffi
    assert _ffi.lib.hgp_abi_version() == 6
    assert set(_ffi.EXPORTS) == set(header_symbols())
    # argument validation happens before any HIP call
    assert _ffi.lib.hgp_gram_rbf_f64(None, 4, None, 4, 1.0, 1.0, 0.0, None, None) == -1
    assert _ffi.lib.hgp_pairs_plan_device_bytes(0, 8, 2) == 0
    assert _ffi.lib.hgp_pairs_plan_device_bytes(128, 128, 8) > 8 * 7 * 128 * 128 * 8


# hgp_pairs_plan_device_bytes(T, Ts_max, K) as the library returned it before the layout was stated once: one shape per branch
# of the layout (padded sizes 32, 64, 96, 128 of the one-wave kernels; 192, 256 with the cooperative kernel's overflow areas), and
# the padded size taken from the larger of T and Ts_max, across 128.
PLAN_BYTES = {
    (20, 20, 1): 4544512, (20, 20, 8): 5150464, (20, 20, 16): 5843456,
    (50, 50, 1): 17361664, (50, 50, 8): 19605504, (50, 50, 16): 22170368,
    (90, 90, 1): 38714880, (90, 90, 8): 43628800, (90, 90, 16): 49245184,
    (128, 128, 1): 68604160, (128, 128, 8): 77220352, (128, 128, 16): 87067904,
    (150, 150, 1): 179159040, (150, 150, 8): 198276352, (150, 150, 16): 220125184,
    (256, 256, 1): 357410304, (256, 256, 8): 391157504, (256, 256, 16): 429726208,
    (120, 200, 8): 391157504, (200, 120, 8): 391157504, (128, 129, 1): 179159040,
}


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_plan_device_bytes_are_pinned():
    from hdpgpc_amd import _ffi
    got = {shape: _ffi.lib.hgp_pairs_plan_device_bytes(*shape) for shape in PLAN_BYTES}
    assert got == PLAN_BYTES
