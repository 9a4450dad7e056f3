"""CPU-side checks of the boundary: the shared library loads and exports every symbol the header declares, and the ctypes
binding read from the header is the one the C compiler sees."""
import ctypes
import os
import re
import subprocess

import pytest

from hdpgpc_amd import _cheader  # the header parser alone: needs neither the built library nor torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
HEADER = os.path.join(ROOT, "include", "hdpgpc_hip.h")
CLANG = "/opt/rocm/llvm/bin/clang"       # the host C compiler the build already requires


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
    assert _ffi.lib.hgp_abi_version() == 7
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


# The binding as it was written by hand before it was read from the header: the parser must reproduce it element for element.
i32, i64, f64, vp, sz = ctypes.c_int, ctypes.c_long, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
PINNED = {
    "hgp_abi_version": (i32, []),
    "hgp_debug_mfma_f64": (i32, [vp, vp, vp, vp]),
    "hgp_debug_exp_neg_f64": (i32, [vp, i32, vp, vp]),
    "hgp_gram_rbf_f64": (i32, [vp, i32, vp, i32, f64, f64, f64, vp, vp]),
    "hgp_potrf_batched_f64": (i32, [vp, i32, i32, f64, f64, vp, vp, vp, vp]),
    "hgp_chol_inverse_batched_f64": (i32, [vp, i32, i32, f64, f64, vp, vp, vp]),
    "hgp_chol_inverse_ws_f64": (i32, [vp, i32, i32, f64, f64, vp, vp, vp, vp]),
    "hgp_rts_chain_f64": (i32, [vp, vp, vp, vp, vp, i32, i32, vp]),
    "hgp_gemm_add_batched_f64": (i32, [i32, i32, i32, i32, i32, f64, vp, i32, i64, vp, i32, i64, f64, vp, i32, i64, vp, i32, i64, i32, vp]),
    "hgp_score_groups_f64": (i32, [vp, i32, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, i32, vp, f64, vp, vp, vp, vp]),
    "hgp_score_each_f64": (i32, [vp, i32, vp, i64, vp, i64, i32, vp, vp, vp, i32, f64, i32, vp, vp, vp, vp]),
    "hgp_pairs_plan_device_bytes": (sz, [i32, i32, i32]),
    "hgp_pairs_plan_create": (i32, [ctypes.POINTER(vp), i32, i32, i32, ctypes.POINTER(f64), vp, sz]),
    "hgp_pairs_plan_destroy": (None, [vp]),
    "hgp_pairs_plan_update": (i32, [vp, vp, vp, vp, vp, vp]),
    "hgp_pairs_plan_scalars": (vp, [vp]),
    "hgp_pairs_plan_set_accuracy": (i32, [vp, f64]),
    "hgp_pairs_plan_set_score_output": (i32, [vp, i32]),
    "hgp_loglik_pairs_f64": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]),
    "hgp_gemm_batched_f64": (i32, [i32, i32, i32, i32, i32, f64, vp, i32, i64, vp, i32, i64, f64, vp, i32, i64, i32, vp]),
    "hgp_matrix_lik_ws_bytes": (sz, [i32, i32]),
    "hgp_lat_error_f64": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]),
    "hgp_mniw_loglik_f64": (i32, [vp, vp, vp, vp, vp, i32, i64, i32, i32, vp, vp, vp, sz, vp]),
    "hgp_warp_cov_f64": (i32, [vp, i32, f64, f64, f64, i32, vp, vp]),
    "hgp_chol_rank1_f64": (i32, [vp, vp, vp, vp, i32, i32, vp, vp]),
    "hgp_trsv_lower_quad_f64": (i32, [vp, i32, vp, i32, vp, vp]),
    "hgp_hmm_messages_f64": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, vp]),
    "hgp_hmm_local_terms_f64": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "hgp_loglik_rows_f64": (i32, [vp, i32, i32, vp, vp, vp]),
    "hgp_assign_f64": (i32, [vp, vp, i32, i32, vp, vp, vp]),
    "hgp_warp_batch_f64": (i32, [vp, vp, vp, i64, i32, i32, i32, i32, i32, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp, vp]),
    "hgp_gemm_list_f64": (i32, [vp, i32, i32, vp]),
    "hgp_gemm_list_mapped_f64": (i32, [vp, i32, vp, i32, vp]),
    "hgp_chol_inverse_rhs_batched_f64": (i32, [vp, i32, i32, f64, f64, vp, vp, vp, i32, vp, vp, vp]),
    "hgp_copy_list_f64": (i32, [vp, i32, i64, vp]),
    "hgp_lds_chain_gather2_batched_f64": (i32, [vp, i32, i32, vp]),
    "hgp_lds_chain_finish2_batched_f64": (i32, [vp, i32, i32, vp]),
    "hgp_trsv_lower_solve_f64": (i32, [vp, i32, vp, i32, vp, vp, vp]),
    "hgp_lml_grad_f64": (i32, [vp, vp, vp, i32, f64, f64, f64, vp, vp]),
    "hgp_kl_sym_f64": (i32, [vp, vp, vp, i32, vp, vp, vp, i32, i32, vp, vp]),
    "hgp_pred_bands_ws_bytes": (sz, [i32, i32]),
    "hgp_pred_bands_f64": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, sz, vp]),
    "hgp_sample_states_ws_bytes": (sz, [i32, i32]),
    "hgp_sample_states_f64": (i32, [vp, vp, vp, i32, i32, vp, i32, i32, f64, vp, vp, vp, sz, vp]),
}


def parsed():
    with open(HEADER) as f:
        return _cheader.parse_header(f.read())


def test_parser_reproduces_the_pinned_binding():
    funcs, _, defines = parsed()
    assert sorted(funcs) == sorted(PINNED) == header_symbols()
    for name, sig in PINNED.items():
        assert funcs[name] == sig, name
    assert defines == {"HGP_ABI_VERSION": 7, "HGP_MAX_T_WAVE": 128, "HGP_MAX_T_COOP": 256}


STRUCTS = {"hgp_gemm_item": ("GemmItem", 104), "hgp_chain_gather_desc": ("ChainGatherDesc", 128),
           "hgp_chain_finish_desc": ("ChainFinishDesc", 192), "hgp_copy_item": ("CopyItem", 24)}
# hgp_pred_bands_ws_bytes(S, T) and hgp_sample_states_ws_bytes(S, T) as the header's two workspace macros gave
# them (doubles, times 8) before the library reported its workspaces itself: a caller that sized its buffer by
# the macro stays correct.  Both sides of the wave / cooperative switch.
BANDS_WS_BYTES = {(1, 1): 56, (7, 128): 1835288, (7, 129): 2795968, (3, 256): 4718712}
SAMPLE_WS_BYTES = {(1, 1): 16, (7, 128): 917560, (7, 129): 931952, (3, 256): 1572888}


@pytest.fixture(scope="module")
def c_probe(tmp_path_factory):
    """{key: value} as the C compiler sees the header: sizeof of every struct, offsetof of every field."""
    _, structs, _ = parsed()
    assert sorted(structs) == sorted(STRUCTS)
    probes = []
    for s, fields in structs.items():
        probes.append((f"sizeof {s}", f"sizeof({s})"))
        probes += [(f"{s}.{name}", f"offsetof({s}, {name})") for name, _ in fields]
    d = tmp_path_factory.mktemp("c_probe")
    body = "\n".join(f'  printf("{k}=%zu\\n", (size_t)({expr}));' for k, expr in probes)
    (d / "probe.c").write_text(f'#include <stdio.h>\n#include "hdpgpc_hip.h"\nint main(void) {{\n{body}\n  return 0;\n}}\n')
    subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(d / "probe"), str(d / "probe.c")],
                   check=True)
    out = subprocess.run([str(d / "probe")], capture_output=True, text=True, check=True).stdout
    got = {k: int(v) for k, v in (line.split("=") for line in out.splitlines())}
    assert sorted(got) == sorted(k for k, _ in probes)
    return got


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_struct_layouts_match_the_c_compiler(c_probe):
    from hdpgpc_amd import _ffi
    _, structs, _ = parsed()
    for s, (cls_name, size) in STRUCTS.items():
        cls = getattr(_ffi, cls_name)
        assert [n for n, _ in cls._fields_] == [n for n, _ in structs[s]], s
        assert ctypes.sizeof(cls) == c_probe[f"sizeof {s}"] == size, s
        for name, _ in cls._fields_:
            assert getattr(cls, name).offset == c_probe[f"{s}.{name}"], (s, name)


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_workspace_bytes_are_pinned():
    from hdpgpc_amd import _ffi, ops
    for pinned, size_fn, doubles in ((BANDS_WS_BYTES, _ffi.lib.hgp_pred_bands_ws_bytes, ops.pred_bands_ws_doubles),
                                     (SAMPLE_WS_BYTES, _ffi.lib.hgp_sample_states_ws_bytes, ops.sample_ws_doubles)):
        assert {shape: size_fn(*shape) for shape in pinned} == pinned
        assert {shape: 8 * doubles(*shape) for shape in pinned} == pinned
        assert size_fn(0, 16) == size_fn(2, 0) == size_fn(-1, 16) == 0


@pytest.mark.parametrize("decl, names", [
    ("int hgp_bad(const double* x, float scale, void* stream);", "float scale"),
    ("int hgp_bad(const double* x, unsigned n, void* stream);", "unsigned n"),
    ("int hgp_bad(const double* x, unsigned int n, void* stream);", "unsigned int n"),
    ("int hgp_bad(void (*done)(int), void* stream);", "hgp_bad"),
    ("typedef struct hgp_bad { const double* A; int flags : 3; } hgp_bad;", "int flags : 3"),
    ("typedef struct hgp_bad { struct { int a; } in; int T; } hgp_bad;", "hgp_bad"),
    ("int hgp_bad(hgp_unknown x, void* stream);", "hgp_unknown x"),
    ("int hgp_bad(const double* x, int n", "hgp_bad"),
    ("int hgp_bad(const double* x, int n\nint hgp_good(const double* y, int n, void* stream);", "hgp_bad"),
], ids=["float", "unsigned", "unsigned-int", "function-pointer", "bit-field", "nested-struct", "unknown-type", "unterminated",
        "unterminated-then-valid"])
def test_parser_raises_on_what_it_cannot_map(decl, names):
    ok = "int hgp_ok(const double* x, int n, void* stream);\n"
    assert list(_cheader.parse_header(ok)[0]) == ["hgp_ok"]
    with pytest.raises(ValueError, match=re.escape(names)):
        _cheader.parse_header(ok + decl + "\n")


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_abi_guard_refuses_a_library_of_another_header():
    from hdpgpc_amd import _ffi
    _ffi.check_abi(7, 7)
    with pytest.raises(ImportError, match="library built from another header: rebuild"):
        _ffi.check_abi(7, 8)
    assert _ffi.ABI_VERSION == 7 and (_ffi.MAX_T_WAVE, _ffi.MAX_T_COOP) == (128, 256)
