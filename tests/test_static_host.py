"""CPU tier of ``model_type='static'`` (clusters whose template does not evolve: Gamma = 0): the constructor and the bookkeeping
around the option, the offline loop's host logic against the reference's static run (tests/golden/make_golden_static.py) through
tests/cpu_double.py, and the boundary of include/hdpgpc_hip_static.h - the header parses with the one parser, its binding sits in a
table of its own, the main header's table and the ABI version are untouched, and the argument checks happen before any HIP call.
The fused filter chain itself cannot run here: ``install`` below routes static chains to the eager methods, as cpu_double does
with the dynamic ones; the kernel runs in tests/test_gpu_static_chain.py and tests/test_gpu_static_driver.py."""
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import torch

import cpu_double
import static_trace
from conftest import golden
from hdpgpc_amd import _cheader
from offline_trace import compare_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "hdpgpc_amd", "lib", "libhdpgpc_hip.so")
HEADER = os.path.join(ROOT, "include", "hdpgpc_hip.h")
STATIC_HEADER = os.path.join(ROOT, "include", "hdpgpc_hip_static.h")
CLANG = "/opt/rocm/llvm/bin/clang"
i32, i64, vp, f64, sz = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_double, ctypes.c_size_t
WS, CALL = "hgp_static_chain_ws_bytes", "hgp_static_chain_steps_f64"
PINNED = {WS: (sz, [i32, i32]), CALL: (i32, [vp, i32, i32, i32, vp, sz, vp])}
DESC = [("A", vp), ("C", vp), ("Sigma", vp), ("Fs", vp), ("Ps", vp), ("pos", vp), ("Y", vp), ("y_idx", vp), ("info", vp), ("white", f64),
        ("pos0", i64), ("n", ctypes.c_int32), ("first", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32)]
T = 20


def install(monkeypatch):
    """cpu_double.install, and the new binding: no fused static chain on the CPU, one eager pass after the other."""
    cpu_double.install(monkeypatch)
    from hdpgpc_amd import chain_batch
    monkeypatch.setattr(chain_batch, "_static_fused", lambda job: False)


def _sw(**kw):
    import hdpgpc.GPI_HDP as hdpgp
    xb = np.arange(float(T))[:, None]
    sw = hdpgp.GPI_HDP(xb, ini_lengthscale=3.0, bound_lengthscale=(1.0, 20.0), ini_gamma=12.0, ini_sigma=9.0, ini_outputscale=300.0,
                       bound_sigma=(9e-5, 18.0), bound_gamma=(1e-4, 24.0), verbose=False, free_deg_MNIV=5, **kw)
    sw.fixed_theta = (341.0, 1.2, 4.66)
    return sw, xb


def _batch(N, seed=0):
    rng = np.random.default_rng(seed)
    base = 30.0 * np.sin(np.arange(T) / 3.0)
    return np.stack([base * (1.0 + 0.05 * rng.normal()) + rng.normal(size=T) for _ in range(N)])[:, :, None]


def _static(m):
    return not bool(torch.any(m.Gamma[-1] != 0))


def _lens(m):
    return [len(getattr(m, k)) for k in ("A", "Gamma", "C", "Sigma", "f_star", "f_star_sm", "cov_f", "cov_f_sm")]


# ------------------------------------------------------------------------------------------ constructor and bookkeeping
def test_constructor_accepts_static_lists_and_mixed_and_refuses_the_rest(monkeypatch):
    install(monkeypatch)
    from hdpgpc_amd.GPI_model import inv_wishart, matrix_normal_inv_wishart
    sw, _ = _sw(model_type='static')
    assert sw.model_type == ['static'] and sw.model_type_def == 'static' and _static(sw.gpmodels[0][0])
    sw, _ = _sw(M=3, model_type='static')
    assert sw.model_type == ['static'] * 3 and all(_static(m) for m in sw.gpmodels[0])
    sw, _ = _sw(M=2, model_type=['static', 'static'])
    assert all(_static(m) for m in sw.gpmodels[0])
    sw, _ = _sw(M=3, n_outputs=2, model_type=['dynamic', 'static', 'dynamic'])
    assert sw.model_type_def == 'dynamic'
    for lead in sw.gpmodels:
        assert [_static(m) for m in lead] == [False, True, False]
        # the observation distribution the reference gives each kind (GPI_model.py:170-175)
        assert [type(m.observation_params) for m in lead] == [matrix_normal_inv_wishart, inv_wishart, matrix_normal_inv_wishart]
    sw, _ = _sw(M=2, model_type=np.array(['static', 'dynamic']))
    assert [_static(m) for m in sw.gpmodels[0]] == [True, False] and sw.model_type_def == 'static'
    assert _sw(model_type='dynamic')[0].model_type == ['dynamic'] and not _static(_sw()[0].gpmodels[0][0])
    for bad in (dict(model_type='statik'), dict(model_type=None), dict(M=2, model_type=['static', 'fixed']),
                dict(M=2, model_type=['static']), dict(M=2, model_type=['static', 'dynamic', 'static'])):
        with pytest.raises(ValueError, match="model_type"):
            _sw(**bad)


def test_defaults_carry_the_type(monkeypatch):
    install(monkeypatch)
    sw, _ = _sw(M=2, model_type=['static', 'dynamic'])
    for gp in (sw.create_gp_default(), sw.create_gp_default(i=1)):          # a cluster born later takes the default: the first entry
        assert _static(gp) and not bool(torch.any(gp.Gamma_def != 0)) and torch.equal(gp.A[0], torch.eye(T, dtype=torch.float64))
        assert torch.equal(gp.Sigma[0], 9.0 * torch.eye(T, dtype=torch.float64))
    assert sw.get_default_options()["model_type"] == 'static'
    sw.set_default_options(model_type='dynamic')
    assert sw.model_type_def == 'dynamic' and not _static(sw.create_gp_default())
    assert torch.equal(sw.create_gp_default().Gamma[0], 12.0 * torch.eye(T, dtype=torch.float64))
    with pytest.raises(ValueError, match="model_type"):
        sw.set_default_options(model_type='frozen')
    sw, _ = _sw(M=2, model_type=['dynamic', 'static'])
    assert not _static(sw.create_gp_default()) and sw.get_default_options()["model_type"] == 'dynamic'


def test_parameter_lists_keep_length_one(monkeypatch):
    install(monkeypatch)
    N = 7
    sw, xb = _sw(model_type='static')
    y = _batch(N)
    m = sw.gpmodels[0][0]
    q, q_lat = m.full_pass_weighted(np.array([xb] * N), y, torch.ones(N))
    assert m.N == N and _lens(m) == [1] * 4 + [N + 1] * 4 and _static(m)
    assert q.shape == (N,) and bool(torch.all(torch.isfinite(q))) and not bool(torch.any(q_lat != 0))
    assert all(torch.equal(a, b) for a, b in zip(m.f_star, m.f_star_sm)) and all(torch.equal(a, b) for a, b in zip(m.cov_f, m.cov_f_sm))
    c = sw.gpmodel_deepcopy(m)
    assert _lens(c) == _lens(m) and c.N == N and _static(c) and type(c.observation_params) is type(m.observation_params)
    back = pickle.loads(pickle.dumps(sw))
    b = back.gpmodels[0][0]
    assert back.model_type == ['static'] and back.model_type_def == 'static' and _lens(b) == _lens(m) and _static(b)
    assert type(b.observation_params) is type(m.observation_params)
    for k in ("Sigma", "f_star", "cov_f_sm"):
        assert all(torch.equal(u, v) for u, v in zip(getattr(b, k), getattr(m, k)))
    assert _static(back.create_gp_default())
    sw.keep_last_all()
    assert _lens(m) == [1] * 4 + [2] * 4 and _static(m)


def test_online_step_and_warp_refuse_static_models(monkeypatch):
    install(monkeypatch)
    y = _batch(3)
    sw, xb = _sw(model_type='static')
    with pytest.raises(NotImplementedError, match="static"):
        sw.include_sample(xb, y[0], with_warp=False)
    sw, xb = _sw(M=2, model_type=['dynamic', 'static'])
    with pytest.raises(NotImplementedError, match="static"):
        sw.include_sample(xb, y[0], with_warp=False)
    with pytest.raises(NotImplementedError, match="static"):
        sw.include_batch(np.array([xb] * 3), y, warp=True)


def test_include_batch_static_trace_cpu(monkeypatch):
    """The host logic of the offline loop with static clusters against the reference's run on the first 60 beats of record 102
    (M = 6, sizes 28 / 20 / 6 / 3 / 2 / 1, six EM iterations, Q_lat identically zero): every call, every assignment, the
    numbers at the gate of test_offline_loop_host.py::test_include_batch_trace_cpu."""
    install(monkeypatch)
    g = golden("include_batch_r102_n60_static.npz")
    sw, tr = static_trace.run_offline(g)
    compare_trace(g, sw, tr, q_tol=1e-8)
    assert sw.M == 6 and [len(m.indexes) for m in sw.gpmodels[0]] == [28, 20, 6, 3, 2, 1]
    assert static_trace.static_lists_ok(sw)
    assert all(not e[2].any() for e in tr["em"])


# ------------------------------------------------------------------------------------------ the boundary
def parsed(path):
    with open(path) as f:
        return _cheader.parse_header(f.read())


def test_static_header_parses_to_the_pinned_binding():
    funcs, structs, defines = parsed(STATIC_HEADER)
    assert funcs == PINNED and defines == {}
    assert list(structs) == ["hgp_static_chain_desc"] and structs["hgp_static_chain_desc"] == DESC


def test_static_header_compiles_as_c_alone_and_next_to_the_main_header(tmp_path):
    for k, inc in enumerate(('#include "hdpgpc_hip_static.h"', '#include "hdpgpc_hip.h"\n#include "hdpgpc_hip_static.h"',
                             '#include "hdpgpc_hip_static.h"\n#include "hdpgpc_hip.h"')):
        src = tmp_path / f"probe{k}.c"
        src.write_text(f"{inc}\n_Static_assert(sizeof(hgp_static_chain_desc) == 104, \"layout\");\n"
                       f"int main(void) {{ return {CALL}(0, 0, 1, 1, 0, {WS}(1, 1), 0) == 0; }}\n")
        subprocess.run([CLANG, "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.dirname(HEADER), str(src)], check=True)


def test_library_exports_both_symbols_and_the_table_is_separate():
    from hdpgpc_amd import _ffi
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    assert {WS, CALL} <= set(re.findall(r"\bT (hgp_[a-z0-9_]+)", out))
    assert _ffi.STATIC_EXPORTS == sorted(PINNED)
    assert _ffi.EXPORTS == sorted(parsed(HEADER)[0])
    for name in PINNED:
        assert all(name not in t for t in (_ffi.EXPORTS, _ffi.FIT_EXPORTS, _ffi.MDS_EXPORTS, _ffi.RAGGED_EXPORTS, _ffi.PROJECT_EXPORTS,
                                           _ffi.SEGOPS_EXPORTS))
        fn = getattr(_ffi.lib, name)
        assert (fn.restype, list(fn.argtypes)) == PINNED[name]
    assert _ffi.ABI_VERSION == 7 and ctypes.sizeof(_ffi.StaticChainDesc) == 104


def test_workspace_size_and_bad_arguments_return_before_any_hip_call():
    from hdpgpc_amd import _ffi
    ws, fn = getattr(_ffi.lib, WS), getattr(_ffi.lib, CALL)
    assert ws(0, 90) == 0 and ws(-1, 90) == 0 and ws(3, 0) == 0 and ws(3, 129) == 0
    assert ws(1, 128) == 8 * 128 * 128 * 8 and ws(8, 90) == 8 * 8 * 90 * 90 * 8
    buf = (ctypes.c_double * 64)()             # never dereferenced: every call below returns before a launch
    p = ctypes.cast(buf, vp)
    need = ws(2, 90)
    assert fn(p, 0, 90, 5, p, need, None) == 0 and fn(p, 2, 90, 0, p, need, None) == 0 and fn(None, 0, 90, 5, None, 0, None) == 0
    assert fn(p, -1, 90, 5, p, need, None) == -1 and fn(p, 2, 0, 5, p, need, None) == -1 and fn(p, 2, 90, -1, p, need, None) == -1
    assert fn(None, 2, 90, 5, p, need, None) == -1 and fn(p, 2, 90, 5, None, need, None) == -1
    assert fn(p, 2, 90, 5, p, need - 1, None) == -1                      # one byte short
    assert fn(p, 2, 129, 5, p, 1 << 40, None) == -2                      # beyond the fused range: the caller keeps the eager path
