"""The kernels of hgp_gp.hip called directly at the sizes the goldens (T <= 90, n <= 178) never reach: the triangular solve
with more than one pass of its 256-thread loops, up to its limit T = 2048 and with ld > T; the a10 gradient with fewer and more
elements than threads; the a11 covariance without normalisation, on grids that do not start at zero or decrease; the Gram
matrix at one row, one column and sizes around a block.

References are np.longdouble evaluations of the same sums (bounds from the number of roundings, stated at each test) or, for
the element-wise kernels, the oracle's formula at the rtol the golden test of the Gram matrix uses.  Inputs the kernels must not
read are NaN."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import hdpgpc_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

EPS = 2.0 ** -52
LD = np.longdouble


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------------ triangular solve
def trsv_inputs(T):
    """G [T, T+3]: lower triangle 0.5/sqrt(T) N(0,1), diagonal U(1,2) (cond(tril G) about 3 at every size), everything above
    the diagonal and the three padding columns NaN."""
    rng = np.random.default_rng(1000 + T)
    G = np.full((T, T + 3), np.nan)
    G[:, :T][np.tril_indices(T, -1)] = (0.5 / np.sqrt(T) * rng.normal(size=(T, T)))[np.tril_indices(T, -1)]
    G[np.arange(T), np.arange(T)] = rng.uniform(1.0, 2.0, T)
    return G, rng.normal(size=T)


def trsv_reference(G, y):
    """w = L^-1 y, |w|^2 and alpha = L^-T w by the two substitutions in np.longdouble."""
    T = y.size
    L = np.tril(np.nan_to_num(G[:, :T])).astype(LD)
    w = y.astype(LD)
    for k in range(T):
        w[k] /= L[k, k]
        w[k + 1:] -= L[k + 1:, k] * w[k]
    quad = np.sum(w * w)
    for k in range(T - 1, -1, -1):
        w[k] /= L[k, k]
        w[:k] -= L[k, :k] * w[k]
    return quad, w


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 700, 2048])
def test_trsv_lower(T):
    """Each substitution is backward stable with a constant of T roundings per row; with cond about 3 the forward error stays
    below 8 T eps with room (float64 NumPy in the kernel's column order: 4e-15 at T = 2048, bound 3.6e-12)."""
    G, y = trsv_inputs(T)
    quad_ref, alpha_ref = trsv_reference(G, y)
    Gd, yd = dev(G), dev(y)
    assert Gd.shape[1] == T + 3
    quad = float(ops.trsv_lower_quad(Gd, yd))
    alpha, quad2 = ops.trsv_lower_solve(Gd, yd)
    alpha, quad2 = alpha.cpu().numpy(), float(quad2)
    e_quad = abs(float((LD(quad) - quad_ref) / quad_ref))
    e_alpha = float(np.max(np.abs(alpha.astype(LD) - alpha_ref)) / np.max(np.abs(alpha_ref)))
    print(f"trsv T={T}: quad {e_quad:.2e}  alpha {e_alpha:.2e}  bound {8 * T * EPS:.2e}")
    assert np.all(np.isfinite(alpha)) and np.isfinite(quad)
    assert e_quad <= 8 * T * EPS and e_alpha <= 8 * T * EPS
    assert quad2 == quad                                   # same kernel, same bits


def test_trsv_status_codes():
    lib = _ffi.lib
    T = 2049
    G = torch.eye(T, dtype=torch.float64, device="cuda")
    y = torch.ones(T, dtype=torch.float64, device="cuda")
    out = torch.full((T + 1,), float("nan"), dtype=torch.float64, device="cuda")
    z = ctypes.c_void_p(0)
    assert lib.hgp_trsv_lower_quad_f64(ptr(G), T, ptr(y), T, ptr(out), z) == -2
    assert lib.hgp_trsv_lower_solve_f64(ptr(G), T, ptr(y), T, ptr(out[1:]), ptr(out), z) == -2
    assert lib.hgp_trsv_lower_quad_f64(ptr(G), 63, ptr(y), 64, ptr(out), z) == -1
    assert lib.hgp_trsv_lower_solve_f64(ptr(G), 63, ptr(y), 64, ptr(out[1:]), ptr(out), z) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ a10 gradient
@pytest.mark.parametrize("theta", [(341.0, 1.2, 0.9), (3.0, 7.5, 1e-3)])
@pytest.mark.parametrize("T", [1, 15, 16, 17, 257])
def test_lml_grad(T, theta):
    """out[k] = 0.5 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dtheta_k.  Each of the 256 threads adds about T^2 / 256 terms by fma
    in turn, an eight-level tree adds the partial sums, exp and the products before it cost a few ulp per term:
    |out - ref| <= (T^2 / 256 + 32) eps sum |term|."""
    c, ell, noise = theta
    rng = np.random.default_rng(2000 + T)
    x = np.cumsum(rng.uniform(0.3, 1.7, T))
    alpha = rng.normal(size=T)
    Kinv = rng.normal(size=(T, T))
    xl, al = x.astype(LD), alpha.astype(LD)
    t = al[:, None] * al[None, :] - Kinv.astype(LD)
    u = xl[:, None] / LD(ell) - xl[None, :] / LD(ell)
    d2 = u * u
    cr = LD(c) * np.exp(-LD(0.5) * d2)
    terms = [LD(0.5) * t * cr, LD(0.5) * t * cr * d2, LD(0.5) * LD(noise) * np.diag(t)]
    out = ops.lml_grad(dev(x), dev(alpha), dev(Kinv), c, ell, noise).cpu().numpy()
    for k in range(3):
        ref, scale = np.sum(terms[k]), np.sum(np.abs(terms[k]))
        err, bound = abs(float(LD(out[k]) - ref)), float((T * T / 256 + 32) * EPS * scale)
        print(f"lml_grad T={T} theta={theta} component {k}: error {err:.2e}  bound {bound:.2e}  ({err / max(float(scale), 1e-300) / EPS:.1f} eps)")
        assert err <= bound, (k, err, bound)


# ------------------------------------------------------------------------------------------------ a11 covariance
def warp_grids(T):
    rng = np.random.default_rng(3000 + T)
    up = 37.5 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 1.7, T - 1))])
    return {"from 37.5": up, "decreasing": np.ascontiguousarray(up[::-1]) - 50.0}


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("T", [1, 2, 17, 300])
def test_warp_cov(T, normalize):
    omega = 1.3
    for gname, x in warp_grids(T).items():
        for diag_add in (0.0, 0.25):
            rho = 0.2 if normalize else 0.2 * max(abs(x[-1] - x[0]), 1.0)      # a fifth of the grid either way
            K = ops.warp_cov(dev(x), rho, omega, diag_add, normalize=bool(normalize)).cpu().numpy()
            ref = orc.warp_rbf_cov(x, rho, omega, diag_add, jitter=0.0, normalize_x=bool(normalize))
            assert K.shape == (T, T) and np.allclose(K, ref, rtol=1e-13, atol=1e-300), (gname, diag_add)
            assert np.all(np.diag(K) == omega * omega + diag_add), (gname, diag_add)
            if T > 2:
                assert np.min(K) < 0.1 * omega * omega         # the length-scale is short enough for the grid to matter


# ------------------------------------------------------------------------------------------------ a1 Gram matrix
@pytest.mark.parametrize("shape", [(1, 1), (1, 700), (700, 3), (257, 255)])
def test_gram_rbf(shape):
    nx, ny = shape
    rng = np.random.default_rng(4000 + nx)
    c, ell, noise = 341.0, 6.5, 0.9
    x = 12.0 + np.cumsum(rng.uniform(0.02, 0.1, nx))
    y = 12.0 + np.sort(rng.uniform(0.0, 0.06 * max(nx, ny), ny))
    K2 = ops.gram_rbf(dev(x), dev(y), c, ell).cpu().numpy()
    assert K2.shape == (nx, ny) and np.allclose(K2, orc.gram_rbf(x, y, c, ell), rtol=1e-13, atol=1e-300)
    K1 = ops.gram_rbf(dev(x), None, c, ell, noise).cpu().numpy()
    assert K1.shape == (nx, nx) and np.allclose(K1, orc.gram_rbf(x, None, c, ell, noise), rtol=1e-13, atol=1e-300)
    assert np.all(np.diag(K1) == c + noise)
    if nx > 1:
        assert np.min(K1) < 0.5 * c and np.array_equal(K1, K1.T)


def test_gram_rbf_status_codes():
    lib = _ffi.lib
    x = torch.arange(4, dtype=torch.float64, device="cuda")
    K = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    z = ctypes.c_void_p(0)
    assert lib.hgp_gram_rbf_f64(ptr(x), 4, z, 0, 1.0, 0.0, 0.0, ptr(K), z) == -1      # ell = 0
    assert lib.hgp_gram_rbf_f64(ptr(x), 0, z, 0, 1.0, 1.0, 0.0, ptr(K), z) == -1      # nx = 0
    assert lib.hgp_gram_rbf_f64(ptr(x), 0, ptr(x), 4, 1.0, 1.0, 0.0, ptr(K), z) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(K).all())
