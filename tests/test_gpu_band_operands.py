"""Operand addressing of the static band sweeps (band_sweeps, csrc/hgp_pairs.hip): the M' loads take a scalar base, the E reads
an immediate offset from one of two lane addresses 64 KiB apart.  The mask-driven kernel (HGP_PAIRS_GENERIC=1) is the second
implementation, untouched by that: info and logdet must agree with it bit for bit, quad to the 1e-12 the two kernels agree to
(the band kernel sums the right-hand side's updates once per block).

Shapes: N = 5 segments, K = 3 clusters of synthetic_workload.synthetic_batch (jittered unit grids, length-scale 1.2).
  T = 128 (NB = 8): E is 128 KiB, every column panel has blocks on both sides of the 64 KiB boundary; all 13 passes.
  T = 96  (NB = 6, eight waves): E is 72 KiB, the boundary falls inside the matrix.
  ragged rows on the T = 128 plan: the last column blocks are empty, the band kernel hands the segment over.
  K = 1 and K = 5: one wave busy / waves with unequal pair counts.
  Sigma_k = K~_k: see test_sigma_equal_to_the_basis_gram.
That no segment reaches the fall-back list is shown from the data: band_pattern() applies the kernel's own rule (csrc/hgp_pairs.hip,
PairsBand) to the grids.  At NB = 8 there is a second witness: only the band kernel defers the right-hand side's cross-row sums
(wave_factor<NB, 2, BAND || NB < 8>), so the quadratic forms of the two runs differ in their last bits somewhere, which they
cannot if the mask-driven kernel had scored the pairs both times.  Below NB = 8 both kernels defer: there quad agrees bit for bit."""
import functools

import numpy as np
import pytest
import torch

import synthetic_workload as synth
from oracle import hdpgpc_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import ops

PAIRS_CUT = 55.45177444479562    # csrc/hgp_internal.hpp: 80 ln 2
RT_PAIR = 1e-8                   # tests/test_gpu_parity.py: the per-pair gate against the oracle
N = 5


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def band_pattern(x, xb, ell, NB):
    """The kernel's test of one segment: E and K** block-tridiagonal, every live k-step one the static sweeps multiply."""
    TP = 16 * NB
    pad = np.arange(TP, dtype=np.float64) + 1.0
    xs = np.where(np.arange(TP) < x.size, np.resize(x, TP) / ell, 1e150 * pad)
    xbs = np.where(np.arange(TP) < xb.size, np.resize(xb, TP) / ell, -1e150 * pad)
    with np.errstate(over="ignore"):
        near = 0.5 * (xbs[:, None] - xs[None, :]) ** 2 < PAIRS_CUT          # [k, j]
        nk = 0.5 * (xs[:, None] - xs[None, :]) ** 2 < PAIRS_CUT
    Kt, s, J = np.meshgrid(np.arange(NB), np.arange(4), np.arange(NB), indexing="ij")
    alive = (Kt == J) | ((Kt == J - 1) & (s >= 1)) | ((Kt == J + 1) & (s <= 2))
    steps = near.reshape(NB, 4, 4, NB, 16).any(axis=(2, 4))                  # [Kt, s, J]
    blocks = near.reshape(NB, 16, NB, 16).any(axis=(1, 3))
    tiles = np.triu(nk.reshape(NB, 16, NB, 16).any(axis=(1, 3)))
    I2, J2 = np.meshgrid(np.arange(NB), np.arange(NB), indexing="ij")
    return (np.array_equal(blocks, np.abs(I2 - J2) <= 1) and not (steps & ~alive).any()
            and np.array_equal(tiles, (I2 <= J2) & (I2 >= J2 - 1)))


@functools.lru_cache(maxsize=None)
def batch(T, K):
    return synth.synthetic_batch(N, K, T, seed=400 + T + K)


def both_kernels(plan, x, y, monkeypatch, **kw):
    monkeypatch.delenv("HGP_PAIRS_GENERIC", raising=False)
    band = plan.loglik(x, y, **kw)
    monkeypatch.setenv("HGP_PAIRS_GENERIC", "1")
    gen = plan.loglik(x, y, **kw)
    monkeypatch.delenv("HGP_PAIRS_GENERIC", raising=False)
    return band, gen


def check_against_generic(band, gen, T=128):
    (q1, l1, i1), (q0, l0, i0) = band, gen
    assert int(i1.abs().max()) == 0 and int(i0.abs().max()) == 0
    assert torch.equal(i0, i1) and torch.equal(l0, l1)
    dq = float(((q0 - q1).abs() / q0.abs()).max())
    print(f"quad, band against generic: max rel diff {dq:.3e}")
    assert dq <= 1e-12
    if T > 96:
        assert not torch.equal(q0, q1), "both runs gave the generic kernel's bits: the band kernel scored nothing"
    else:
        assert torch.equal(q0, q1)


@pytest.mark.parametrize("T, K", [(128, 3), (96, 3), (128, 1), (128, 5)])
def test_band_kernel_equals_the_generic_one(T, K, monkeypatch):
    b = batch(T, K)
    for n in range(N):
        assert band_pattern(b["x"][n], b["xb"], 1.2, T // 16), f"segment {n} is not the band kernel's pattern"
    plan = ops.PairsPlan(T, T, b["theta"]).update(dev(b["xb"]), dev(b["mean"]), dev(b["Sigma"]))
    assert not plan.solve_based().any()
    band, gen = both_kernels(plan, dev(b["x"]), dev(b["y"]), monkeypatch)
    check_against_generic(band, gen, T)
    _, q_ref, ld_ref = orc.loglik_pairs(b["x"][:2], b["y"][:2], b["xb"], b["theta"], b["mean"], b["Sigma"])
    assert np.abs(band[0][:2].cpu().numpy() / q_ref - 1.0).max() < RT_PAIR
    assert np.abs(band[1][:2].cpu().numpy() / ld_ref - 1.0).max() < RT_PAIR


def test_ragged_rows_on_the_128_plan(monkeypatch):
    """Rows shorter than 113 points leave the last column block(s) of E empty: not the static pattern, the band kernel hands
    them to the generic one; rows of 113 .. 128 points stay.  Every row has the bits of the rectangular call of its length."""
    T, K = 128, 3
    b = batch(T, K)
    lens = np.array([128, 100, 113, 64, 127], dtype=np.int32)
    stay = [band_pattern(b["x"][n, :L], b["xb"], 1.2, 8) for n, L in enumerate(lens)]
    assert stay == [True, False, True, False, True]
    x, y = b["x"].copy(), b["y"].copy()
    for n, L in enumerate(lens):
        x[n, L:] = np.nan
        y[n, L:] = np.nan
    plan = ops.PairsPlan(T, T, b["theta"]).update(dev(b["xb"]), dev(b["mean"]), dev(b["Sigma"]))
    band, gen = both_kernels(plan, dev(x), dev(y), monkeypatch, lengths=lens)
    check_against_generic(band, gen)
    sc, isc = plan.score(dev(x), dev(y), lengths=lens)
    for n, L in enumerate(lens):
        xr, yr = dev(b["x"][n:n + 1, :L]), dev(b["y"][n:n + 1, :L])
        q, ld, info = plan.loglik(xr, yr)
        assert torch.equal(q[0], band[0][n]) and torch.equal(ld[0], band[1][n]) and torch.equal(info[0], band[2][n])
        s, _ = plan.score(xr, yr)
        assert torch.equal(s[0], sc[n])
    assert int(isc.abs().max()) == 0


def test_sigma_equal_to_the_basis_gram(monkeypatch):
    """Sigma_k = K~_k makes M' = K~^-1 Sigma K~^-1 - K~^-1 vanish: cov is K** plus the regularisation, and every MFMA of sweep 2 -
    the first one into a tile above all - adds (rounding-level) zeros.  K~ = c R + jitter I has a constant diagonal, though, and a
    Sigma with a constant diagonal takes the reference's short cut cov = mean(diag Sigma) I (GPI.py:497), which never reaches the
    sweeps.  So Sigma = K~ + diag(w) with w alternating +-1e-4 c: just past the short cut's tolerance of 1e-5 relative, M' =
    K~^-1 diag(w) K~^-1.  quad against the NumPy fp64 solve of that banded matrix (the oracle's explicit formula) at the per-pair
    tolerance of tests/test_gpu_parity.py."""
    T, K = 128, 3
    b = batch(T, K)
    Sigma = np.empty_like(b["Sigma"])
    for k in range(K):
        c, ell, _ = b["theta"][k]
        R = orc.gram_rbf(b["xb"], b["xb"], c, ell)
        w = 1e-4 * c * np.where(np.arange(T) % 2 == 0, 1.0, -1.0)
        jit = 1e-4 * c / (1.0 - 1e-4)                                       # jitter = 1e-4 mean(diag Sigma) (GPI.py:488), mean(w) = 0
        Sigma[k] = 0.5 * (R + R.T) + jit * np.eye(T) + np.diag(w)
    plan = ops.PairsPlan(T, T, b["theta"]).update(dev(b["xb"]), dev(b["mean"]), dev(Sigma))
    assert not plan.solve_based().any()
    band, gen = both_kernels(plan, dev(b["x"]), dev(b["y"]), monkeypatch)
    check_against_generic(band, gen)
    _, q_ref, ld_ref = orc.loglik_pairs(b["x"], b["y"], b["xb"], b["theta"], b["mean"], Sigma)
    eq = np.abs(band[0].cpu().numpy() / q_ref - 1.0).max()
    el = np.abs(band[1].cpu().numpy() / ld_ref - 1.0).max()
    print(f"Sigma = K~ + diag(w): quad rel err {eq:.3e}, logdet rel err {el:.3e}")
    assert eq < RT_PAIR and el < RT_PAIR
