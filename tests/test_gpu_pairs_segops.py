"""The segment-operator store (hgp_loglik_pairs_segops_f64, include/hdpgpc_hip_segops.h): the band pair kernel with its per-segment
prologue - E blocks, K** tiles, band decision - built once by k_segops and streamed from a caller-owned buffer afterwards.

The contract is that the store changes WHEN things are computed and nothing else: quad, logdet and info of the new entry are,
BIT FOR BIT, those of hgp_loglik_pairs_f64 / hgp_loglik_pairs_ragged_f64 of the same build on the same inputs - whatever the
store held before the call (zeros, this batch, this batch before an input changed, another plan's records).  Every case below calls
both entries directly and compares the three outputs on the bits; outputs start as NaN / 7 on both sides, so an element that
neither entry writes compares equal and one that only one writes does not.

Sizes: N <= 8 segments, K = 3 clusters, T = Ts = 90 (padded 96, the eight-wave band kernel) and T = Ts = 128 (padded 128).  The
flag words of the records are read back where a case depends on which kernel took a segment (3 = valid + band, 1 = valid, not
band: the mask-driven kernel, 5 = valid + bad length)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import hdpgpc_oracle as orc

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, ops

DEV = "cuda"
SIZES = (90, 128)
K = 3
VALID, BAND, BADLEN = 1, 2, 4


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)


def idev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32, device=DEV)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def make_plan(T, ells=(1.2, 1.2, 1.2), seed=3, N=8):
    b = orc.synthetic_batch(N, K, T, seed=seed)
    theta = b["theta"].copy()
    theta[:, 1] = ells
    plan = ops.PairsPlan(T, T, theta, device=DEV).update(dev(b["xb"]), dev(b["mean"]), dev(b["Sigma"]))
    return plan, b


def outputs(N, sel):
    shape = (N,) if sel is not None else (N, K)
    return (torch.full(shape, float("nan"), dtype=torch.float64, device=DEV),
            torch.full(shape, float("nan"), dtype=torch.float64, device=DEV),
            torch.full(shape, 7, dtype=torch.int32, device=DEV))


def old_entry(plan, x, y, lengths=None, sel=None, first_noise=None):
    N, ld = x.shape
    q, l, i = outputs(N, sel)
    if lengths is None:
        rc = _ffi.lib.hgp_loglik_pairs_f64(plan._h, _ptr(x), _ptr(y), N, ld, _ptr(first_noise), _ptr(sel), _ptr(q), _ptr(l), _ptr(i), None)
    else:
        rc = _ffi.lib.hgp_loglik_pairs_ragged_f64(plan._h, _ptr(x), _ptr(y), N, ld, _ptr(lengths), _ptr(first_noise), _ptr(sel),
                                                  _ptr(q), _ptr(l), _ptr(i), None)
    assert rc == 0
    return q, l, i


def new_entry(plan, store, x, y, lengths=None, sel=None, first_noise=None):
    N, ld = x.shape
    q, l, i = outputs(N, sel)
    rc = _ffi.lib.hgp_loglik_pairs_segops_f64(plan._h, _ptr(store), store.numel(), _ptr(x), _ptr(y), N, ld, _ptr(lengths),
                                              _ptr(first_noise), _ptr(sel), _ptr(q), _ptr(l), _ptr(i), None)
    assert rc == 0
    return q, l, i


def new_store(plan, N, ld):
    need = _ffi.lib.hgp_pairs_segops_bytes(plan._h, N, ld)
    assert need > 0
    return torch.zeros(need, dtype=torch.uint8, device=DEV)


def flags(store, T, N, groups=1):
    """Flag word of every record, [groups, N] (layout of csrc/hgp_segops.hpp: tiles, two keys of TP doubles, then the words)."""
    nb = 6 if T <= 96 else 8
    rec = store.numel() // (groups * N)
    assert rec == 8 * ((5 * nb - 3) * 256 + 2 * 16 * nb + 16)
    words = store.view(torch.int32).view(groups * N, rec // 4)[:, 2 * ((5 * nb - 3) * 256 + 2 * 16 * nb)]
    return words.view(groups, N).cpu().numpy()


def same_bits(a, b):
    for u, v in zip(a, b):
        if u.dtype == torch.float64:
            u, v = u.contiguous().view(torch.int64), v.contiguous().view(torch.int64)
        if u.shape != v.shape or not torch.equal(u, v):
            return False
    return True


def check(plan, store, x, y, **kw):
    """One call of each entry on the same inputs; the new one against whatever `store` holds."""
    torch.cuda.synchronize()
    ref = old_entry(plan, x, y, **kw)
    got = new_entry(plan, store, x, y, **kw)
    torch.cuda.synchronize()
    assert same_bits(got, ref)
    return ref


@pytest.mark.parametrize("T", SIZES)
def test_cold_warm_and_changed_inputs(T):
    """Cases 1-5: cold store, the same call again, one grid point changed in place, a shifted basis grid, y alone changed."""
    plan, b = make_plan(T)
    x, y = dev(b["x"]), dev(b["y"])
    store = new_store(plan, 8, T)
    r0 = check(plan, store, x, y)                      # 1: cold
    assert int(r0[2].abs().max()) == 0 and bool(torch.isfinite(r0[0]).all())
    assert (flags(store, T, 8) == VALID | BAND).all()
    before = store.clone()
    check(plan, store, x, y)                           # 2: warm; nothing of the store is rewritten
    assert torch.equal(store, before)
    x[2, 17] = 17.125                                  # 3: same address, one point
    r3 = check(plan, store, x, y)
    assert not torch.equal(r3[0][2], r0[0][2]) and same_bits((r3[0][3:],), (r0[0][3:],))
    assert not torch.equal(store, before)
    plan.update(dev(b["xb"] + 0.05), dev(b["mean"]), dev(b["Sigma"]))   # 4: the basis grid moved
    r4 = check(plan, store, x, y)
    assert not torch.equal(r4[0], r3[0])
    check(plan, store, x, y)
    y2 = dev(b["y"][::-1])                             # 5: y alone
    before = store.clone()
    r5 = check(plan, store, x, y2)
    assert torch.equal(store, before) and not torch.equal(r5[0], r4[0])
    plan.close()


@pytest.mark.parametrize("T", SIZES)
def test_band_generic_and_nan_segments_in_one_batch(T):
    """Case 6: band segments next to one jittered by +-0.45 (a k-step outside the static pattern: mask-driven kernel) and one whose
    grid holds a NaN (its key compares equal to itself on the bits; whichever kernel the old entry gives it to, the new one does too)."""
    plan, b = make_plan(T, N=6)
    xh = b["x"].copy()
    xh[1] = b["xb"] - 0.45 * (-1.0) ** np.arange(T)   # |xb[j - 13] - x[j]| = 12.55 for even j: inside the cut-off radius 12.64
    xh[4, T // 2] = np.nan
    x, y = dev(xh), dev(b["y"])
    store = new_store(plan, 6, T)
    for _ in range(2):   # cold, warm
        check(plan, store, x, y)
        f = flags(store, T, 6)[0].tolist()
        assert f[:4] + f[5:] == [3, 1, 3, 3, 3] and f[4] in (1, 3)
    before = store.clone()
    check(plan, store, x, y)
    assert torch.equal(store, before)   # the NaN row was not rebuilt
    plan.close()


@pytest.mark.parametrize("T", SIZES)
def test_ragged_lengths_and_a_length_that_changes(T):
    """Case 7: lengths including 1 and ld, one outside [1, ld]; then one length changed between calls."""
    plan, b = make_plan(T)
    xh = b["x"].copy()
    lens = np.array([1, T, T - 1, 45, 0, 17, T, 64], dtype=np.int32)
    for n, L in enumerate(lens):
        xh[n, L:] = np.nan   # never read
    x, y = dev(xh), dev(b["y"])
    store = new_store(plan, 8, T)
    lengths = idev(lens)
    for _ in range(2):
        r = check(plan, store, x, y, lengths=lengths)
        assert flags(store, T, 8)[0, 4] == VALID | BADLEN and int(r[2][4].min()) == -1
        assert flags(store, T, 8)[0, 1] == VALID | BAND
    x[3, 45:50] = dev(b["x"][3, 45:50])
    lengths[3] = 50
    lengths[4] = 30
    x[4, :30] = dev(b["x"][4, :30])
    check(plan, store, x, y, lengths=lengths)
    check(plan, store, x, y, lengths=lengths)
    check(plan, store, x, y)   # the same store, now rectangular: NaN tails are read by both entries alike
    plan.close()


@pytest.mark.parametrize("T", SIZES)
def test_sel_first_noise_and_two_length_scale_groups(T):
    """Cases 8 and 9: per-segment selection (with first_noise), and a plan with two length-scale groups, both of the band
    pattern on a unit-spaced grid."""
    plan, b = make_plan(T, ells=(1.2, 1.0, 1.2))
    x, y = dev(b["x"]), dev(b["y"])
    assert _ffi.lib.hgp_pairs_segops_bytes(plan._h, 8, T) == 2 * new_store(make_plan_bytes_probe(T), 8, T).numel()
    store = new_store(plan, 8, T)
    for _ in range(2):
        check(plan, store, x, y)
        assert (flags(store, T, 8, groups=2) == VALID | BAND).all()
    sel = idev(np.arange(8) % K)
    fn = dev(np.linspace(0.0, 0.5, 8))
    check(plan, store, x, y, sel=sel, first_noise=fn)
    fresh = torch.zeros_like(store)
    check(plan, fresh, x, y, sel=sel)
    check(plan, fresh, x, y, first_noise=dev(np.linspace(0.0, 0.5, 8 * K).reshape(8, K)))
    plan.close()


_PROBES = {}


def make_plan_bytes_probe(T):
    """A one-group plan of the size, kept for the byte counts."""
    if T not in _PROBES:
        _PROBES[T] = make_plan(T)[0]
    return _PROBES[T]


@pytest.mark.parametrize("T", SIZES)
def test_store_filled_by_another_plan(T):
    """Case 10: a store that holds valid records of the same segments for another length-scale."""
    other, b = make_plan(T, ells=(1.0, 1.0, 1.0))
    plan, _ = make_plan(T)
    x, y = dev(b["x"]), dev(b["y"])
    store = new_store(other, 8, T)
    check(other, store, x, y)
    assert (flags(store, T, 8) == VALID | BAND).all()
    filled = store.clone()
    check(plan, store, x, y)
    assert not torch.equal(store, filled)
    check(plan, store, x, y)
    other.close()
    plan.close()


@pytest.mark.parametrize("T", SIZES)
def test_pairs_plan_keeps_one_store_and_follows_n(T):
    """Case 11: PairsPlan.loglik owns the store; N changes between calls, and a batch over the byte cap takes the old entry."""
    plan, b = make_plan(T)
    x, y = dev(b["x"]), dev(b["y"])
    for N in (8, 8, 5, 8):
        got = plan.loglik(x[:N], y[:N])
        assert plan._segops is not None and plan._segops_key[0] == N
        assert same_bits(got, old_entry(plan, x[:N].contiguous(), y[:N].contiguous()))
    lens = idev([T, 1, 33, T, 2])
    assert same_bits(plan.loglik(x[:5], y[:5], lengths=lens), old_entry(plan, x[:5].contiguous(), y[:5].contiguous(), lengths=lens))
    held = plan._segops
    plan.SEGOPS_MAX_BYTES = 1024   # instance attribute: this plan alone
    assert same_bits(plan.loglik(x, y), old_entry(plan, x, y)) and plan._segops is held
    plan.close()


FB_CAP = 65536   # PAIRS_FB_CAP of csrc/hgp_internal.hpp: segments per slice of a call (capacity of the fall-back list)


def test_streamed_route_beyond_the_fall_back_list():
    """PAIRS_FB_CAP + 5 segments through the store (T = 90, ld = 96, two clusters of one length-scale, sorted jittered unit grids,
    lengths cycling through 40 values in 60 ... 96 - shorter than 81 is not the band pattern): the second slice starts at segment
    65 536 and must use ITS rows, lengths, selection, first_noise, outputs and records of the store.  The rows around the boundary
    have reversed grids and go through the fall-back list on both sides of it.  Rows on both sides against the same rows scored
    alone, through a store of their own and by the in-kernel route, on the bits; ragged, with sel and first_noise, and rectangular."""
    T, ld, N, K2, base = 90, 96, FB_CAP + 5, 2, 40
    rng = np.random.default_rng(11)
    sb = orc.synthetic_batch(4, K2, T, seed=2)
    theta = sb["theta"].copy()
    theta[:, 1] = 1.2
    lens_b = np.array([60 + (7 * n) % 37 for n in range(base)], dtype=np.int32)
    assert lens_b.min() == 60 and lens_b.max() == ld and FB_CAP % base != 0   # out of step with the slice: an unshifted pointer shows
    Xb = np.arange(ld) + rng.uniform(-0.3, 0.3, (base, ld))
    Yb = np.stack([np.interp(Xb[n], sb["xb"], sb["mean"][n % K2]) for n in range(base)]) + rng.normal(0.0, 3.0, (base, ld))
    reps = N // base + 1
    Xh, Yh = np.tile(Xb, (reps, 1))[:N], np.tile(Yb, (reps, 1))[:N]
    listed = [FB_CAP - 1, FB_CAP, FB_CAP + 1]
    Xh[listed], Yh[listed] = Xh[listed, ::-1], Yh[listed, ::-1]
    X, Y, lens = dev(Xh), dev(Yh), idev(np.tile(lens_b, reps)[:N])
    sel, fn = idev(np.arange(N) % K2), dev(np.linspace(0.0, 0.5, N))
    plan = ops.PairsPlan(T, ld, theta, device=DEV).update(dev(sb["xb"]), dev(sb["mean"]), dev(sb["Sigma"]))
    need = _ffi.lib.hgp_pairs_segops_bytes(plan._h, N, ld)
    assert need == N * 56960 > 1 << 31   # 3.7 GB

    def cut(t, lo, hi):
        return None if t is None else t[lo:hi].contiguous()

    variants = (dict(lengths=lens), dict(lengths=lens, sel=sel, first_noise=fn), dict())
    plan.SEGOPS_MAX_BYTES = 1 << 33   # instance attribute: this plan alone
    whole = []
    for kw in variants:   # every whole batch first: they share the one large store
        r = plan.loglik(X, Y, **kw)
        assert plan._segops.numel() == need and plan._segops_key[0] == N
        assert int(r[2].abs().max()) == 0
        assert same_bits(plan.loglik(X, Y, **kw), r)   # warm
        assert (flags(plan._segops, T, N)[0, listed] == VALID).all()   # not the band pattern: the fall-back list
        whole.append(r)
    for kw, r in zip(variants, whole):
        for lo, hi in ((0, 12), (FB_CAP - 7, FB_CAP), (FB_CAP, N), (FB_CAP - 3, FB_CAP + 3)):
            kw_w = {k: cut(v, lo, hi) for k, v in kw.items()}
            want = tuple(t[lo:hi] for t in r)
            plan.SEGOPS_MAX_BYTES = 1 << 33   # alone through a store
            got = plan.loglik(cut(X, lo, hi), cut(Y, lo, hi), **kw_w)
            assert plan._segops_key[0] == hi - lo and same_bits(got, want), (sorted(kw), lo, hi)
            plan.SEGOPS_MAX_BYTES = 0         # alone, the prologue built in the kernel
            assert same_bits(plan.loglik(cut(X, lo, hi), cut(Y, lo, hi), **kw_w), want), (sorted(kw), lo, hi)
    plan.close()


def test_sizes_and_argument_errors():
    """hgp_pairs_segops_bytes is 0 where no band kernel serves the plan and the record size times groups times N where one does;
    a store that is too small, missing or misaligned is -1 and nothing is launched."""
    lib = _ffi.lib
    for T, rec in ((90, 8 * (27 * 256 + 2 * 96 + 16)), (128, 8 * (37 * 256 + 2 * 128 + 16))):
        p = make_plan_bytes_probe(T)
        assert lib.hgp_pairs_segops_bytes(p._h, 5, T) == 5 * rec
        assert lib.hgp_pairs_segops_bytes(p._h, 5, 16 * ((T + 15) // 16) + 1) == 0
        assert lib.hgp_pairs_segops_bytes(p._h, 0, T) == lib.hgp_pairs_segops_bytes(p._h, 5, 0) == 0
    for T in (40, 64, 150):
        p, b = make_plan(T, N=2)
        assert lib.hgp_pairs_segops_bytes(p._h, 2, T) == 0
        x, y = dev(b["x"]), dev(b["y"])
        q, l, i = outputs(2, None)
        assert lib.hgp_loglik_pairs_segops_f64(p._h, None, 0, _ptr(x), _ptr(y), 2, T, None, None, None, _ptr(q), _ptr(l), _ptr(i), None) == 0
        torch.cuda.synchronize()
        assert same_bits((q, l, i), old_entry(p, x, y))   # forwarded
        p.close()
    p, b = make_plan(128, N=2)
    x, y = dev(b["x"]), dev(b["y"])
    q, l, i = outputs(2, None)
    store = new_store(p, 2, 128)
    call = lambda s, nbytes, off=0: lib.hgp_loglik_pairs_segops_f64(  # noqa: E731
        p._h, ctypes.c_void_p(s.data_ptr() + off) if s is not None else None, nbytes, _ptr(x), _ptr(y), 2, 128, None, None, None,
        _ptr(q), _ptr(l), _ptr(i), None)
    assert call(store, store.numel() - 1) == -1 and call(None, store.numel()) == -1 and call(store, store.numel(), off=8) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(q).all()) and int(store.max()) == 0
    p.close()
