"""The element-wise glue of the member step through the C-ABI, against tests/chain_glue_ref.py (pinned to the reference by
tests/test_chain_glue_ref.py): hgp_lds_chain_gather2_batched_f64, hgp_lds_chain_finish2_batched_f64, hgp_copy_list_f64.

Every buffer a kernel may touch is a slice of ONE float64 arena (or one int32 arena) with NaN (sentinel) words between the slices;
a launch is checked by comparing the WHOLE arena with the expected one bit for bit: what the kernel had to write, what it had to
leave (untouched stack rows, W / n0 / Nf / pos of a candidate step, the chains outside a sub-range) and every guard word between
the buffers.  Bit equality of the finish is derived, not measured: the kernel is compiled with fp contract(off), every operation
is one correctly rounded IEEE fp64 operation, and the order is the header's - which is what chain_glue_ref.finish_ref evaluates.
"""
import ctypes

import numpy as np
import pytest
import torch

import chain_glue_ref as cg

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi, member_step, ops

L = 5                   # rows of every stack
SENT = -7777            # guard word of the int32 arena
MATS, VECS = cg.STACKS[:6], cg.STACKS[6:]
INPUT_VECS, INPUT_MATS, INPUT_PAIRS = ("f_post", "f_sm_prev", "y"), ("c_post", "P_sm_prev"), ("part", "Snew")


class Layout:
    """Named slices of a float64 arena and of an int32 arena, with guard words before, between and behind them."""

    def __init__(self):
        self.slots, self.nf, self.ni = {}, 3, 3

    def f64(self, name, *shape, parity=None):
        if parity is not None and self.nf % 2 != parity:     # parity 0: 16-byte aligned (the arena itself is), 1: not
            self.nf += 1
        self.slots[name] = ("f", self.nf, shape)
        self.nf += int(np.prod(shape)) + 3

    def i32(self, name, n, align=1):
        self.ni += (-self.ni) % align
        self.slots[name] = ("i", self.ni, (n,))
        self.ni += n + 3

    def host(self):
        return np.full(self.nf, np.nan), np.full(self.ni, SENT, dtype=np.int32)

    def view(self, arenas, name):
        kind, off, shape = self.slots[name]
        return arenas[kind == "i"][off:off + int(np.prod(shape))].reshape(shape)

    def ptr(self, devs, name):
        kind, off, _ = self.slots[name]
        return devs[kind == "i"].data_ptr() + off * (4 if kind == "i" else 8)

    def names(self, prefix):
        return [n for n in self.slots if n.startswith(prefix + ".")]


def upload(H):
    return tuple(torch.from_numpy(a).cuda() for a in H)


def download(D):
    torch.cuda.synchronize()
    return tuple(d.cpu().numpy() for d in D)


def assert_same_bits(lay, got, exp):
    """The whole arenas, bit for bit; on a mismatch the slices (or the guard words) that differ are named."""
    gf, ef = got[0].view(np.uint64), exp[0].view(np.uint64)
    if np.array_equal(gf, ef) and np.array_equal(got[1], exp[1]):
        return
    wrong, covered = [], [np.zeros(got[0].size, dtype=bool), np.zeros(got[1].size, dtype=bool)]
    for name, (kind, off, shape) in lay.slots.items():
        n, i = int(np.prod(shape)), int(kind == "i")
        covered[i][off:off + n] = True
        g, e = (got[i], exp[i]) if i else (gf, ef)
        if not np.array_equal(g[off:off + n], e[off:off + n]):
            wrong.append(f"{name} ({int(np.sum(g[off:off + n] != e[off:off + n]))} of {n} words)")
    if np.any((gf != ef) & ~covered[0]) or np.any((got[1] != exp[1]) & ~covered[1]):
        wrong.append("guard words between the buffers")
    raise AssertionError("device state differs from the reference in: " + ", ".join(wrong))


def add_chain(lay, c, T):
    for k in MATS:
        lay.f64(f"{c}.{k}", L, T, T)
    for k in VECS:
        lay.f64(f"{c}.{k}", L, T)
    lay.f64(f"{c}.W", 3, 2, T, T)
    lay.f64(f"{c}.n0", 1)
    lay.f64(f"{c}.Nf", 1)
    for k in INPUT_VECS:
        lay.f64(f"{c}.{k}", T)
    for k in INPUT_MATS:
        lay.f64(f"{c}.{k}", T, T)
    for k in INPUT_PAIRS:
        lay.f64(f"{c}.{k}", 2, T, T)
    lay.i32(f"{c}.info1", 4)
    lay.i32(f"{c}.info2", 2)
    lay.i32(f"{c}.bad", 2)
    lay.i32(f"{c}.sync", 1)
    lay.i32(f"{c}.pos", 2, align=2)                          # one int64


def fill_chain(lay, H, c, rng):
    """Distinct random numbers in every double of the chain."""
    for name in lay.names(c):
        if lay.slots[name][0] == "f":
            v = lay.view(H, name)
            v[...] = rng.normal(size=v.shape)


def set_words(lay, H, c, pos, n0, Nf, info1=(0, 0, 0, 0), info2=(0, 0), bad=(0, 0)):
    lay.view(H, f"{c}.n0")[0], lay.view(H, f"{c}.Nf")[0] = n0, Nf
    lay.view(H, f"{c}.info1")[:], lay.view(H, f"{c}.info2")[:], lay.view(H, f"{c}.bad")[:] = info1, info2, bad
    lay.view(H, f"{c}.sync")[0] = 0
    lay.view(H, f"{c}.pos").view(np.int64)[0] = pos


def state_of(lay, H, c):
    s = {k: lay.view(H, f"{c}.{k}").copy() for k in cg.STACKS + ("W",)}
    s.update(n0=float(lay.view(H, f"{c}.n0")[0]), Nf=float(lay.view(H, f"{c}.Nf")[0]),
             pos=int(lay.view(H, f"{c}.pos").view(np.int64)[0]), bad_count=lay.view(H, f"{c}.bad").copy())
    inputs = {k: lay.view(H, f"{c}.{k}").copy() for k in INPUT_VECS + INPUT_MATS + INPUT_PAIRS}
    return s, inputs, lay.view(H, f"{c}.info1").tolist(), lay.view(H, f"{c}.info2").tolist()


def store_state(lay, E, c, s):
    for k in cg.STACKS + ("W",):
        lay.view(E, f"{c}.{k}")[...] = s[k]
    set_words(lay, E, c, s["pos"], s["n0"], s["Nf"], lay.view(E, f"{c}.info1"), lay.view(E, f"{c}.info2"), s["bad_count"])


def expect_finish(lay, H, chains, flags, times=1):
    """The arenas after `times` finish launches over `chains` (their flags in `flags`)."""
    E = (H[0].copy(), H[1].copy())
    for c, fl in zip(chains, flags):
        for _ in range(times):
            s, inputs, i1, i2 = state_of(lay, E, c)
            store_state(lay, E, c, cg.finish_ref(s, inputs, i1, i2, fl))
    return E


def finish_desc(lay, D, c, T, flags):
    f = _ffi.ChainFinishDesc()
    p = lambda k: lay.ptr(D, f"{c}.{k}")                     # noqa: E731
    f.f_post, f.c_post, f.f_sm_prev, f.P_sm_prev, f.y = p("f_post"), p("c_post"), p("f_sm_prev"), p("P_sm_prev"), p("y")
    f.part, f.Snew, f.info1, f.info2 = p("part"), p("Snew"), p("info1"), p("info2")
    f.W, f.n0, f.Nf, f.bad_count = p("W"), p("n0"), p("Nf"), p("bad")
    f.stA, f.stG, f.stC, f.stS = p("A"), p("G"), p("C"), p("S")
    f.stF, f.stFsm, f.stP, f.stPsm = p("F"), p("Fsm"), p("P"), p("Psm")
    f.pos, f.sync, f.T, f.annealing = p("pos"), p("sync"), T, flags
    return f


def launch_finish(fdev, lo, hi, T):
    base = ctypes.c_void_p(fdev.data_ptr() + lo * ctypes.sizeof(_ffi.ChainFinishDesc))
    return _ffi.lib.hgp_lds_chain_finish2_batched_f64(base, hi - lo, T, ops._stream())


# flags 0..7 on a good step; each of the four status words that make a step keep its distributions, alone (annealed, candidate,
# no-smoother variants among them); each of the two words that only latch bad_count[1], alone
FINISH_CASES = ([(fl, (0, 0, 0, 0), (0, 0)) for fl in range(8)] +
                [(1, (0, 0, 4, 0), (0, 0)), (3, (0, 0, 0, 1), (0, 0)), (4, (0, 0, 0, 0), (9, 0)), (0, (0, 0, 0, 0), (0, 2)),
                 (0, (6, 0, 0, 0), (0, 0)), (1, (0, 1, 0, 0), (0, 0))])


@pytest.mark.parametrize("T", [1, 17, 90, 91, 144, 256])
def test_finish_every_flag_and_status_word(T):
    """T = 1: one block; 17: 3 blocks; 90: exactly 64 blocks in one pass; 91: the first size whose grid-stride loop makes a second
    pass; 144: 3 passes; 256: 8 passes.  The last-block election (sync) has to count every block of every pass once."""
    lay = Layout()
    add_chain(lay, "c", T)
    H = lay.host()
    fill_chain(lay, H, "c", np.random.default_rng(T))
    D = upload(H)
    for n, (flags, info1, info2) in enumerate(FINISH_CASES):
        set_words(lay, H, "c", pos=(0, 2)[n % 2], n0=5.0 + n, Nf=2.0 + n, info1=info1, info2=info2, bad=(n % 3, 0))
        for d, h in zip(D, H):
            d.copy_(torch.from_numpy(h))
        fdev = member_step.upload_descs([finish_desc(lay, D, "c", T, flags)], "cuda")
        assert launch_finish(fdev, 0, 1, T) == 0
        E = expect_finish(lay, H, ["c"], [flags])
        bad = any(info1[2:]) or any(info2)
        assert lay.view(E, "c.bad").tolist() == [n % 3 + int(bad), (0, 2)[n % 2] + 1 if any(info1[:2]) else 0]
        assert lay.view(E, "c.sync")[0] == 0
        assert_same_bits(lay, download(D), E)


@pytest.mark.parametrize("T", [17, 91])
def test_finish_twice_without_the_host(T):
    """Two launches on the same descriptors: the second appends at pos + 2 with n0 + 2 - pos, n0, Nf are read from the device and
    the inter-block counter was re-armed.  Chain b fails both times: counted twice, distributions kept, and the step latched in
    bad_count[1] by the first launch is not overwritten by the second."""
    lay = Layout()
    add_chain(lay, "a", T)
    add_chain(lay, "b", T)
    H = lay.host()
    rng = np.random.default_rng(50 + T)
    fill_chain(lay, H, "a", rng)
    fill_chain(lay, H, "b", rng)
    set_words(lay, H, "a", pos=2, n0=6.0, Nf=3.0)
    set_words(lay, H, "b", pos=0, n0=7.0, Nf=1.0, info1=(0, 3, 0, 0), info2=(0, 2))
    D = upload(H)
    fdev = member_step.upload_descs([finish_desc(lay, D, "a", T, 1), finish_desc(lay, D, "b", T, 1)], "cuda")
    assert launch_finish(fdev, 0, 2, T) == 0
    assert launch_finish(fdev, 0, 2, T) == 0
    E = expect_finish(lay, H, ["a", "b"], [1, 1], times=2)
    sa, sb = state_of(lay, E, "a")[0], state_of(lay, E, "b")[0]
    assert (sa["pos"], sa["n0"], sa["Nf"], sa["bad_count"].tolist()) == (4, 8.0, 5.0, [0, 0])
    assert (sb["pos"], sb["n0"], sb["Nf"], sb["bad_count"].tolist()) == (2, 7.0, 3.0, [2, 1])
    assert_same_bits(lay, download(D), E)


@pytest.mark.parametrize("T", [17, 91])
def test_finish_batch_and_sub_range(T):
    """Five chains in one launch, each with its own position, counters, flags and status words; then chains [1, 4) of the same
    descriptor array (base pointer offset, as member_step.member_step launches a slice): chains 0 and 4 stay as they were."""
    lay = Layout()
    chains = [f"c{i}" for i in range(5)]
    flags = [1, 0, 5, 3, 7]
    for c in chains:
        add_chain(lay, c, T)
    H = lay.host()
    rng = np.random.default_rng(80 + T)
    info1 = [(0, 0, 0, 0), (0, 0, 0, 0), (0, 0, 2, 0), (1, 0, 0, 0), (0, 0, 0, 0)]
    for i, c in enumerate(chains):
        fill_chain(lay, H, c, rng)
        set_words(lay, H, c, pos=(0, 2, 1, 3, 2)[i], n0=4.0 + i, Nf=1.0 + 2 * i, info1=info1[i], info2=(0, int(i == 4)), bad=(i, 0))
    for lo, hi in ((0, 5), (1, 4)):
        D = upload(H)
        fdev = member_step.upload_descs([finish_desc(lay, D, c, T, fl) for c, fl in zip(chains, flags)], "cuda")
        assert launch_finish(fdev, lo, hi, T) == 0
        assert_same_bits(lay, download(D), expect_finish(lay, H, chains[lo:hi], flags[lo:hi]))


def test_finish_and_gather_argument_checks():
    T = 8
    lay = Layout()
    add_chain(lay, "c", T)
    H = lay.host()
    fill_chain(lay, H, "c", np.random.default_rng(1))
    set_words(lay, H, "c", pos=1, n0=5.0, Nf=2.0)
    D = upload(H)
    fdev = member_step.upload_descs([finish_desc(lay, D, "c", T, 1)], "cuda")
    lib, st = _ffi.lib, ops._stream()
    for fn in (lib.hgp_lds_chain_finish2_batched_f64, lib.hgp_lds_chain_gather2_batched_f64):
        assert fn(ctypes.c_void_p(fdev.data_ptr()), 0, T, st) == 0           # no chains: nothing to do
        assert fn(None, 1, T, st) == -1
        assert fn(ctypes.c_void_p(fdev.data_ptr()), 1, 0, st) == -1
        assert fn(ctypes.c_void_p(fdev.data_ptr()), 1, -3, st) == -1
        assert fn(ctypes.c_void_p(fdev.data_ptr()), -1, T, st) == -1
    assert_same_bits(lay, download(D), H)


# ------------------------------------------------------------------------------------------------------------------ gather
def add_gather(lay, c, T):
    lay.f64(f"{c}.W", 3, 2, T, T)
    lay.f64(f"{c}.Y", 3, T)
    lay.f64(f"{c}.out", 6 * T * T + 2 * T)
    lay.f64(f"{c}.y_out", T)
    lay.f64(f"{c}.Rp", 2, T, T)
    lay.i32(f"{c}.pos", 2, align=2)


def gather_desc(lay, D, c, stacks, T, y_mode, pos):
    g = _ffi.ChainGatherDesc()
    for i, k in enumerate(cg.STACKS):
        g.st[i] = lay.ptr(D, f"{stacks}.{k}")
    g.pos, g.out, g.y_out, g.W, g.Rp = (lay.ptr(D, f"{c}.{k}") for k in ("pos", "out", "y_out", "W", "Rp"))
    g.Y = None if y_mode == "none" else lay.ptr(D, f"{c}.Y")
    g.y_row0 = y_row0_of(y_mode, pos)
    g.T = T
    return g


def y_row0_of(y_mode, pos):
    return pos - 1 if y_mode == "run" else -1       # "run": Y holds the run's observations from row y_row0 on; else Y is the observation


GATHER_MODES = [("run", 3), ("own", 0), ("none", 3), ("run", 0), ("own", 3), ("none", 0)]


@pytest.mark.parametrize("n_chains", [1, 9])
@pytest.mark.parametrize("T", [1, 17, 90, 128, 256])
def test_gather_rows_observation_and_jittered_right_covariances(T, n_chains):
    """The eight stacks at pos in {0, 3}, y_out from row pos - y_row0 (row 1 at pos = 3, y_row0 = 2), from row 0 (y_row0 < 0) and not
    at all (Y == NULL: y_out stays NaN), Rp off the diagonal: bit for bit.  Rp on the diagonal: a sum of T non-negative terms in
    any order, one multiply, one add - |got - ref| <= T eps jitter + eps |ref| against the longdouble value.
    n_chains = 1: grid capped at 256 blocks; 9: at 64 (from 8 chains on)."""
    lay = Layout()
    for s in ("s0", "s1"):                           # two sets of stacks, shared by the chains of a launch (only read)
        for k in MATS:
            lay.f64(f"{s}.{k}", L, T, T)
        for k in VECS:
            lay.f64(f"{s}.{k}", L, T)
    chains = [f"c{i}" for i in range(n_chains)]
    for c in chains:
        add_gather(lay, c, T)
    H = lay.host()
    rng = np.random.default_rng(7 * T + n_chains)
    for s in ("s0", "s1"):
        fill_chain(lay, H, s, rng)
    for c in chains:
        for k in ("W", "Y"):
            v = lay.view(H, f"{c}.{k}")
            v[...] = rng.normal(size=v.shape)
    rounds = [GATHER_MODES] if n_chains > 1 else [[m] for m in GATHER_MODES]      # one chain: every mode in a launch of its own
    worst = 0.0
    for modes in rounds:
        for i, c in enumerate(chains):
            lay.view(H, f"{c}.pos").view(np.int64)[0] = modes[i % len(modes)][1]
        D = upload(H)
        descs = [gather_desc(lay, D, c, f"s{i % 2}", T, *modes[i % len(modes)]) for i, c in enumerate(chains)]
        gdev = member_step.upload_descs(descs, "cuda")
        assert _ffi.lib.hgp_lds_chain_gather2_batched_f64(ctypes.c_void_p(gdev.data_ptr()), n_chains, T, ops._stream()) == 0
        got = download(D)
        E = (H[0].copy(), H[1].copy())
        for i, c in enumerate(chains):
            y_mode, pos = modes[i % len(modes)]
            stacks = {k: lay.view(H, f"s{i % 2}.{k}") for k in cg.STACKS}
            W = lay.view(H, f"{c}.W")
            out, y_out, Rp, jit = cg.gather_ref(stacks, pos, W, None if y_mode == "none" else lay.view(H, f"{c}.Y"), y_row0_of(y_mode, pos))
            lay.view(E, f"{c}.out")[:] = out
            if y_out is not None:
                assert np.array_equal(y_out, lay.view(H, f"{c}.Y")[1 if (y_mode, pos) == ("run", 3) else 0])
                lay.view(E, f"{c}.y_out")[:] = y_out
            gRp, eRp = lay.view(got, f"{c}.Rp"), lay.view(E, f"{c}.Rp")
            eRp[...] = W[1]                                                       # off the diagonal: W[1] itself
            for m in range(2):
                ref = np.diag(Rp[m])
                err = np.abs(np.diag(gRp[m]).astype(np.longdouble) - ref)
                bound = T * cg.EPS * jit[m] + cg.EPS * np.abs(ref)
                worst = max(worst, float(np.max(err / bound)))
                assert np.all(err <= bound), (c, m, float(np.max(err / bound)))
                eRp[m][np.diag_indices(T)] = np.diag(gRp[m])                      # checked above; the rest bit for bit below
        assert_same_bits(lay, got, E)
    print(f"gather T={T} n_chains={n_chains}: worst diagonal error / bound = {worst:.3f}")


# --------------------------------------------------------------------------------------------------------------- copy list
def test_copy_list_every_alignment_and_tail():
    """One launch: n in {1, 2, 3, 255, 256, 257, 8100, 65537} x the four (src, dst) 16-byte alignments (both aligned: the double2
    path with its odd-n tail; otherwise the scalar path), and an item with n = 0.  Destinations bit-equal to the sources, NaN
    everywhere else."""
    sizes = [1, 2, 3, 255, 256, 257, 8100, 65536 + 1]
    src, dst = Layout(), Layout()
    items = []
    for n in sizes:
        for ps in (0, 1):
            for pd in (0, 1):
                name = f"n{n}.{ps}{pd}"
                src.f64(name, n, parity=ps)
                dst.f64(name, n, parity=pd)
                items.append((name, n))
    src.f64("empty", 4)
    dst.f64("empty", 4)
    S, Dh = src.host(), dst.host()
    rng = np.random.default_rng(3)
    S[0][:] = rng.normal(size=S[0].size)             # the sources' surroundings are numbers too: a copy that runs over shows up
    dS, dD = upload(S), upload(Dh)
    assert dS[0].data_ptr() % 16 == 0 and dD[0].data_ptr() % 16 == 0
    table = np.array([(src.ptr(dS, name), dst.ptr(dD, name), n) for name, n in items] + [(src.ptr(dS, "empty"), dst.ptr(dD, "empty"), 0)],
                     dtype=np.int64)
    for name, _ in items:                            # the alignment each item was built for
        assert (src.ptr(dS, name) % 16 == 0, dst.ptr(dD, name) % 16 == 0) == (name[-2] == "0", name[-1] == "0")
    assert ctypes.sizeof(_ffi.CopyItem) == 24
    tdev = torch.from_numpy(table).cuda()
    lib, st = _ffi.lib, ops._stream()
    assert lib.hgp_copy_list_f64(ctypes.c_void_p(tdev.data_ptr()), 0, max(sizes), st) == 0
    assert lib.hgp_copy_list_f64(ctypes.c_void_p(tdev.data_ptr()), len(table), 0, st) == -1
    assert lib.hgp_copy_list_f64(ctypes.c_void_p(tdev.data_ptr()), len(table), -5, st) == -1
    assert lib.hgp_copy_list_f64(None, len(table), max(sizes), st) == -1
    assert_same_bits(dst, download(dD), Dh)           # nothing ran so far
    ops.copy_list(tdev, len(table), max(sizes))
    E = (Dh[0].copy(), Dh[1].copy())
    cg.copy_ref([(src.view(S, name), dst.view(E, name), n) for name, n in items] + [(src.view(S, "empty"), dst.view(E, "empty"), 0)])
    assert np.isnan(dst.view(E, "empty")).all() and not np.isnan(dst.view(E, "n257.11")).any()
    assert_same_bits(dst, download(dD), E)
    assert_same_bits(src, download(dS), S)
