"""The static filter chain (hgp_static_chain_steps_f64, include/hdpgpc_hip_static.h) against its NumPy restatement
(tests/static_ref.py): T = 20 and 90 (a partial last tile), 32 (exact tiles), 128 (the largest size); chains of 1, 2 and 5 members,
alone and three in one call; with and without the first-step branch; A and C the identity (the short-cut) and the identity plus a
1e-2 perturbation (every product).  Gate 1e-9 relative to the row's largest entry on every appended row (the
producer lists' gate).  Bit for bit: a chain alone = the chain inside a batch at any position; n members in one call = n1 + n2 in
two; the identity short-cut = the full products; the NaN guard words behind every output and the workspace stand; an indefinite
Sigma or a NaN observation in one chain leaves the other chains' bits alone."""
import ctypes

import numpy as np
import pytest
import torch

import conftest
import static_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64          # NaN words behind every output
SIZES = (20, 32, 90, 128)
LENS = (1, 5, 2)


def host_case(T, n, seed, ident, first, pos0=2):
    """One chain's inputs as arrays: rows 0 .. pos0 of the stacks are filled (row pos0 is the state the chain starts from)."""
    rng = np.random.default_rng(seed)
    x = np.arange(T, dtype=np.float64)
    gram = 2.0 * np.exp(-0.5 * ((x[:, None] - x[None, :]) / 1.2) ** 2)
    eye = np.eye(T)
    A, C = eye.copy(), eye.copy()
    if not ident:
        A += 1e-2 * rng.standard_normal((T, T))
        C += 1e-2 * rng.standard_normal((T, T))
    G = rng.standard_normal((T, T)) / np.sqrt(T)
    Sigma = 0.25 * eye + 0.05 * (G @ G.T)
    rows = pos0 + n + 1
    Fs, Ps = rng.standard_normal((rows, T)), rng.standard_normal((rows, T, T))
    if first:
        Ps[pos0], Fs[pos0] = gram + 0.01 * eye, 0.0
    else:
        H = rng.standard_normal((T, T)) / np.sqrt(T)
        Ps[pos0] = 0.3 * gram + 0.1 * eye + 0.1 * (H @ H.T)
    Y = rng.standard_normal((n + 3, T))
    y_idx = rng.permutation(n + 3)[:n]
    return dict(A=A, C=C, Sigma=Sigma, Fs=Fs, Ps=Ps, pos=pos0, Y=Y, y_idx=y_idx, first=first, white=0.01, n=n, T=T)


def guarded(a, dtype=torch.float64):
    """(a fresh device copy of `a`, the buffer it lies in - GUARD NaN words behind it -, the words it takes)."""
    a = np.ascontiguousarray(a)
    used = (a.nbytes + 7) // 8
    buf = torch.full((used + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    view = buf[:used].view(dtype)[:a.size].view(*a.shape)
    view.copy_(torch.as_tensor(a, dtype=dtype))
    return view, buf, used


def guards_ok(buf, used):
    return buf.numel() - used == GUARD and bool(torch.isnan(buf[used:]).all())


class DevChain:
    def __init__(self, h, flags=0):
        from hdpgpc_amd import ops
        self.h = h
        up = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=DEV)      # noqa: E731
        self.A, self.C, self.Sigma, self.Y = up(h["A"]), up(h["C"]), up(h["Sigma"]), up(h["Y"])
        self.Fs, self.Ps = guarded(h["Fs"]), guarded(h["Ps"])
        self.pos = guarded(np.array([h["pos"]], dtype=np.int64), torch.int64)
        self.info = guarded(np.zeros(2, dtype=np.int32), torch.int32)          # [1]: the word next to the status word
        self.guarded = (self.Fs, self.Ps, self.pos, self.info)
        self.Fs, self.Ps, self.pos, self.info = (g[0] for g in self.guarded)
        self.y_idx = torch.as_tensor(np.asarray(h["y_idx"], dtype=np.int64), device=DEV)
        self.desc = ops.static_chain_desc(self.A, self.C, self.Sigma, self.Fs, self.Ps, self.pos, self.Y, self.y_idx, self.info,
                                          h["n"], h["pos"], first=h["first"], white=h["white"], flags=flags)

    def result(self):
        torch.cuda.synchronize()
        assert all(guards_ok(buf, used) for _, buf, used in self.guarded) and int(self.info[1]) == 0
        return self.Fs.cpu().numpy(), self.Ps.cpu().numpy(), int(self.pos[0]), int(self.info[0])


def launch(chains, T, max_steps):
    """One call over the chains, on a workspace of exactly the reported size with guard words behind it."""
    from hdpgpc_amd import _ffi
    from hdpgpc_amd.member_step import upload_descs
    B = len(chains)
    need = int(_ffi.lib.hgp_static_chain_ws_bytes(B, T))
    assert need % 8 == 0 and need > 0
    ws = torch.full((need // 8 + GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    descs = upload_descs([c.desc for c in chains], DEV)
    rc = _ffi.lib.hgp_static_chain_steps_f64(ctypes.c_void_p(descs.data_ptr()), B, T, max_steps, ctypes.c_void_p(ws.data_ptr()), need, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert guards_ok(ws, need // 8)
    return descs


def run(hosts, T, max_steps=1 << 20, flags=0, calls=1):
    chains = [DevChain(h, flags) for h in hosts]
    for _ in range(calls):
        launch(chains, T, max_steps)
    return [c.result() for c in chains]


def reference(h, max_steps=1 << 20):
    r = static_ref.Chain(h["A"], h["C"], h["Sigma"], h["Fs"], h["Ps"], h["pos"], h["Y"], h["y_idx"], h["first"], h["white"])
    r.steps(max_steps)
    return r.Fs, r.Ps, r.pos, r.info


def same_bits(a, b):
    """Two results (Fs, Ps, pos, info) equal bit for bit."""
    return (np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1].view(np.int64), b[1].view(np.int64))
            and a[2:] == b[2:])


def check_rows(got, want, h):
    """Every appended row at 1e-9 of the row's scale; every other row untouched."""
    (F, P, pos, info), (Fr, Pr, pos_r, info_r) = got, want
    assert (pos, info) == (pos_r, info_r)
    p0 = h["pos"]
    assert np.array_equal(F[:p0 + 1], h["Fs"][:p0 + 1]) and np.array_equal(P[:p0 + 1], h["Ps"][:p0 + 1])
    for r in range(p0 + 1, p0 + h["n"] + 1):
        assert conftest.relclose(F[r], Fr[r], 1e-9), ("mean", r)
        assert conftest.relclose(P[r], Pr[r], 1e-9), ("cov", r)


@pytest.mark.parametrize("first", (False, True), ids=("later", "first"))
@pytest.mark.parametrize("ident", (True, False), ids=("identity", "perturbed"))
@pytest.mark.parametrize("T", SIZES)
def test_chains_match_the_restatement_alone_and_in_a_batch(T, ident, first):
    hosts = [host_case(T, n, 100 * T + k, ident, first) for k, n in enumerate(LENS)]
    batch = run(hosts, T)
    for h, got in zip(hosts, batch):
        check_rows(got, reference(h), h)
    for k, h in enumerate(hosts):                                  # B = 1: the same bits as inside the batch
        assert same_bits(run([h], T)[0], batch[k]), k
    back = run(hosts[::-1], T)[::-1]                               # ... and at any position
    for k in range(len(hosts)):
        assert same_bits(back[k], batch[k]), k


@pytest.mark.parametrize("ident", (True, False), ids=("identity", "perturbed"))
@pytest.mark.parametrize("T", SIZES)
def test_two_calls_leave_the_bits_of_one(T, ident):
    hosts = [host_case(T, n, 7 * T + k, ident, k == 0) for k, n in enumerate((5, 2, 4))]
    once = run(hosts, T)
    twice = run(hosts, T, max_steps=2, calls=3)                    # 2 + 2 + 1 members; the shorter chains end earlier
    for k in range(len(hosts)):
        assert same_bits(once[k], twice[k]), k
    part = run(hosts, T, max_steps=2)                              # one short call: progress as the restatement states it
    for h, got in zip(hosts, part):
        Fr, Pr, pos_r, info_r = reference(h, 2)
        assert (got[2], got[3]) == (pos_r, info_r) == (h["pos"] + min(2, h["n"]), 0)
        assert np.array_equal(got[1][pos_r + 1:], h["Ps"][pos_r + 1:])          # rows not yet appended: untouched


@pytest.mark.parametrize("T", SIZES)
def test_identity_short_cut_has_the_bits_of_the_full_products(T):
    hosts = [host_case(T, 3, 11 * T + k, True, k == 1) for k in range(3)]
    hosts[2]["Ps"][hosts[2]["pos"], 1, 3] = -0.0                   # a signed zero in the state must come out as the products leave it
    hosts[2]["Fs"][hosts[2]["pos"], 0] = -0.0
    rng = np.random.default_rng(T)
    hosts[0]["C"] = hosts[0]["C"] + 1e-2 * rng.standard_normal((T, T))      # A the identity, C not
    short, full = run(hosts, T), run(hosts, T, flags=1)
    for k in range(3):
        assert short[k][3] == 0 and same_bits(short[k], full[k]), k


def test_indefinite_sigma_ends_its_chain_and_no_other():
    T = 90
    hosts = [host_case(T, n, 900 + k, False, False) for k, n in enumerate(LENS)]
    clean = run(hosts, T)
    bad = dict(hosts[1])
    bad["Sigma"] = hosts[1]["Sigma"].copy()
    bad["Sigma"][7, 7] = -50.0
    got = run([hosts[0], bad, hosts[2]], T)
    assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])
    F, P, pos, info = got[1]
    Fr, Pr, pos_r, info_r = reference(bad)
    assert info == info_r == 8 and pos == pos_r == bad["pos"] + bad["n"]
    assert np.isnan(F[bad["pos"] + 1:]).all() and np.isnan(P[bad["pos"] + 1:]).all()
    assert np.array_equal(F[:bad["pos"] + 1], bad["Fs"][:bad["pos"] + 1]) and np.array_equal(P[:bad["pos"] + 1], bad["Ps"][:bad["pos"] + 1])
    again = DevChain(bad)                                          # a chain that has ended is left alone by later calls
    launch([again], T, 1 << 20)
    first_call = again.result()
    launch([again], T, 1 << 20)
    assert same_bits(again.result(), first_call)


@pytest.mark.parametrize("ident", (True, False), ids=("identity", "perturbed"))
def test_a_nan_observation_stays_in_its_chain(ident):
    T = 32
    hosts = [host_case(T, n, 300 + k, ident, False) for k, n in enumerate(LENS)]
    clean = run(hosts, T)
    bad = dict(hosts[1])
    bad["Y"] = hosts[1]["Y"].copy()
    bad["Y"][bad["y_idx"][1], 5] = np.nan
    got = run([hosts[0], bad, hosts[2]], T)
    assert same_bits(got[0], clean[0]) and same_bits(got[2], clean[2])
    F, P, pos, info = got[1]
    Fr, Pr, pos_r, info_r = reference(bad)
    assert (pos, info) == (pos_r, info_r) == (bad["pos"] + bad["n"], 0)
    assert np.array_equal(np.isnan(F), np.isnan(Fr)) and np.isnan(F[bad["pos"] + 2:]).all() and not np.isnan(F[bad["pos"] + 1]).any()
    assert np.array_equal(P.view(np.int64), clean[1][1].view(np.int64))                         # the covariances do not depend on the observations


def test_return_codes_and_the_wrapper():
    from hdpgpc_amd import _ffi, ops
    from hdpgpc_amd.member_step import upload_descs
    T = 20
    h = host_case(T, 2, 5, True, False)
    ch = DevChain(h)
    descs = upload_descs([ch.desc], DEV)
    p = ctypes.c_void_p(descs.data_ptr())
    need = int(_ffi.lib.hgp_static_chain_ws_bytes(1, T))
    ws = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    w = ctypes.c_void_p(ws.data_ptr())
    fn = _ffi.lib.hgp_static_chain_steps_f64
    assert fn(p, 1, 129, 1, w, need, None) == -2
    assert fn(p, 1, T, 1, w, need - 1, None) == -1
    assert fn(p, 1, T, 0, w, need, None) == 0 and fn(p, 0, T, 1, w, need, None) == 0
    torch.cuda.synchronize()
    assert int(ch.pos[0]) == h["pos"]                              # nothing ran
    with pytest.raises(NotImplementedError):
        ops.static_chain_steps(descs, 1, 129, 1)
    ops.static_chain_steps(descs, 1, T, 5)                         # the wrapper, on its own workspace
    check_rows(ch.result(), reference(h), h)
    ops.static_chain_release()
