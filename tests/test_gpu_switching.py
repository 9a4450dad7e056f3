"""The switching-variable step on the device, entry point by entry point, against tests/hmm_ref.py (longdouble NumPy; pinned to
the reference's outputs, the oracle and the CPU stand-ins in tests/test_hmm_ref.py) and torch on the CPU:
hgp_hmm_local_terms_f64 (all seven outputs), hgp_loglik_rows_f64, hgp_assign_f64 and hgp_hmm_messages_f64 with non-finite scores.

Every output lives inside a larger tensor with a guard band on both sides and is pre-filled with a marker (a NaN with a payload
no arithmetic produces; -1 for the int64 outputs): a call must leave the guards alone and no marker where an output is defined.

Tolerances are the project's own for these kernels: messages rtol 1e-10 on short chains (test_hmm_messages_edge_sizes), 1e-9
beyond a thousand steps and 1e-8 on the pair table (test_hmm_messages_8f3_golden_and_large), atol 1e-300 on messages.
last_log is the log of a message: a relative error r of the message is an absolute error r of its log, hence rtol = atol = r."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import hmm_ref
from conftest import rel_err

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import _ffi

GUARD = 64                                   # elements on each side of every output
F64_GUARD = -6.02214076e23
F64_MARK = 0x7FF8DEAD0000BEEF                # bits of the pre-fill NaN
I64_GUARD, I64_MARK = -0x5EED, -1
SHAPES = [(1, 1), (1, 5), (2, 2), (7, 3), (8, 9), (9, 9), (10, 2), (17, 64), (300, 33), (1100, 9)]
OUTPUTS = ("qnorm", "fmsg", "marg", "bmsg", "labels", "pair_first", "last_log")


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """same_bits, except that a NaN only has to be a NaN (its sign and payload are not part of any contract)."""
    ok = ~np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), ~ok) and np.array_equal(bits(a)[ok], bits(b)[ok])


class Out:
    """An output buffer of the given shape in the middle of a guarded, pre-filled tensor."""

    def __init__(self, shape, dtype=torch.float64):
        self.shape, self.n, self.f64 = shape, int(np.prod(shape)), dtype == torch.float64
        self.raw = torch.full((self.n + 2 * GUARD,), F64_GUARD if self.f64 else I64_GUARD, dtype=dtype, device="cuda")
        self.body = self.raw[GUARD:GUARD + self.n]
        if self.f64:
            self.body.view(torch.int64).fill_(F64_MARK)
        else:
            self.body.fill_(I64_MARK)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.body.data_ptr())

    def get(self):
        """The output as a NumPy array, after checking the guards and that the call wrote every element."""
        raw = self.raw.cpu().numpy()
        g = np.concatenate([raw[:GUARD], raw[GUARD + self.n:]])
        assert (g == (F64_GUARD if self.f64 else I64_GUARD)).all(), "a guard element was overwritten"
        body = raw[GUARD:GUARD + self.n]
        left = (bits(body) == F64_MARK) if self.f64 else (body == I64_MARK)
        assert not left.any(), f"{int(left.sum())} of {self.n} output elements were never written"
        return body.reshape(self.shape).copy()


def run_local_terms(Q, lp, lt, want_pair=True, want_last=True):
    """hgp_hmm_local_terms_f64 on Q [B,N,K] through the C-ABI: dict of the seven outputs (None for one not asked for)."""
    B, N, K = Q.shape
    o = dict(qnorm=Out((B, N, K)), fmsg=Out((B, N, K)), marg=Out((B, N)), bmsg=Out((B, N, K)), labels=Out((B, N), torch.int64),
             pair_first=Out((B, N), torch.int64) if want_pair else None, last_log=Out((B, K)) if want_last else None)
    p = {k: (None if v is None else v.ptr) for k, v in o.items()}
    Qd, lpd, ltd = dev(Q), dev(lp), dev(lt)
    rc = _ffi.lib.hgp_hmm_local_terms_f64(ptr(Qd), ptr(lpd), ptr(ltd), N, K, B, p["qnorm"], p["fmsg"], p["marg"], p["bmsg"],
                                          p["labels"], p["pair_first"], p["last_log"], stream())
    assert rc == 0
    torch.cuda.synchronize()
    return {k: (None if v is None else v.get()) for k, v in o.items()}


def run_messages(q, lp, lt, want_pair=True):
    """hgp_hmm_messages_f64 through the C-ABI: (fmsg, marg, bmsg, table or None)."""
    N, K = q.shape
    o = [Out((N, K)), Out((N,)), Out((N, K)), Out((N, K, K)) if want_pair else None]
    qd, lpd, ltd = dev(q), dev(lp), dev(lt)
    rc = _ffi.lib.hgp_hmm_messages_f64(ptr(qd), ptr(lpd), ptr(ltd), N, K, o[0].ptr, o[1].ptr, o[2].ptr,
                                       None if o[3] is None else o[3].ptr, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(None if v is None else v.get() for v in o)


@functools.lru_cache(maxsize=None)
def case(N, K):
    """Three score matrices of the shape (seed = position of the shape in SHAPES, mod 3: the seeds tests/test_hmm_ref.py checks
    for near-ties), their reference, the B = 3 call and the three B = 1 calls - computed once, shared by the tests below."""
    Q, lp, lt = hmm_ref.random_case(N, K, 3, SHAPES.index((N, K)) % 3)
    ref = [hmm_ref.local_terms(Q[v], lp, lt) for v in range(3)]
    return Q, lp, lt, ref, run_local_terms(Q, lp, lt), [run_local_terms(Q[v:v + 1], lp, lt) for v in range(3)]


def msg_tol(N):
    return 1e-9 if N > 1000 else 1e-10


def check_against_reference(got, ref, N):
    """One matrix: got = dict of the device outputs [N,K] / [N] / [K], ref = hmm_ref.local_terms of the same input."""
    r = msg_tol(N)
    assert same_bits_or_nan(got["qnorm"], ref["qnorm"])                        # a maximum and one subtraction: exact
    errs = {k: rel_err(got[k], ref[k]) for k in ("fmsg", "marg", "bmsg")}
    fin = np.isfinite(ref["last_log"])
    assert np.array_equal(np.isfinite(got["last_log"]), fin)
    errs["last_log"] = float(np.max(np.abs(got["last_log"][fin] - ref["last_log"][fin]), initial=0.0))
    print(f"N={N} K={got['fmsg'].shape[1]} max errors {errs}")
    # the figures are printed above (pytest -s); the same formulas in float64 on the CPU are 1.2e-15 from this reference
    assert np.allclose(got["fmsg"], ref["fmsg"], rtol=r, atol=1e-300) and np.allclose(got["marg"], ref["marg"], rtol=r, atol=0)
    assert np.allclose(got["bmsg"], ref["bmsg"], rtol=r, atol=1e-300)
    assert np.allclose(got["last_log"][fin], ref["last_log"][fin], rtol=r, atol=r)
    for name, gap in (("labels", "label_gap"), ("pair_first", "pair_gap")):
        decided = ref[gap] > 1e-6
        assert decided.mean() >= 0.99
        assert np.array_equal(got[name][decided], ref[name][decided]), name


# ------------------------------------------------------------------------------------------------ a. hgp_hmm_local_terms_f64
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,K", SHAPES)
def test_local_terms_all_outputs_match_the_reference(N, K, B):
    """qnorm to the bit, fmsg / marg / bmsg / last_log within the message tolerance, labels and pair_first equal on every row
    the reference decides by more than 1e-6 (at least 99 % of the rows; tests/test_hmm_ref.py: all of them)."""
    Q, lp, lt, ref, got3, got1 = case(N, K)
    for v in range(B):
        got = got3 if B == 3 else got1[0]
        check_against_reference({k: got[k][v] for k in OUTPUTS}, ref[v], N)


@pytest.mark.parametrize("N,K", SHAPES)
def test_local_terms_variants_of_a_batch_are_independent(N, K):
    """Variant b of a B = 3 call = the B = 1 call on the same matrix, all seven outputs, to the bit (blockIdx.y / blockIdx.x offsets)."""
    Q, lp, lt, ref, got3, got1 = case(N, K)
    for v in range(3):
        for k in OUTPUTS:
            a, b = got3[k][v], got1[v][k][0]
            assert np.array_equal(a, b) if a.dtype == np.int64 else same_bits(a, b), (k, v)


@pytest.mark.parametrize("N,K", SHAPES)
def test_local_terms_pair_first_is_the_first_arg_max_of_the_table(N, K):
    """pair_first (k_hmm_pair_first) against the table hgp_hmm_messages_f64 (k_hmm_pair) writes for the same qnorm: the two
    kernels evaluate the same expression element by element, so the arg-max agrees on EVERY row; the messages agree to the bit."""
    Q, lp, lt, ref, got3, got1 = case(N, K)
    for v in range(3):
        f, m, b, table = run_messages(got3["qnorm"][v], lp, lt)
        assert same_bits(f, got3["fmsg"][v]) and same_bits(m, got3["marg"][v]) and same_bits(b, got3["bmsg"][v])
        assert np.array_equal(got3["pair_first"][v], hmm_ref.pair_first(table))
        fin = np.isfinite(ref[v]["pair"])
        assert np.array_equal(np.isfinite(table), fin) and not np.isnan(table).any()
        print(f"N={N} K={K} table max abs error {np.max(np.abs(table[fin] - ref[v]['pair'][fin]), initial=0.0):.2e}")
        # the figure is printed above (pytest -s); float64 on the CPU: 7.1e-15
        assert np.allclose(table[fin], ref[v]["pair"][fin], rtol=1e-8, atol=1e-8)


def test_local_terms_unchanged_input_rule_is_per_matrix():
    """Only the middle variant holds a +inf score: its qnorm is its input, the other two are normalised, all three match."""
    Q, lp, lt = hmm_ref.random_case(9, 9, 3, 2)
    Q[1, 4, 3] = np.inf
    got = run_local_terms(Q, lp, lt)
    assert same_bits(got["qnorm"][1], Q[1])
    for v in (0, 2):
        assert same_bits(got["qnorm"][v], Q[v] - Q[v].max(axis=1, keepdims=True)) and not same_bits(got["qnorm"][v], Q[v])
    for v in range(3):
        check_against_reference({k: got[k][v] for k in OUTPUTS}, hmm_ref.local_terms(Q[v], lp, lt), 9)


@pytest.mark.parametrize("N,K", [(9, 9), (300, 33)])
def test_local_terms_optional_outputs(N, K):
    """pair_first == NULL and last_log == NULL are accepted and leave the other outputs as they were."""
    Q, lp, lt, ref, got3, got1 = case(N, K)
    for want_pair, want_last in ((False, True), (True, False), (False, False)):
        got = run_local_terms(Q, lp, lt, want_pair, want_last)
        for k in OUTPUTS:
            if got[k] is None:
                assert not (want_pair if k == "pair_first" else want_last)
            else:
                assert np.array_equal(got[k], got3[k]) if got[k].dtype == np.int64 else same_bits(got[k], got3[k]), k


# ------------------------------------------------------------------------------------------------ b. hgp_loglik_rows_f64
def run_loglik(q, want_rowmax=True):
    N, K = q.shape
    out, rowmax = Out((N, K)), Out((N,)) if want_rowmax else None
    qd = dev(q)
    assert _ffi.lib.hgp_loglik_rows_f64(ptr(qd), N, K, out.ptr, None if rowmax is None else rowmax.ptr, stream()) == 0
    torch.cuda.synchronize()
    return out.get(), None if rowmax is None else rowmax.get()


def torch_loglik(q):
    """GPI_HDP.LogLik(axis=1), torch branch, on the CPU."""
    t = torch.as_tensor(q)
    c = torch.max(t, dim=1)[0]
    return (t if bool(torch.any(torch.isinf(c))) else t - c[:, None]).numpy(), c.numpy()


@pytest.mark.parametrize("K", [1, 9, 64])
@pytest.mark.parametrize("N", [1, 1024, 1025, 2272])
def test_loglik_rows_matches_torch_to_the_bit(N, K):
    """Finite scores, -inf entries beside a finite maximum (normal path), and the two ways into the unchanged-input branch: a
    +inf in one late row (beyond the first 1024 where there are that many: the flag crosses the workgroup) and an all -inf row."""
    rng = np.random.default_rng(1000 * K + N)
    q = rng.normal(size=(N, K)) * 5 - 20
    out, rowmax = run_loglik(q)
    ro, rc = torch_loglik(q)
    assert same_bits(out, ro) and same_bits(rowmax, rc) and (out.max(axis=1) == 0.0).all()
    assert same_bits(run_loglik(q, want_rowmax=False)[0], ro)
    late = N - 1 if N <= 1024 else (1024 if N == 1025 else 2000)
    if K > 1:
        qm = q.copy()
        qm[rng.random(size=(N, K)) < 0.3] = -np.inf
        qm[np.arange(N), rng.integers(0, K, size=N)] = -7.0          # every row keeps a finite maximum
        qm[late, :K - 1], qm[late, K - 1] = -np.inf, -3.0
        out, rowmax = run_loglik(qm)
        ro, rc = torch_loglik(qm)
        assert np.isfinite(rc).all() and same_bits(out, ro) and same_bits(rowmax, rc) and not same_bits(out, qm)
    for value, cols in ((np.inf, slice(K - 1, K)), (-np.inf, slice(0, K))):
        qi = q.copy()
        qi[late, cols] = value
        out, rowmax = run_loglik(qi)
        ro, rc = torch_loglik(qi)
        assert same_bits(ro, qi) and same_bits(out, qi) and same_bits(rowmax, rc) and rowmax[late] == value
        assert same_bits(run_loglik(qi, want_rowmax=False)[0], qi)


# ------------------------------------------------------------------------------------------------ c. hgp_assign_f64
def run_assign(f, b, want_labels=True, want_resp=True):
    N, K = f.shape
    labels, resp = Out((N,), torch.int64) if want_labels else None, Out((N, K)) if want_resp else None
    fd, bd = dev(f), dev(b)
    assert _ffi.lib.hgp_assign_f64(ptr(fd), ptr(bd), N, K, None if labels is None else labels.ptr,
                                   None if resp is None else resp.ptr, stream()) == 0
    torch.cuda.synchronize()
    return None if labels is None else labels.get(), None if resp is None else resp.get()


def assign_rows(N, K, seed):
    """fmsg, bmsg whose products are exact powers of two (so log() cannot reorder them: distinct products are log 2 apart, equal
    ones are exact ties - frequent at K = 64), with constructed rows every third row: ties of every entry, a tie of two maxima
    away from column 0, all-zero products, a NaN in the first / a middle / the last column, two NaNs."""
    rng = np.random.default_rng(seed)
    f = 2.0 ** -rng.integers(0, 40, size=(N, K)).astype(np.float64)
    b = 2.0 ** -rng.integers(0, 40, size=(N, K)).astype(np.float64)
    mid = K // 2
    for n in range(0, N, 3):
        kind = (n // 3) % 7
        if kind == 0:
            f[n], b[n] = 2.0 ** -np.arange(K), 2.0 ** (np.arange(K) - 70.0)
        elif kind == 1:
            f[n], b[n] = 2.0 ** -30, 2.0 ** -30
            f[n, [mid, K - 1]], b[n, [mid, K - 1]] = (0.5, 0.25), (0.25, 0.5)
        elif kind == 2:
            f[n, ::2], b[n, 1::2] = 0.0, 0.0
        elif kind == 3:
            f[n, 0] = np.nan
        elif kind == 4:
            b[n, mid] = np.nan
        elif kind == 5:
            f[n, K - 1] = np.nan
        else:
            f[n, mid], b[n, K - 1] = np.nan, np.nan
    return f, b


@pytest.mark.parametrize("K", [1, 2, 64])
@pytest.mark.parametrize("N", [1, 255, 256, 257])
def test_assign_labels_and_one_hot_rows(N, K):
    """labels = torch.argmax(torch.log(f * b)) (first maximum, first NaN wins), resp = exactly one 1.0 per row, at the label;
    the labels-only and the resp-only call give the same."""
    f, b = assign_rows(N, K, 10 * N + K)
    want = torch.argmax(torch.log(torch.as_tensor(f) * torch.as_tensor(b)), dim=1).numpy()
    assert np.array_equal(want, hmm_ref.assign(f, b)[0])
    onehot = np.zeros((N, K))
    onehot[np.arange(N), want] = 1.0
    labels, resp = run_assign(f, b)
    assert np.array_equal(labels, want) and same_bits(resp, onehot)
    assert np.array_equal(run_assign(f, b, want_resp=False)[0], want)
    assert same_bits(run_assign(f, b, want_labels=False)[1], onehot)


# ------------------------------------------------------------------------------------------------ d. non-finite scores
@pytest.mark.parametrize("N,K", [(12, 4), (9, 9)])
@pytest.mark.parametrize("where", [0, 1, 2])
@pytest.mark.parametrize("kind", hmm_ref.NONFINITE_KINDS)
def test_messages_with_non_finite_scores(kind, where, N, K):
    """One NaN / one +inf / an all -inf row of q at the first, a middle, the last step; a -inf in log_pi; an all -inf row and a
    NaN in log_trans: hgp_hmm_messages_f64 with and without the table, and hgp_hmm_local_terms_f64 on a matrix LogLik hands on
    unchanged.  The reference's safe_exp takes torch.max, which propagates NaN: a NaN score turns its whole row into 1e-8."""
    q, lp, lt, row = hmm_ref.nonfinite_case(kind, where, N, K)
    fr, mr = hmm_ref.forward(q, lp, lt)
    br = hmm_ref.backward(q, lt)
    pr = hmm_ref.pair_coef(fr, br, q, lt)
    f, m, b, table = run_messages(q, lp, lt)
    f2, m2, b2, _ = run_messages(q, lp, lt, want_pair=False)
    assert same_bits(f, f2) and same_bits(m, m2) and same_bits(b, b2)
    print(f"{kind} at {where}: fmsg {rel_err(f, fr):.2e} marg {rel_err(m, mr):.2e} bmsg {rel_err(b, br):.2e}")
    # the figures are printed here (pytest -s); float64 on the CPU: messages 1.8e-15, table 3.6e-15
    assert np.allclose(f, fr, rtol=1e-10, atol=1e-300) and np.allclose(m, mr, rtol=1e-10, atol=0)
    assert np.allclose(b, br, rtol=1e-10, atol=1e-300)
    fin = np.isfinite(pr)
    assert np.array_equal(np.isfinite(table), fin) and not np.isnan(table).any()
    print(f"table max abs error {np.max(np.abs(table[fin] - pr[fin]), initial=0.0):.2e}")
    assert np.allclose(table[fin], pr[fin], rtol=1e-8, atol=1e-8)
    q2 = hmm_ref.with_infinite_row_max(q, row)
    got = run_local_terms(q2[None], lp, lt)
    assert same_bits_or_nan(got["qnorm"][0], q2)
    check_against_reference({k: got[k][0] for k in OUTPUTS}, hmm_ref.local_terms(q2, lp, lt), N)
    f3, m3, b3, table3 = run_messages(q2, lp, lt)
    assert same_bits(f3, got["fmsg"][0]) and same_bits(b3, got["bmsg"][0])
    assert np.array_equal(got["pair_first"][0], hmm_ref.pair_first(table3))
