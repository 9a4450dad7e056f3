"""TEST INFRASTRUCTURE ONLY - an independent restatement of the switching-variable step in plain NumPy at ``np.longdouble``,
returning float64: GPI_HDP.LogLik(axis=1) (GPI_HDP.py:632-661), forward / backward / coupled_state_coef (GPI_HDP.py:3546-3700),
the hard assignment GPI_HDP._safe_exp (GPI_HDP.py:338-350), and the two reductions of it that ``hgp_hmm_local_terms_f64`` hands
back (``pair_first``, ``last_log``; include/hdpgpc_hip.h).

It is a second opinion beside ``oracle.hdpgpc_oracle`` and ``tests/cpu_double.py`` and imports neither.  What the reference
leaves to torch's conventions is spelled out here instead of inherited from NumPy:

  - the row maximum PROPAGATES NaN (torch.max): a row holding a NaN has the maximum NaN;
  - safe_exp: exp(x - rowmax) with every NaN result replaced by 1e-8 (nan_to_num) - so a row with a NaN, an all -inf row
    (-inf - -inf) and the +inf entries of a row (inf - inf) become 1e-8, the finite entries beside a +inf become 0;
  - the clamps add, they do not floor: forward transition < 1e-6 -> += 1e-4, backward transition < 1e-5 -> += 1e-4,
    exp(log_pi) < 1e-10 -> += 1e-4;
  - the backward normaliser is the sum WITHOUT the last state (GPI_HDP.py:3646);
  - pair table: den == 0 -> 1e-10, so row 0 (respPair[0] = 0) is log(0 / 1e-10) = -inf;
  - every arg-max takes the FIRST index among equals; for the labels NaN counts as the maximum (torch.argmax), the first NaN wins;
  - pair_first is 0 for a row holding a NaN and for an all -inf row (row 0 among them), as the header documents.

  - the logs (pair table, log(fmsg * bmsg)) see float64's range: a product too small for float64 is 0 there, its log -inf.

LogLik alone is evaluated in float64: a row maximum is exact and one subtraction is correctly rounded, so float64 IS the
reference's result to the bit, while a longdouble difference rounded to float64 would round twice.
"""
import numpy as np

LD = np.longdouble
NAN_FILL = LD(1e-8)
EPS_ADD = LD(1e-4)


def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _f64_range(a):
    """longdouble keeps what float64 cannot hold (below 4.9e-324): where the reference takes the LOG of a float64 product, a
    product that underflows there is 0 and its log -inf, so the argument of such a log is rounded to float64 first."""
    return a.astype(np.float64).astype(LD)


def row_max(x):
    """torch.max(x, dim=1)[0]: NaN anywhere in a row is that row's maximum."""
    x = np.asarray(x)
    nan = np.isnan(x)
    m = np.max(np.where(nan, -np.inf, x), axis=1)
    return np.where(nan.any(axis=1), np.nan, m).astype(x.dtype)


def loglik_rows(q):
    """GPI_HDP.LogLik(axis=1): (q - rowmax, rowmax); the input itself if ANY row maximum is infinite.  float64 (see above)."""
    q = np.asarray(q, dtype=np.float64)
    c = row_max(q)
    if np.isinf(c).any():
        return q.copy(), c
    with np.errstate(invalid="ignore"):
        return q - c[:, None], c


def safe_exp(x):
    """The local safe_exp of forward / backward / coupled_state_coef (GPI_HDP.py:3577-3578) on a longdouble [R,C] array."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(x - row_max(x)[:, None])
    return np.where(np.isnan(e), NAN_FILL, e)


def _clamped(P, below):
    return np.where(P < LD(below), P + EPS_ADD, P)


def _forward(q, log_pi, log_trans):
    N, K = q.shape
    pi_ = _clamped(np.exp(log_pi), 1e-10)
    PiT = _clamped(safe_exp(log_trans.T), 1e-6)
    q_ = safe_exp(q)
    fmsg, marg = np.zeros((N, K), dtype=LD), np.zeros(N, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(N):
            v = pi_ * q_[0] if t == 0 else (PiT @ fmsg[t - 1]) * q_[t]
            marg[t] = v.sum()
            fmsg[t] = v / marg[t]
    return fmsg, marg


def _backward(q, log_trans):
    N, K = q.shape
    Pi = _clamped(safe_exp(log_trans), 1e-5)
    q_ = safe_exp(q)
    bmsg = np.ones((N, K), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(N - 2, -1, -1):
            v = Pi @ (bmsg[t + 1] * q_[t + 1])
            bmsg[t] = v / v[:-1].sum()              # the last state is left out of the normaliser
    return bmsg


def _pair(alpha, beta, q, log_trans):
    N, K = q.shape
    Pi = safe_exp(log_trans)                        # no clamp here (GPI_HDP.py:3687)
    soft = safe_exp(q) * beta
    rp = np.zeros((N, K, K), dtype=LD)              # row 0 stays 0
    rp[1:] = alpha[:-1][:, :, None] * soft[1:][:, None, :]
    rp = _f64_range(rp * Pi[None])
    den = rp.sum(axis=(1, 2))
    den = np.where(den == 0, LD(1e-10), den)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log(rp / den[:, None, None])


def forward(q, log_pi, log_trans):
    """GPI_HDP.forward, full recursion: (fmsg [N,K], margPrObs [N])."""
    f, m = _forward(_ld(q), _ld(log_pi).reshape(-1), _ld(log_trans))
    return f.astype(np.float64), m.astype(np.float64)


def backward(q, log_trans):
    """GPI_HDP.backward: bmsg [N,K], last row 1."""
    return _backward(_ld(q), _ld(log_trans)).astype(np.float64)


def pair_coef(alpha, beta, q, log_trans):
    """GPI_HDP.coupled_state_coef: log of the normalised pair responsibilities [N,K,K], row 0 = -inf."""
    return _pair(_ld(alpha), _ld(beta), _ld(q), _ld(log_trans)).astype(np.float64)


def first_argmax_nan_wins(a):
    """torch.argmax over the last axis of a 2-D array: the first NaN if there is one, else the first maximum (an all -inf row: 0)."""
    a = np.asarray(a)
    nan = np.isnan(a)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, a).argmax(axis=1)).astype(np.int64)


def pair_first(table):
    """First arg-max over the flattened K x K entries of every row of the pair table; 0 for a row holding a NaN or nothing
    above -inf (include/hdpgpc_hip.h, hgp_hmm_local_terms_f64)."""
    flat = np.asarray(table).reshape(table.shape[0], -1)
    nan = np.isnan(flat).any(axis=1)
    idx = np.where(np.isnan(flat), -np.inf, flat).argmax(axis=1)
    return np.where(nan, 0, idx).astype(np.int64)


def top_two_gap(a):
    """Per row: largest minus second-largest value; +inf where magnitudes do not decide the arg-max (one column, a NaN in the
    row, nothing above -inf, or a single entry above -inf)."""
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    gap = np.full(a.shape[0], np.inf)
    if a.shape[1] < 2:
        return gap
    s = np.sort(np.where(np.isnan(a), -np.inf, a), axis=1)
    ok = ~np.isnan(a).any(axis=1) & np.isfinite(s[:, -2])
    gap[ok] = (s[ok, -1] - s[ok, -2]).astype(np.float64)
    return gap


def assign(fmsg, bmsg):
    """GPI_HDP._safe_exp of log(fmsg * bmsg): (labels [N] int64, one-hot resp [N,K])."""
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.log(_f64_range(_ld(fmsg) * _ld(bmsg)))
    lab = first_argmax_nan_wins(lg)
    resp = np.zeros(lg.shape)
    resp[np.arange(lg.shape[0]), lab] = 1.0
    return lab, resp


def local_terms(q, log_pi, log_trans):
    """What hgp_hmm_local_terms_f64 computes for ONE score matrix q [N,K], every intermediate carried at longdouble.  Returns a
    dict of float64 / int64 arrays: qnorm, fmsg, marg, bmsg, pair [N,K,K], labels, pair_first, last_log [K], and the top-two
    gaps label_gap [N] / pair_gap [N] of the two arg-max inputs (the rows a float64 evaluation is entitled to reorder)."""
    qn, rowmax = loglik_rows(q)
    ql, lt = _ld(qn), _ld(log_trans)
    f, m = _forward(ql, _ld(log_pi).reshape(-1), lt)
    b = _backward(ql, lt)
    pair = _pair(f, b, ql, lt)
    with np.errstate(invalid="ignore", divide="ignore"):
        lg = np.log(_f64_range(_f64_range(f) * _f64_range(b)))      # the float64 messages are what the assignment reads
    return dict(qnorm=qn, rowmax=rowmax, fmsg=f.astype(np.float64), marg=m.astype(np.float64), bmsg=b.astype(np.float64),
                pair=pair.astype(np.float64), labels=first_argmax_nan_wins(lg), pair_first=pair_first(pair),
                last_log=lg[-1].astype(np.float64), label_gap=top_two_gap(lg), pair_gap=top_two_gap(pair))


def random_case(N, K, B, seed):
    """The generator of the device tests (tests/test_gpu_switching.py), here so that the CPU tier can check what it promises:
    B score matrices q [B,N,K] = 5 N(0,1) - 20, log_trans = log Dirichlet(0.5) rows, log_pi = log Dirichlet(1)."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(B, N, K)) * 5 - 20
    log_trans = np.log(rng.dirichlet(np.full(K, 0.5), size=K))
    log_pi = np.log(rng.dirichlet(np.ones(K)))
    return q, log_pi, log_trans


NONFINITE_KINDS = ("q_nan", "q_pinf", "q_row_ninf", "pi_ninf", "trans_row_ninf", "trans_nan")


def nonfinite_case(kind, where, N, K, seed=0):
    """One score matrix of random_case with a single non-finite feature; where = 0, 1, 2 puts it at the first, a middle, the last
    step of q (row 0, N // 2, N - 1) or, for log_pi / log_trans, at the first, a middle, the last state.  Returns (q [N,K],
    log_pi, log_trans, row): row = the step of q that carries the feature, or -1 if q is finite."""
    q, log_pi, log_trans = random_case(N, K, 1, seed)
    q = q[0]
    t, s = (0, N // 2, N - 1)[where], (0, K // 2, K - 1)[where]
    col = (1 + where) % K
    if kind == "q_nan":
        q[t, col] = np.nan
    elif kind == "q_pinf":
        q[t, col] = np.inf
    elif kind == "q_row_ninf":
        q[t, :] = -np.inf
    elif kind == "pi_ninf":
        log_pi[s] = -np.inf
    elif kind == "trans_row_ninf":
        log_trans[s, :] = -np.inf
    elif kind == "trans_nan":
        log_trans[s, col] = np.nan
    else:
        raise ValueError(kind)
    return q, log_pi, log_trans, (t if kind.startswith("q_") else -1)


def with_infinite_row_max(q, avoid_row):
    """q itself if LogLik already returns it unchanged (an infinite row maximum), else a copy with one +inf planted in a row
    other than avoid_row - so that a matrix reaches the messages as it is, not normalised."""
    if np.isinf(row_max(q)).any():
        return q
    q = q.copy()
    q[(max(avoid_row, 0) + 1) % q.shape[0], 0] = np.inf
    return q
