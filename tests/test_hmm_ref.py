"""CPU tier: pins tests/hmm_ref.py - the longdouble restatement the device tests of the switching variable compare with
(tests/test_gpu_switching.py) - to the reference's own outputs, to the oracle and to the CPU stand-ins, and to the conventions
its docstring spells out.  No kernel runs here."""
import numpy as np
import pytest
import torch

import cpu_double
import hmm_ref
from conftest import golden
from oracle import hdpgpc_oracle as orc

# float64 evaluations of the same formulas (the reference's own run, the oracle, the stand-ins) differ from the longdouble one by
# their own rounding: K-term dot products and a handful of products per step, renormalised at every step - a few 1e-16 per entry
# (largest seen 1.2e-15 at K = 64).  1e-13 leaves two digits of margin and is 1000 x below what the device tests ask of the kernels.
RTOL = 1e-13
SHAPES = [(1, 1), (1, 5), (2, 2), (7, 3), (8, 9), (9, 9), (10, 2), (17, 64), (300, 33), (1100, 9)]


def close(a, b, rtol=RTOL, atol=1e-300):
    return np.allclose(a, b, rtol=rtol, atol=atol, equal_nan=True)


def same_table(a, b, tol=RTOL):
    fin = np.isfinite(b)
    return np.array_equal(np.isfinite(a), fin) and np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a[fin], b[fin], rtol=tol, atol=tol)


def test_reference_run_of_record_102():
    """forward / backward / coupled_state_coef as the reference itself computed them (scores down to -1e3: messages underflow)."""
    g = golden("hmm_r102_t45.npz")
    q, lp, lt = g["q"], g["log_pi"], g["log_trans"]
    f, m = hmm_ref.forward(q, lp, lt)
    b = hmm_ref.backward(q, lt)
    assert close(f, g["fmsg"]) and close(m, g["margPrObs"], atol=0) and close(b, g["bmsg"])
    # the table holds logs of products down in float64's subnormals, where the reference's own intermediates lose their digits:
    # values above log(2.3e-308) + 8 are compared, the pattern of -inf everywhere else
    p, pr = hmm_ref.pair_coef(f, b, q, lt), g["log_respPair"]
    top = pr > -700
    assert np.array_equal(p > -700, top) and np.allclose(p[top], pr[top], rtol=1e-12, atol=1e-12)
    assert np.array_equal(np.isneginf(p[0]), np.ones_like(p[0], dtype=bool))
    assert np.array_equal(hmm_ref.assign(f, b)[0], np.argmax(g["fmsg"] * g["bmsg"], axis=1))


@pytest.mark.parametrize("N,K", SHAPES)
def test_oracle_and_stand_ins_on_the_device_tests_generator(N, K):
    """The generator, shapes and seeds of the device tests: hmm_ref = oracle = cpu_double on finite scores, and the arg-max
    inputs of hmm_ref leave no row within 1e-6 of a tie (the device tests assert >= 99 % of the rows on this promise)."""
    for seed in (0, 1, 2):
        Q, lp, lt = hmm_ref.random_case(N, K, 3, seed)
        assert np.isfinite(lp).all() and np.isfinite(lt).all()
        lab_cd, pair_cd, last_cd = cpu_double.hmm_local_terms(torch.as_tensor(Q), torch.as_tensor(lp), torch.as_tensor(lt))
        for v in range(3):
            r = hmm_ref.local_terms(Q[v], lp, lt)
            qn, c = cpu_double.loglik_rows(torch.as_tensor(Q[v]))
            assert np.array_equal(r["qnorm"], qn.numpy()) and np.array_equal(r["rowmax"], c.numpy())
            with np.errstate(divide="ignore", invalid="ignore"):
                fo, mo = orc.hmm_forward(r["qnorm"], lp, lt)
                bo = orc.hmm_backward(r["qnorm"], lt)
                po = orc.hmm_pair_coef(fo, bo, r["qnorm"], lt)
            assert close(r["fmsg"], fo) and close(r["marg"], mo, atol=0) and close(r["bmsg"], bo)
            assert same_table(r["pair"], po, 1e-12)
            assert (r["label_gap"] > 1e-6).all() and (r["pair_gap"] > 1e-6).all()
            assert np.array_equal(r["labels"], lab_cd[v].numpy()) and np.array_equal(r["pair_first"], pair_cd[v].numpy())
            assert np.allclose(r["last_log"], last_cd[v].numpy(), rtol=RTOL, atol=RTOL, equal_nan=True)
            lab, resp = cpu_double.assign(torch.as_tensor(r["fmsg"]), torch.as_tensor(r["bmsg"]), want_resp=True)
            lab_r, resp_r = hmm_ref.assign(r["fmsg"], r["bmsg"])
            assert np.array_equal(lab_r, lab.numpy()) and np.array_equal(resp_r, resp.numpy())


@pytest.mark.parametrize("K,N", [(4, 12), (9, 9)])
@pytest.mark.parametrize("where", [0, 1, 2])
@pytest.mark.parametrize("kind", hmm_ref.NONFINITE_KINDS)
def test_non_finite_cases_agree_with_the_oracle(kind, where, N, K):
    """The non-finite cases of the device tests: the oracle (np.max propagates NaN, like torch.max) and hmm_ref (which says so
    explicitly) give the same messages and the same table; so do they for the matrix LogLik hands on unchanged."""
    q, lp, lt, row = hmm_ref.nonfinite_case(kind, where, N, K)
    for qq in (q, hmm_ref.with_infinite_row_max(q, row)):
        with np.errstate(divide="ignore", invalid="ignore"):
            fo, mo = orc.hmm_forward(qq, lp, lt)
            bo = orc.hmm_backward(qq, lt)
            po = orc.hmm_pair_coef(fo, bo, qq, lt)
        f, m = hmm_ref.forward(qq, lp, lt)
        b = hmm_ref.backward(qq, lt)
        assert np.isfinite(f).all() and np.isfinite(b).all()          # nan_to_num leaves nothing non-finite in these cases
        assert close(f, fo) and close(m, mo, atol=0) and close(b, bo)
        assert same_table(hmm_ref.pair_coef(f, b, qq, lt), po, 1e-12)
    r = hmm_ref.local_terms(hmm_ref.with_infinite_row_max(q, row), lp, lt)
    assert np.array_equal(r["qnorm"], hmm_ref.with_infinite_row_max(q, row), equal_nan=True)
    lab, pf, last = cpu_double.hmm_local_terms(torch.as_tensor(r["qnorm"])[None], torch.as_tensor(lp), torch.as_tensor(lt))
    assert np.array_equal(r["labels"], lab[0].numpy()) and np.array_equal(r["pair_first"], pf[0].numpy())
    assert np.allclose(r["last_log"], last[0].numpy(), rtol=RTOL, atol=RTOL)


def test_loglik_rows_conventions():
    nan, inf = np.nan, np.inf
    q = np.array([[-3.0, nan, -1.0], [-2.0, -5.0, -4.0], [nan, 1.0, 2.0], [-inf, -7.0, -inf]])
    out, c = hmm_ref.loglik_rows(q)
    to, tc = cpu_double.loglik_rows(torch.as_tensor(q))
    assert np.array_equal(c, tc.numpy(), equal_nan=True) and np.array_equal(out, to.numpy(), equal_nan=True)
    assert np.isnan(c[0]) and c[1] == -2.0 and np.isnan(c[2]) and c[3] == -7.0 and np.isnan(out[0]).all()
    assert np.array_equal(out[3], [-inf, 0.0, -inf])                 # -inf beside a finite maximum: the normal path
    for bad in (inf, -inf):                                           # any infinite row maximum: the input comes back unchanged
        q2 = q.copy()
        q2[1] = bad
        out, c = hmm_ref.loglik_rows(q2)
        to, tc = cpu_double.loglik_rows(torch.as_tensor(q2))
        assert np.array_equal(out, q2, equal_nan=True) and np.array_equal(out, to.numpy(), equal_nan=True)
        assert np.array_equal(c, tc.numpy(), equal_nan=True) and c[1] == bad


def test_safe_exp_and_clamp_conventions():
    nan, inf = np.nan, np.inf
    x = np.array([[0.0, nan, -1.0], [-inf, -inf, -inf], [1.0, inf, inf], [-inf, 2.0, 1.0]]).astype(hmm_ref.LD)
    e = hmm_ref.safe_exp(x).astype(np.float64)
    assert np.array_equal(e[0], [1e-8] * 3)                          # one NaN poisons its row (torch.max propagates it)
    assert np.array_equal(e[1], [1e-8] * 3)                          # -inf - -inf
    assert np.array_equal(e[2], [0.0, 1e-8, 1e-8])                   # inf - inf, and exp(-inf) beside it
    assert e[3, 0] == 0.0 and e[3, 1] == 1.0 and abs(e[3, 2] - np.exp(-1.0)) < 1e-16
    ref = torch.nan_to_num(torch.exp(torch.as_tensor(x.astype(np.float64)) - torch.max(torch.as_tensor(x.astype(np.float64)), dim=1)[0][:, None]), 1e-8)
    assert np.allclose(e, ref.numpy(), rtol=1e-15, atol=0)
    # the clamps add 1e-4 (they do not floor): two states, the second never entered; log_pi with an impossible first state
    lp = np.array([-inf, 0.0])
    q = np.zeros((2, 2))
    with np.errstate(divide="ignore"):
        lt = np.log(np.array([[1.0, 0.0], [0.5, 0.5]]))
        f, m = hmm_ref.forward(q, lp, lt)
        b = hmm_ref.backward(q, lt)
    assert close(m[0], 1.0 + 1e-4, atol=0) and close(f[0], np.array([1e-4, 1.0]) / (1.0 + 1e-4))
    PiT = np.array([[1.0, 0.5], [1e-4, 1.0]])                        # safe_exp(lt.T) = [[1, .5], [0, 1]], 0 < 1e-6 -> + 1e-4
    assert close(f[1], PiT @ f[0] / (PiT @ f[0]).sum())
    Pi = np.array([[1.0, 1e-4], [1.0, 1.0]])                         # safe_exp(lt) = [[1, 0], [1, 1]], 0 < 1e-5 -> + 1e-4
    v = Pi @ np.ones(2)
    assert close(b[0], v / v[0]) and np.array_equal(b[1], [1.0, 1.0])      # normalised WITHOUT the last state: b[0, 0] = 1
    assert b[0, 0] == 1.0 and b[0].sum() > 1.0


def test_pair_table_and_arg_max_conventions():
    nan, inf = np.nan, np.inf
    Q, lp, lt = hmm_ref.random_case(5, 3, 1, 0)
    r = hmm_ref.local_terms(Q[0], lp, lt)
    assert np.isneginf(r["pair"][0]).all() and r["pair_first"][0] == 0 and np.isfinite(r["pair"][1:]).all()
    assert close(np.exp(r["pair"][1:]).sum(axis=(1, 2)), 1.0, rtol=1e-14)
    assert np.array_equal(r["last_log"], np.log(r["fmsg"][-1]))      # bmsg[-1] = 1
    # den == 0 -> 1e-10: a step nobody can reach keeps -inf, not NaN
    a = np.array([[1.0, 0.0], [0.0, 0.0], [0.5, 0.5]])
    p = hmm_ref.pair_coef(a, np.ones((3, 2)), np.zeros((3, 2)), np.log(np.full((2, 2), 0.5)))
    assert np.isneginf(p[0]).all() and np.isneginf(p[2]).all() and np.isfinite(p[1, 0]).all() and np.isneginf(p[1, 1]).all()
    t = np.array([[1.0, 3.0, 3.0], [nan, 5.0, nan], [-inf, -inf, -inf], [2.0, nan, 9.0], [7.0, 7.0, 1.0]])
    assert np.array_equal(hmm_ref.first_argmax_nan_wins(t), [1, 0, 0, 1, 0])
    assert np.array_equal(hmm_ref.first_argmax_nan_wins(t), torch.argmax(torch.as_tensor(t), dim=1).numpy())
    tab = np.stack([np.full((2, 2), -inf), [[1.0, 4.0], [4.0, 0.0]], [[1.0, nan], [9.0, 0.0]], [[-inf, -inf], [-inf, -3.0]]])
    assert np.array_equal(hmm_ref.pair_first(tab), [0, 1, 0, 3])
    assert np.array_equal(hmm_ref.top_two_gap(t), [0.0, inf, inf, inf, 0.0])
    assert np.array_equal(hmm_ref.top_two_gap(np.array([[1.0, 3.5, -inf], [-inf, 2.0, -inf]])), [2.5, inf])
    f = np.array([[0.25, 0.5, 0.125], [0.0, 0.3, 0.0], [0.2, nan, nan]])
    bm = np.array([[0.5, 0.25, 1.0], [0.4, 0.0, 0.1], [1.0, 1.0, 1.0]])
    lab, resp = hmm_ref.assign(f, bm)
    assert np.array_equal(lab, [0, 0, 1]) and np.array_equal(resp, np.eye(3)[[0, 0, 1]])
    assert np.array_equal(lab, cpu_double.assign(torch.as_tensor(f), torch.as_tensor(bm)).numpy())
