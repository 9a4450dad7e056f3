"""The finish kernel with bit 3 of its flag word (parameters frozen: a cluster at its estimation limit) through the C-ABI,
against tests/chain_frozen_ref.py (pinned to the reference by tests/test_chain_frozen_ref.py) - whole arenas with NaN guard
words between the buffers, bit for bit, with the arena helpers of tests/test_gpu_chain_glue.py - and the member step on the
frozen level lists against the full lists run with the same flag."""
import numpy as np
import pytest
import torch

import chain_frozen_ref as fz
import test_gpu_chain_glue as glue
from conftest import golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from hdpgpc_amd import member_step

FROZEN_FLAGS = (8, 8 | 1, 8 | 4, 8 | 2 | 4 | 1)


def expect(lay, H, chains, flags):
    E = (H[0].copy(), H[1].copy())
    for c, fl in zip(chains, flags):
        s, inputs, i1, i2 = glue.state_of(lay, E, c)
        glue.store_state(lay, E, c, fz.finish_ref(s, inputs, i1, i2, fl))
    return E


def poison(lay, H, c):
    """What a frozen finish must not read: NaN in part / Snew (whatever it read would end up in W or a row)."""
    for k in glue.INPUT_PAIRS:
        lay.view(H, f"{c}.{k}")[...] = np.nan


@pytest.mark.parametrize("T", [20, 91])       # 91: the first size whose grid-stride loop makes a second pass (test_gpu_chain_glue.py)
def test_frozen_finish_every_flag(T):
    """Stale, non-zero info2 / info1[2..3] and NaN part / Snew change nothing: W, n0 and bad_count[0] stay; a non-zero info1[0]
    or info1[1] still latches bad_count[1]; Nf and pos advance unless the step is a candidate."""
    lay = glue.Layout()
    glue.add_chain(lay, "c", T)
    H = lay.host()
    glue.fill_chain(lay, H, "c", np.random.default_rng(T))
    poison(lay, H, "c")
    D = glue.upload(H)
    cases = [(fl, (0, 0, 3, 9), (5, 1)) for fl in FROZEN_FLAGS] + [(8, (6, 0, 0, 2), (0, 7)), (8 | 2 | 4, (0, 1, 4, 0), (2, 0))]
    for n, (flags, info1, info2) in enumerate(cases):
        pos = (1, 3)[n % 2]
        glue.set_words(lay, H, "c", pos=pos, n0=5.0 + n, Nf=2.0 + n, info1=info1, info2=info2, bad=(n % 3, 0))
        for d, h in zip(D, H):
            d.copy_(torch.from_numpy(h))
        fdev = member_step.upload_descs([glue.finish_desc(lay, D, "c", T, flags)], "cuda")
        assert glue.launch_finish(fdev, 0, 1, T) == 0
        E = expect(lay, H, ["c"], [flags])
        s = glue.state_of(lay, E, "c")[0]
        dry = bool(flags & 2)
        assert s["bad_count"].tolist() == [n % 3, pos + 1 if any(info1[:2]) else 0] and s["n0"] == 5.0 + n
        assert (s["Nf"], s["pos"]) == ((2.0 + n, pos) if dry else (3.0 + n, pos + 1))
        assert np.array_equal(s["W"], lay.view(H, "c.W")) and lay.view(E, "c.sync")[0] == 0
        for k in fz.PARAMS:
            assert np.array_equal(s[k][pos + 1], lay.view(H, f"c.{k}")[pos])
        glue.assert_same_bits(lay, glue.download(D), E)


@pytest.mark.parametrize("T", [20, 91])
def test_batch_of_frozen_and_live_chains(T):
    """Three descriptors in one launch: a frozen annealed chain, a live one, a frozen candidate without the smoother."""
    lay = glue.Layout()
    chains, flags = ["a", "b", "c"], [8 | 1, 1, 8 | 2 | 4]
    for c in chains:
        glue.add_chain(lay, c, T)
    H = lay.host()
    rng = np.random.default_rng(7 + T)
    for i, c in enumerate(chains):
        glue.fill_chain(lay, H, c, rng)
        if flags[i] & 8:
            poison(lay, H, c)
        glue.set_words(lay, H, c, pos=(2, 1, 3)[i], n0=6.0 + i, Nf=3.0 + i, info1=((0, 0, 1, 1), (0, 0, 0, 0), (0, 4, 0, 8))[i],
                       info2=((3, 3), (0, 0), (0, 1))[i], bad=(i, 0))
    D = glue.upload(H)
    fdev = member_step.upload_descs([glue.finish_desc(lay, D, c, T, fl) for c, fl in zip(chains, flags)], "cuda")
    assert glue.launch_finish(fdev, 0, 3, T) == 0
    E = expect(lay, H, chains, flags)
    sa, sb, sc = (glue.state_of(lay, E, c)[0] for c in chains)
    assert (sa["pos"], sa["n0"], sa["Nf"], sa["bad_count"].tolist()) == (3, 6.0, 4.0, [0, 0])
    assert (sb["pos"], sb["n0"], sb["Nf"], sb["bad_count"].tolist()) == (2, 8.0, 5.0, [1, 0])
    assert (sc["pos"], sc["n0"], sc["Nf"], sc["bad_count"].tolist()) == (3, 8.0, 5.0, [2, 4])
    glue.assert_same_bits(lay, glue.download(D), E)


# ------------------------------------------------------------------------------------------ frozen lists against full lists
def _model(T, n):
    from hdpgpc_amd.GPI import RBFWhiteKernel
    from hdpgpc_amd.GPI_model import GPI_model
    y90 = golden("mitbih100_lead0.npz")["y"][:n + 1]
    t = np.linspace(0, y90.shape[1] - 1, T)
    y = np.stack([np.interp(t, np.arange(y90.shape[1]), r) for r in y90])
    m = GPI_model(RBFWhiteKernel(300.0, 3.0, 9e-5), np.arange(float(T))[:, None], annealing=True, bayesian=True, free_deg_MNIV=5)
    cond = m.GPR_dynamic(12.0, 9.0)
    m.initial_conditions(ini_A=cond[0], ini_Gamma=cond[1], ini_C=cond[2], ini_Sigma=cond[3])
    m.fixed_theta, m.noise_bounds = (341.0, 1.2, 4.66), (9e-5, 18.0)
    x = np.repeat(np.arange(float(T))[None, :, None], n, axis=0)
    m.full_pass_weighted(x, y[:n, :, None], torch.ones(n), use_graphs=False)
    return m, torch.as_tensor(y[n], device=m.device).reshape(1, T).contiguous()


def _one_step(m, y, frozen_lists):
    from hdpgpc_amd import chain_batch
    T, dev = m.x_basis.shape[0], m.device
    ch = member_step.Chain.from_model(m, len(m.f_star) + 2)
    ch.ws = torch.empty(member_step.ws_size(T), dtype=torch.float64, device=dev)
    ch.bad = torch.zeros(2, dtype=torch.int32, device=dev)
    ch.sync = torch.zeros(1, dtype=torch.int32, device=dev)
    ch.Y, ch.y_row0 = y, int(ch.pos[0])
    sh = member_step.shared_buffers(1, T, dev)
    for k in ("S__", "S_", "Zs", "Y3"):
        sh[k].fill_(float("nan"))                     # what the frozen lists leave alone the frozen finish must not read
    sh["i2"].fill_(3)
    ch.build_lists(sh, 0, frozen=frozen_lists)
    gdev = member_step.upload_descs([member_step.gather_desc(ch)], dev)
    fdev = member_step.upload_descs([member_step.finish_desc(ch, 1 | 8, ch.bad)], dev)
    member_step.member_step(chain_batch._MergedLevels([ch]), sh, gdev, fdev, 0, 1, T, frozen=frozen_lists)
    torch.cuda.synchronize()
    return ch


@pytest.mark.parametrize("T", [20, 144])       # 144: cooperative inversions, the right-hand sides one list level behind them
def test_frozen_lists_equal_full_lists_with_flag_8(T):
    m, y = _model(T, 4)
    pos = len(m.f_star) - 1
    full, frz = _one_step(m, y, False), _one_step(m, y, True)
    assert len(frz.lv) < len(full.lv) or T <= 128
    assert sum(len(l_._items) for l_ in frz.lv) == sum(len(l_._items) for l_ in full.lv) - (12 if T > 128 else 10)
    for ch in (full, frz):
        assert int(ch.pos[0]) == pos + 1 and ch.bad.tolist() == [0, 0] and float(ch.Nf[0]) == 5.0
    for k in ("F", "Fsm", "P", "Psm"):
        a, b = getattr(full, k)[pos:pos + 2], getattr(frz, k)[pos:pos + 2]
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
    assert not torch.equal(frz.Fsm[pos].reshape(-1), m.f_star_sm[pos].reshape(-1))      # the smoother did rewrite the previous state
    for k in ("A", "G", "C", "S"):
        assert torch.equal(getattr(frz, k)[pos + 1], getattr(frz, k)[pos]) and torch.equal(getattr(frz, k), getattr(full, k))
    assert torch.equal(frz.W, full.W) and float(frz.n0[0]) == float(full.n0[0]) == float(m.internal_params.n0)
