"""A caller-provided workspace of exactly the bytes a size function reports, between two guard pads: the tests that call an
entry point directly hand it the pointer behind the first pad and check afterwards that neither pad has changed a bit."""
import ctypes

import torch

PAD = 256                              # doubles on either side
NAN_BITS = 0x7FF8DEADBEEF0001          # a quiet NaN no arithmetic produces: the pads and the workspace start as this


def guarded(need, device):
    """(the whole buffer, the pointer `need` bytes of workspace start at)"""
    assert need > 0 and need % 8 == 0
    buf = torch.full((PAD + need // 8 + PAD,), NAN_BITS, dtype=torch.int64, device=device).view(torch.float64)
    return buf, ctypes.c_void_p(buf.data_ptr() + 8 * PAD)


def assert_pads_untouched(buf):
    bits = buf.view(torch.int64)
    assert bool((bits[:PAD] == NAN_BITS).all()) and bool((bits[-PAD:] == NAN_BITS).all())


def assert_same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    as_int = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t  # noqa: E731
    assert torch.equal(as_int(got), as_int(want))
