"""Host-side checks of the predictive-bands entry (hgp_pred_bands_f64): declared, bound, and validating its arguments
before any HIP call.  No GPU needed."""
import ctypes
import os

import pytest

from test_abi_exports import LIB, header_symbols

ENTRY = "hgp_pred_bands_f64"


def test_header_declares_the_entry():
    assert ENTRY in header_symbols()


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_binding_and_argument_validation():
    from hdpgpc_amd import _ffi
    assert ENTRY in _ffi.EXPORTS and set(_ffi.EXPORTS) == set(header_symbols())
    fn = _ffi.lib.hgp_pred_bands_f64
    p = ctypes.c_void_p(64)          # never dereferenced: every call below returns before the first launch
    big = 1 << 40                    # a workspace size that no check below finds too small
    assert fn(p, 90, p, p, p, None, 0, p, 10, p, p, p, p, big, None) == 0            # S = 0: nothing to do
    assert fn(None, 90, None, None, None, None, 0, None, 10, None, None, None, None, 0, None) == 0
    assert fn(None, 90, p, p, p, None, 2, p, 10, p, p, p, p, big, None) == -1        # NULL pointers
    assert fn(p, 90, p, p, p, None, 2, p, 10, p, p, p, None, big, None) == -1        # no workspace
    assert fn(p, 90, p, p, p, None, -1, p, 10, p, p, p, p, big, None) == -1
    assert fn(p, 0, p, p, p, None, 2, p, 10, p, p, p, p, big, None) == -1
    assert fn(p, 257, p, p, p, None, 2, p, 10, p, p, p, p, big, None) == -2          # beyond HGP_MAX_T_COOP
    assert fn(p, 257, p, p, p, None, 2, p, 10, p, p, p, p, 0, None) == -2            # ... reported before a workspace too small


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
@pytest.mark.parametrize("T", [16, 129])
def test_workspace_one_byte_short_is_refused(T):
    """Everything else valid: -1, and with no GPU on this tier that is also before any HIP call."""
    from hdpgpc_amd import _ffi
    p = ctypes.c_void_p(64)
    need = _ffi.lib.hgp_pred_bands_ws_bytes(2, T)
    assert need > 0
    assert _ffi.lib.hgp_pred_bands_f64(p, T, p, p, p, None, 2, p, 10, p, p, p, p, need - 1, None) == -1


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_workspace_size_matches_the_header():
    from hdpgpc_amd import ops
    assert ops.pred_bands_ws_doubles(16, 90) == 2 * 16 * 90 * 90 + 5 * 16
    assert ops.pred_bands_ws_doubles(3, 129) == 3 * 3 * 129 * 129 + 5 * 3
