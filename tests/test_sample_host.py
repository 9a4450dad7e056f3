"""Host-side checks of the state-sampling entry (hgp_sample_states_f64): declared, bound, and validating its arguments
before any HIP call.  No GPU needed."""
import ctypes
import os

import pytest

from test_abi_exports import LIB, header_symbols

ENTRY = "hgp_sample_states_f64"


def test_header_declares_the_entry():
    assert ENTRY in header_symbols()


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_binding_and_argument_validation():
    from hdpgpc_amd import _ffi
    assert ENTRY in _ffi.EXPORTS and set(_ffi.EXPORTS) == set(header_symbols())
    fn = _ffi.lib.hgp_sample_states_f64
    p = ctypes.c_void_p(64)          # never dereferenced: every call below returns before the first launch
    big = 1 << 40                    # a workspace size that no check below finds too small
    #          mean cov idx   T  S  z  n  shared jitter out info ws ws_bytes stream
    assert fn(p, p, None, 90, 0, p, 10, 1, 0.0, p, p, p, big, None) == 0         # S = 0: nothing to do
    assert fn(p, p, None, 90, 3, p, 0, 1, 0.0, p, p, p, big, None) == 0          # n = 0: nothing to do
    assert fn(None, None, None, 90, 0, None, 10, 0, 0.0, None, None, None, 0, None) == 0
    assert fn(None, None, None, 90, 3, None, 0, 0, 0.0, None, None, None, 0, None) == 0
    for hole in (0, 1, 5, 9, 10, 11):                                            # a NULL among the required pointers
        args = [p, p, None, 90, 2, p, 10, 1, 0.0, p, p, p, big, None]
        args[hole] = None
        assert fn(*args) == -1, hole
    assert fn(p, p, p, 90, 2, p, 10, 0, 1e-8, p, p, None, big, None) == -1       # no workspace
    assert fn(p, p, None, 90, -1, p, 10, 1, 0.0, p, p, p, big, None) == -1
    assert fn(p, p, None, 90, 2, p, -1, 1, 0.0, p, p, p, big, None) == -1
    assert fn(p, p, None, 0, 2, p, 10, 1, 0.0, p, p, p, big, None) == -1
    assert fn(p, p, None, 257, 2, p, 10, 1, 0.0, p, p, p, big, None) == -2       # beyond HGP_MAX_T_COOP
    assert fn(p, p, None, 257, 2, p, 10, 1, 0.0, p, p, p, 0, None) == -2         # ... reported before a workspace too small


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
@pytest.mark.parametrize("T", [16, 129])
def test_workspace_one_byte_short_is_refused(T):
    """Everything else valid: -1, and with no GPU on this tier that is also before any HIP call."""
    from hdpgpc_amd import _ffi
    p = ctypes.c_void_p(64)
    need = _ffi.lib.hgp_sample_states_ws_bytes(2, T)
    assert need > 0
    assert _ffi.lib.hgp_sample_states_f64(p, p, None, T, 2, p, 10, 1, 0.0, p, p, p, need - 1, None) == -1


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")
def test_workspace_size_matches_the_header():
    from hdpgpc_amd import ops
    assert ops.sample_ws_doubles(16, 90) == 16 * 90 * 90 + 16
    assert ops.sample_ws_doubles(3, 129) == 3 * 129 * 129 + 3
