"""ctypes binding of libhdpgpc_hip.so, read from include/hdpgpc_hip.h: the header is the one statement of the boundary.

Signatures, struct layouts and the integer #defines all come from parse_header(); an entry point is added by declaring it
there and wrapping it in ops.py.  The library's further headers (HEADERS below) are bound the same way, each into an export table
of its own; EXPORTS stays the main header's list.  The product path has no CPU fallback: importing this module without the
built library raises.
"""
import ctypes
import os

import torch  # noqa: F401  (first: the library must bind to the HIP runtime PyTorch-ROCm already loaded, not a second copy)

from ._cheader import parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# HGP_LIB selects another build of the same library (only the diagnostic `make stamps` build uses it)
LIB_PATH = os.environ.get("HGP_LIB") or os.path.join(_HERE, "lib", "libhdpgpc_hip.so")
_INCLUDE = os.path.join(os.path.dirname(_HERE), "include")                          # where csrc/hgp_internal.hpp includes them from
# (exports attribute of this module, header file): the main header first, then the kernel fit, the MDS embedding, ragged pair
# batches, ragged projection, the pair path with a segment-operator store and the static filter chain
HEADERS = (("EXPORTS", "hdpgpc_hip.h"), ("FIT_EXPORTS", "hdpgpc_hip_fit.h"), ("MDS_EXPORTS", "hdpgpc_hip_mds.h"),
           ("RAGGED_EXPORTS", "hdpgpc_hip_ragged.h"), ("PROJECT_EXPORTS", "hdpgpc_hip_project.h"),
           ("SEGOPS_EXPORTS", "hdpgpc_hip_segops.h"), ("STATIC_EXPORTS", "hdpgpc_hip_static.h"))
HEADER_PATH = os.path.join(_INCLUDE, HEADERS[0][1])

c_dp = ctypes.c_void_p  # device pointers travel as integers


def check_abi(library, header):
    """hgp_abi_version() of the loaded library against HGP_ABI_VERSION of the header it is bound from."""
    if library != header:
        raise ImportError(f"{LIB_PATH} reports ABI version {library}, include/hdpgpc_hip.h declares {header}: "
                          "library built from another header: rebuild")


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). hdpgpc_amd has no CPU fallback.")
    paths = [os.path.join(_INCLUDE, header) for _, header in HEADERS]
    for path in paths:
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: the binding of {LIB_PATH} is read from it. hdpgpc_amd runs from its source tree.")
    lib = ctypes.CDLL(LIB_PATH)
    exports, structs, defines = {}, {}, {}
    for (attr, _), path in zip(HEADERS, paths):
        with open(path) as f:
            funcs, s, d = parse_header(f.read())
        for name, (res, args) in funcs.items():
            fn = getattr(lib, name)  # AttributeError here = header and library disagree
            fn.restype = res
            fn.argtypes = args
        exports[attr] = sorted(funcs)
        structs.update(s)
        defines.update(d)
    check_abi(lib.hgp_abi_version(), defines["HGP_ABI_VERSION"])
    return lib, exports, structs, defines


def _struct(name, c_name):
    return type(name, (ctypes.Structure,), {"_fields_": _structs[c_name], "__doc__": f"{c_name} of include/hdpgpc_hip.h."})


lib, _exports, _structs, _defines = _load()
globals().update(_exports)          # EXPORTS, FIT_EXPORTS, MDS_EXPORTS, RAGGED_EXPORTS, PROJECT_EXPORTS, SEGOPS_EXPORTS, STATIC_EXPORTS: sorted names, one list per header
FIT_STATE_DOUBLES, MDS_STATE_DOUBLES = _defines["HGP_FIT_STATE_DOUBLES"], _defines["HGP_MDS_STATE_DOUBLES"]
ABI_VERSION, MAX_T_WAVE, MAX_T_COOP = (_defines[k] for k in ("HGP_ABI_VERSION", "HGP_MAX_T_WAVE", "HGP_MAX_T_COOP"))
GemmItem, ChainGatherDesc = _struct("GemmItem", "hgp_gemm_item"), _struct("ChainGatherDesc", "hgp_chain_gather_desc")
ChainFinishDesc, CopyItem = _struct("ChainFinishDesc", "hgp_chain_finish_desc"), _struct("CopyItem", "hgp_copy_item")
StaticChainDesc = _struct("StaticChainDesc", "hgp_static_chain_desc")


class HgpError(RuntimeError):
    pass


def check(rc, what):
    if rc == 0:
        return
    if rc == -1:
        raise ValueError(f"{what}: bad argument")
    if rc == -2:
        raise NotImplementedError(f"{what}: size not supported by this build")
    raise HgpError(f"{what}: HIP error {rc - 1000}")
