"""ctypes binding of libhdpgpc_hip.so, read from include/hdpgpc_hip.h: the header is the one statement of the boundary.

Signatures, struct layouts and the integer #defines all come from parse_header(); an entry point is added by declaring it
there and wrapping it in ops.py.  include/hdpgpc_hip_fit.h (the batched kernel fit) is a second header of the same library, bound
into a table of its own (FIT_EXPORTS), and so are include/hdpgpc_hip_mds.h (the MDS embedding, MDS_EXPORTS) and
include/hdpgpc_hip_ragged.h (the pair path for segments of different lengths, RAGGED_EXPORTS) and include/hdpgpc_hip_project.h
(projection of ragged batches onto the basis grid, PROJECT_EXPORTS); EXPORTS stays the main header's list.  The product path has no CPU fallback: importing this module without the built library raises.
"""
import ctypes
import os

import torch  # noqa: F401  (first: the library must bind to the HIP runtime PyTorch-ROCm already loaded, not a second copy)

from ._cheader import parse_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# HGP_LIB selects another build of the same library (only the diagnostic `make stamps` build uses it)
LIB_PATH = os.environ.get("HGP_LIB") or os.path.join(_HERE, "lib", "libhdpgpc_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hdpgpc_hip.h")     # where csrc/hgp_internal.hpp includes it from
FIT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hdpgpc_hip_fit.h")  # the kernel fit: a header and a table of its own
MDS_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hdpgpc_hip_mds.h")  # the MDS embedding: likewise
RAGGED_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hdpgpc_hip_ragged.h")  # ragged pair batches: likewise
PROJECT_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "hdpgpc_hip_project.h")  # ragged projection: likewise

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
    for path in (HEADER_PATH, FIT_HEADER_PATH, MDS_HEADER_PATH, RAGGED_HEADER_PATH, PROJECT_HEADER_PATH):
        if not os.path.exists(path):
            raise ImportError(f"{path} is missing: the binding of {LIB_PATH} is read from it. hdpgpc_amd runs from its source tree.")
    with open(HEADER_PATH) as f:
        funcs, structs, defines = parse_header(f.read())
    with open(FIT_HEADER_PATH) as f:
        fit_funcs, _, fit_defines = parse_header(f.read())
    with open(MDS_HEADER_PATH) as f:
        mds_funcs, _, mds_defines = parse_header(f.read())
    with open(RAGGED_HEADER_PATH) as f:
        ragged_funcs, _, _ = parse_header(f.read())
    with open(PROJECT_HEADER_PATH) as f:
        project_funcs, _, _ = parse_header(f.read())
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in {**funcs, **fit_funcs, **mds_funcs, **ragged_funcs, **project_funcs}.items():
        fn = getattr(lib, name)  # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    check_abi(lib.hgp_abi_version(), defines["HGP_ABI_VERSION"])
    return (lib, sorted(funcs), structs, defines, sorted(fit_funcs), fit_defines, sorted(mds_funcs), mds_defines, sorted(ragged_funcs),
            sorted(project_funcs))


def _struct(name, c_name):
    return type(name, (ctypes.Structure,), {"_fields_": _structs[c_name], "__doc__": f"{c_name} of include/hdpgpc_hip.h."})


(lib, EXPORTS, _structs, _defines, FIT_EXPORTS, _fit_defines, MDS_EXPORTS, _mds_defines, RAGGED_EXPORTS,
 PROJECT_EXPORTS) = _load()
FIT_STATE_DOUBLES = _fit_defines["HGP_FIT_STATE_DOUBLES"]
MDS_STATE_DOUBLES = _mds_defines["HGP_MDS_STATE_DOUBLES"]
ABI_VERSION, MAX_T_WAVE, MAX_T_COOP = (_defines[k] for k in ("HGP_ABI_VERSION", "HGP_MAX_T_WAVE", "HGP_MAX_T_COOP"))
GemmItem, ChainGatherDesc = _struct("GemmItem", "hgp_gemm_item"), _struct("ChainGatherDesc", "hgp_chain_gather_desc")
ChainFinishDesc, CopyItem = _struct("ChainFinishDesc", "hgp_chain_finish_desc"), _struct("CopyItem", "hgp_copy_item")


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
