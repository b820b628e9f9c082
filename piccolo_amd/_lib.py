"""ctypes binding of include/piccolo_hip.h (the product's only compute back end), derived from the header's text at import (_header.py):
an entry point, a struct field or a constant is declared there and nowhere else.

There is deliberately NO fallback: if libpiccolo_hip.so is missing or has the wrong ABI, importing the
product's ops raises.  Build it with `python -m piccolo_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import os

from . import build as _build
from ._header import Header, PiccoloHipError  # noqa: F401  (PiccoloHipError is part of this module's surface)

HEADER = os.path.normpath(os.path.join(_build.HERE, "..", "include", "piccolo_hip.h"))     # the file build.py hashes into the library
_H = Header.read(HEADER)

(ABI_VERSION, RESULT_STRIDE, GD_RESULT_STRIDE, GD_SEQUENTIAL, GD_BATCH, GD_MAX_ROOMS, GD_PRUNE_MAX, ROBUST_TRUNC, ROBUST_HUBER,
 PANO_F32, PANO_U8, PANO_F16, PANO_U8P, PANO_U8V) = (_H.constant("PCL_" + name) for name in (
     "ABI_VERSION", "RESULT_STRIDE", "GD_RESULT_STRIDE", "GD_SEQUENTIAL", "GD_BATCH", "GD_MAX_ROOMS", "GD_PRUNE_MAX", "ROBUST_TRUNC", "ROBUST_HUBER",
     "PANO_F32", "PANO_U8", "PANO_F16", "PANO_U8P", "PANO_U8V"))

try:
    GdHyper, GnHyper, GdRoom, AlignParams, AlignOut = (_H.structs[name] for name in (
        "pcl_gd_hyper", "pcl_gn_hyper", "pcl_gd_room", "PclAlignParams", "PclAlignOut"))
except KeyError as e:
    raise PiccoloHipError("%s: no `typedef struct ... %s`" % (HEADER, e.args[0])) from None
ALIGN_OUT_WORDS = ctypes.sizeof(AlignOut) // 8      # the device record pcl_align_vote writes, read back as 8-byte words

SIGNATURES = _H.signatures      # name -> (restype, argtypes); every symbol include/piccolo_hip.h declares

_lib = None


def so_path():
    return os.environ.get("PCL_SO", _build.SO)       # PCL_SO: A/B a differently built library (experiments)


def load():
    """Load libpiccolo_hip.so (never builds implicitly on the hot path; raises if absent)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; import it first so this process has ONE runtime (ours resolves to the
    # already-loaded libamdhip64 by soname).  Loading ours first leaves two runtimes, one of which sees no device.
    import torch  # noqa: F401
    path = so_path()
    if not os.path.exists(path):
        raise PiccoloHipError(
            "piccolo_amd: %s not found. The MI355X HIP library is the only back end (no CPU fallback); "
            "build it with `python -m piccolo_amd.build`." % path)
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)        # AttributeError if the library lacks a declared symbol
        fn.restype, fn.argtypes = res, args
    if lib.pcl_abi_version() != ABI_VERSION:         # was this .so built from this tree's header?
        raise PiccoloHipError("piccolo_amd: ABI mismatch: library %s is %d, %s says %d" % (path, lib.pcl_abi_version(), HEADER, ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise PiccoloHipError("%s failed: %s (code %d)" % (what, load().pcl_error_string(rc).decode(), rc))
