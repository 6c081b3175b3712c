"""ctypes binding of libdiffsal_hip.so, derived at import from the C ABI declared in include/diffsal.h: argument lists, struct
layouts, constants and the ABI version are read from the header (_cdecl.py), none is restated here.

The library is the product path: if it is missing or does not load, importing the ops fails
loudly -- there is no PyTorch/CPU fallback.
"""
import ctypes as C
import os

from . import _cdecl
from . import build as _build

_LIB = None

try:
    with open(_build.HEADER) as _f:
        _H = _cdecl.parse(_f.read())
except OSError as e:
    raise ImportError(f"{_build.HEADER} cannot be read ({e}): the binding of libdiffsal_hip.so is derived from that header, "
                      "which ships with the package") from e
K = _H.constants      # every enumerator and `#define DIFFSAL_X <integer>` of the header


def constants(prefix, names):
    """Values of the header's DIFFSAL_<prefix><name> for the space-separated ``names``; a name the header lacks is a KeyError."""
    return [K["DIFFSAL_" + prefix + n] for n in names.split()]


# the two structs the host fills and passes by reference, the element of diffsal_pack_weight_many's device job table and the
# element of diffsal_resample_u8_groups' host array
_STRUCTS = dict.fromkeys(_H.structs)
ConvDesc = _cdecl.structure("ConvDesc", _H.structs["diffsal_conv_desc"], _STRUCTS, "struct diffsal_conv_desc (include/diffsal.h).")
Wino4Ext = _cdecl.structure("Wino4Ext", _H.structs["diffsal_wino4_ext"], _STRUCTS,
                            "struct diffsal_wino4_ext (include/diffsal.h): optional extras of diffsal_conv_wino4.")
PackJob = _cdecl.structure("PackJob", _H.structs["diffsal_pack_job"], _STRUCTS, "struct diffsal_pack_job (include/diffsal.h).")
ResampleGroup = _cdecl.structure("ResampleGroup", _H.structs["diffsal_resample_group"], _STRUCTS,
                                 "struct diffsal_resample_group (include/diffsal.h): a host array of them is passed as c_void_p.")
_STRUCTS.update(diffsal_conv_desc=ConvDesc, diffsal_wino4_ext=Wino4Ext)

# the header's value; diffsal_version() is the one the loaded binary was compiled with.  load() refuses a binary whose value
# differs, so that a stale libdiffsal_hip.so is never called with the current argument lists
ABI_VERSION = K["DIFFSAL_ABI_VERSION"]

# name -> (restype, argtypes) of every prototype in the header.  Device pointers travel as integers (c_void_p), and so do host
# arrays: c_void_p takes a ctypes array, a byref() result or None
SIGNATURES = {name: (_cdecl.ctype(res, _STRUCTS), [_cdecl.ctype(a, _STRUCTS) for a in args])
              for name, (res, args) in _H.prototypes.items()}

(WS_GROUPNORM, WS_CONV_IGEMM, WS_CONV_WINO4, WS_CONV_WINO4_STATS, WS_CONV_WGRAD, WS_WGRAD_SEGMENTED, WS_TAPSUM_BWD,
 WS_SALIENCY_METRICS, WS_ATTENTION_TAIL, WS_ATTENTION_BWD_QTAIL, WS_ATTENTION_BWD_DS) = constants(
    "WS_", "GROUPNORM CONV_IGEMM CONV_WINO4 CONV_WINO4_STATS CONV_WGRAD WGRAD_SEGMENTED TAPSUM_BWD SALIENCY_METRICS "
           "ATTENTION_TAIL ATTENTION_BWD_QTAIL ATTENTION_BWD_DS")


def workspace_bytes(op: int, desc=None, dims=()):
    """``diffsal_workspace_bytes``: scratch bytes of operator ``op`` (WS_*) for a descriptor and / or a tuple of integers."""
    arr = (C.c_long * len(dims))(*[int(v) for v in dims]) if dims else None
    return load().diffsal_workspace_bytes(op, C.byref(desc) if desc is not None else None, arr, len(dims))


ACT_NONE, ACT_RELU, ACT_GELU, ACT_SIGMOID = constants("ACT_", "NONE RELU GELU_ERF SIGMOID")
ACT_GELU_GRAD = K["DIFFSAL_ACT_GELU_GRAD"]      # training only: product * gelu'(residual) (include/diffsal.h)
PREC_FP32, PREC_BF16X3 = constants("PREC_", "FP32 BF16X3")
F32, BF16, F16 = constants("", "F32 BF16 F16")


def library_path():
    return _build.LIB


def load():
    """dlopen the HIP library (building it first if sources are newer); raises if impossible."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.LIB
    if not os.path.exists(path) or (_build.needs_build() and os.environ.get("DIFFSAL_NO_REBUILD") != "1"):
        try:
            _build.build_library()
        except Exception as e:  # noqa: BLE001
            # never bind the current signatures to a binary older than its sources: a changed argument list would be
            # silent memory corruption on the GPU.  DIFFSAL_NO_REBUILD=1 opts out (the ABI version is still checked).
            raise RuntimeError(
                f"libdiffsal_hip.so is {'stale' if os.path.exists(path) else 'missing'} and could not be built ({e}); "
                "run `python -m diff_sal_amd.build` (or set DIFFSAL_NO_REBUILD=1 to load the existing binary as is)"
            ) from e
    # PyTorch bundles its own libamdhip64 (same soname as /opt/rocm's).  Import it first so that ONE HIP
    # runtime lives in the process and streams / device pointers are shared with torch.
    import torch  # noqa: F401

    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    got = lib.diffsal_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{path} reports ABI version {got}, include/diffsal.h declares {ABI_VERSION}: "
                           "rebuild with `python -m diff_sal_amd.build --force`")
    _LIB = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().diffsal_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libdiffsal_hip {what} failed (code {rc}): {msg}")


TUNING_EPOCH = [0]      # bumped by set_tuning: host-side caches of the library's planner answers key on it


def set_tuning(name: str, value) -> None:
    """Set a test / tuning switch of the library (include/diffsal.h: diffsal_set_tuning); None or a negative value unsets it."""
    check(load().diffsal_set_tuning(name.encode(), -1 if value is None else int(value)), "set_tuning")
    TUNING_EPOCH[0] += 1


def get_tuning(name: str) -> int:
    return load().diffsal_get_tuning(name.encode())
