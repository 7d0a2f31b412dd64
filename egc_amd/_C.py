"""ctypes binding of libegc_hip.so (the C ABI declared in include/egc_hip.h).

The header is the one owner of the ABI: its constants (``EGC_X`` becomes ``_C.X``, enum members included), its structs
(``egc_graph`` becomes ``EgcGraph``) and the prototypes behind ``SYMBOLS`` are read from it when this module is imported
(egc_amd/_abi.py); nothing of them is restated here.

There is NO CPU fallback: if the shared library is missing or cannot be loaded, every entry point
raises RuntimeError.  Build it with ``egc_amd/csrc/build.sh`` (or ``__graft_entry__.build()``).
"""
from __future__ import annotations

import ctypes as C
import os

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("EGC_HIP_LIB") or os.path.join(_HERE, "lib", "libegc_hip.so")
_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "egc_hip.h")
_lib = None


def _read_abi() -> _abi.Abi:
    if not os.path.exists(_HEADER_PATH):
        raise RuntimeError(f"egc_amd: the public header {_HEADER_PATH} is missing: the binding's prototypes, structs and "
                           "constants are read from it")
    with open(_HEADER_PATH) as f:
        return _abi.read_header(f.read())


ABI = _read_abi()
globals().update({name[len("EGC_"):]: value for name, value in ABI.constants.items()})
EGC_MAX_AGGRS = ABI.constants["EGC_MAX_AGGRS"]
_STATUS = {value: name for name, value in ABI.enums["egc_status"].items() if value != 0}

EgcGraph, EgcLayer, EgcPost, EgcTypedRel, EgcHead, EgcCollateField, EgcCollateFields, EgcCollateStore, EgcCollateOut = (
    ABI.structs[name] for name in ("egc_graph", "egc_layer", "egc_post", "egc_typed_rel", "egc_head", "egc_collate_field",
                                   "egc_collate_fields", "egc_collate_store", "egc_collate_out"))

# name -> (restype, argtypes): exactly the symbols include/egc_hip.h declares
SYMBOLS = ABI.prototypes

_ENV_DATA = getattr(os.environ, "_data", None)     # CPython on POSIX: the bytes dict behind os.environ


def env_flag(name: str) -> bool:
    """True when the environment variable is set to something other than "" / "0" -- read on every call (tests and
    notebooks flip these), but through the bytes dict behind os.environ where CPython has one: os.environ.get costs
    1.5 us per lookup (key encoding + value decoding), four of them were a quarter of an eval-mode layer call."""
    if _ENV_DATA is not None:
        v = _ENV_DATA.get(name.encode())
        return v is not None and v not in (b"", b"0")
    return os.environ.get(name, "0") not in ("", "0")


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load libegc_hip.so once; raise RuntimeError (never fall back) if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"egc_amd: HIP library not built: {_LIB_PATH} is missing. Run egc_amd/csrc/build.sh "
            "(hipcc, --offload-arch=gfx950). There is no CPU fallback.")
    try:
        lib = C.CDLL(_LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the host
        raise RuntimeError(f"egc_amd: cannot load {_LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError here == header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status: int, what: str):
    if status != 0:
        detail = load().egc_last_error().decode() if status == 3 else ""
        raise RuntimeError(f"egc_amd: {what} failed with {_STATUS.get(status, status)} {detail}".rstrip())


def make_layer(in_channels, out_channels, num_heads, num_bases, aggr_codes, agg_set, sym_set, loops_all_nodes,
               weight_layout, weight_act, basis_stride=0) -> EgcLayer:
    if len(aggr_codes) > EGC_MAX_AGGRS:
        raise RuntimeError(f"egc_amd: at most {EGC_MAX_AGGRS} aggregators are supported")
    arr = (C.c_int32 * EGC_MAX_AGGRS)(*(list(aggr_codes) + [0] * (EGC_MAX_AGGRS - len(aggr_codes))))
    return EgcLayer(in_channels, out_channels, num_heads, num_bases, len(aggr_codes), arr, agg_set, sym_set,
                    int(loops_all_nodes), weight_layout, weight_act, int(basis_stride))
