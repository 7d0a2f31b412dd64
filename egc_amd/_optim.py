"""ctypes binding of the optimizer entry points of libegc_hip.so (the C ABI declared in include/egc_optim.h).

The second public header has a table of its own, next to ``_C.SYMBOLS`` and read the same way (egc_amd/_abi.py): its
constants (``EGC_ADAM_X`` becomes ``_optim.ADAM_X``), its struct and the prototypes behind ``SYMBOLS``.  ``load()`` binds
them on the library ``_C.load()`` loaded and fails, as that does, where the library lacks a symbol the header declares.
"""
from __future__ import annotations

import os

from . import _C, _abi

_HEADER_PATH = os.path.join(os.path.dirname(_C._HEADER_PATH), "egc_optim.h")
_bound = None


def _read_abi() -> _abi.Abi:
    if not os.path.exists(_HEADER_PATH):
        raise RuntimeError(f"egc_amd: the public header {_HEADER_PATH} is missing: the optimizer binding's prototypes, struct "
                           "and constants are read from it")
    with open(_HEADER_PATH) as f:
        return _abi.read_header(f.read())


ABI = _read_abi()
globals().update({name[len("EGC_"):]: value for name, value in ABI.constants.items()})
EgcAdamTensor = ABI.structs["egc_adam_tensor"]

# name -> (restype, argtypes): exactly the symbols include/egc_optim.h declares
SYMBOLS = ABI.prototypes


def load():
    """libegc_hip.so with the symbols of include/egc_optim.h bound (once); RuntimeError if the library is not there."""
    global _bound
    if _bound is None:
        lib = _C.load()
        for name, (restype, argtypes) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError here == header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        _bound = lib
    return _bound
