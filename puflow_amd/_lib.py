"""ctypes binding of libpuflow_hip.so (C ABI: include/puflow_hip.h).

Nothing of the ABI is written down here: SIGNATURES (name -> (restype, argtypes)), the descriptor structs (PfEcTrain, ...) and
the header's #define constants (PF_EC_PERSISTENT, ...) are made from the header by _abi.py when this module is imported.

The product path has NO fallback: if the HIP library is missing or a call fails, we raise.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int, c_longlong

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PF_LIB_PATH", os.path.join(_HERE, "libpuflow_hip.so"))   # override: tuning builds only
_lib = None

_CONSTANTS, _STRUCTS, SIGNATURES = _abi.header()
globals().update(_CONSTANTS)
globals().update(_STRUCTS)


class PuflowHipError(RuntimeError):
    pass


def bind(cdll):
    """Give every entry point of a loaded library (the product's or a variant build's) its header types."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(cdll, name)         # AttributeError if a declared symbol is missing
        fn.restype, fn.argtypes = res, args
    return cdll


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PuflowHipError(
            f"{LIB_PATH} not found: build it with `python -m puflow_amd.build` "
            "(or __graft_entry__.build()); there is no CPU fallback.")
    _lib = bind(ctypes.CDLL(LIB_PATH))
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().pf_error_string(rc).decode()
        raise PuflowHipError(f"{what}: {msg} (code {rc})")


def offsets(vals):
    return (c_longlong * len(vals))(*[int(v) for v in vals])


def counts(vals):
    """host int array of the ragged entry points (per-cloud point counts)"""
    return (c_int * len(vals))(*[int(v) for v in vals])
