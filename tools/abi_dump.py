#!/usr/bin/env python3
"""CPU: the ctypes binding of libpuflow_hip.so as `puflow_amd._lib` presents it, as text.
  - every symbol of `_lib.SIGNATURES`, sorted: name, restype, and per argument the scalar ctypes type or `ptr`;
  - every `ctypes.Structure` class of `_lib`, sorted: sizeof, then `name offset size` per field.
Public surface only, so the same file runs against two trees: `abi_dump.py [DIR]`, DIR = the directory that holds the other
tree's `puflow_amd` (default: this repository).  Identical text = same binding (`profiles/refactor_abi/`)."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from puflow_amd import _lib


def kind(t):
    return "ptr" if issubclass(t, (ctypes.c_void_p, ctypes._Pointer)) else t.__name__


for name, (res, args) in sorted(_lib.SIGNATURES.items()):
    print(name, res.__name__, "(" + ", ".join(kind(a) for a in args) + ")")
for name, cls in sorted(vars(_lib).items()):
    if isinstance(cls, type) and issubclass(cls, ctypes.Structure):
        print(f"struct {name} sizeof {ctypes.sizeof(cls)}")
        for field, _ in cls._fields_:
            print(f"  {field} {getattr(cls, field).offset} {getattr(cls, field).size}")
