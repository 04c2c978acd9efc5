"""The C ABI as ctypes sees it, read from include/puflow_hip.h: its #define constants, its structs and its prototypes.

The header is the only place where an entry point, a descriptor field or a flag value is written down.  Its style is narrow
enough for regular expressions, and `parse` raises on anything outside that style: a declaration is never skipped.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_void_p

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "puflow_hip.h")
# char, unsigned char and void exist only behind pointers
SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong}
POINTEES = dict(SCALARS, **{"char": ctypes.c_char, "unsigned char": ctypes.c_ubyte, "void": None})
BY_VALUE = tuple(SCALARS.values())


class AbiError(ValueError):
    pass


@functools.lru_cache(maxsize=None)
def pointer_to(elem):
    """argtype of a pointer argument.  The header cannot tell host from device pointers, so it takes None, an address (int: a
    device pointer, ndarray.ctypes.data, addressof()) or a ctypes array / pointer() / byref() of `elem`, and raises on storage of
    another type.  elem None = void*: plain c_void_p, which takes any of these."""
    if elem is None:
        return c_void_p
    address = c_void_p.from_param

    def from_param(cls, v):
        if v is None or isinstance(v, int):
            return address(v)
        obj = getattr(v, "_obj", None)                        # byref(obj)
        if (type(obj) if obj is not None else getattr(v, "_type_", None)) is not elem:
            raise TypeError(f"expected None, an address or ctypes {elem.__name__} storage, got {type(v if obj is None else obj).__name__}")
        return v
    return type("ptr_" + elem.__name__, (c_void_p,), {"from_param": classmethod(from_param), "elem": elem})


def _int(expr, where):
    if not re.fullmatch(r"(?:\d+|<<|[-+*|()\s])+", expr):
        raise AbiError(f"{where}: not an integer expression: {expr!r}")
    try:
        return int(eval(expr, {"__builtins__": {}}))
    except Exception as e:
        raise AbiError(f"{where}: not an integer expression: {expr!r}") from e


def _type(spec, known, where):
    """'const float* const*' -> (ctypes type of the base or a struct class or None for void, number of stars)"""
    base = " ".join(re.sub(r"\bconst\b|\*", " ", spec).split())
    if base not in known:
        raise AbiError(f"{where}: unknown type {base!r}")
    return known[base], spec.count("*")


_ARG = re.compile(r"\s*([\w\s*]+?)\s*\b(\w+)\s*")


def _arg(spec, known, where, seen):
    m = _ARG.fullmatch(spec)
    if not m:
        raise AbiError(f"{where}: malformed argument {spec!r}")
    if m.group(1) not in seen:                                # a few dozen distinct types in 1 250 arguments
        t, stars = _type(m.group(1), known, where)
        if not stars and t not in BY_VALUE:
            raise AbiError(f"{where}: {spec!r} passes a {m.group(1)} by value")
        seen[m.group(1)] = t if not stars else pointer_to(t if stars == 1 else c_void_p)
    return seen[m.group(1)]


def _fields(body, consts, where):
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"[\w\s*]+\(\s*\*\s*(\w+)\s*\)\s*\([\w\s*,]*\)", stmt)      # function pointer
        if m:
            fields.append((m.group(1), c_void_p))
            continue
        first, *more = stmt.split(",")
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(\w+)\s*(?:\[(\w+)\])?", first)
        if not m:
            raise AbiError(f"{where}: malformed declarator {stmt!r}")
        base, stars = _type(m.group(1), POINTEES, where)
        decl = [(stars, m.group(2), m.group(3))]
        for d in more:
            m = re.fullmatch(r"\s*(\**)\s*(\w+)\s*(?:\[(\w+)\])?\s*", d)
            if not m:
                raise AbiError(f"{where}: malformed declarator {d!r} in {stmt!r}")
            decl.append((len(m.group(1)), m.group(2), m.group(3)))
        for stars, name, n in decl:
            t = c_void_p if stars else base
            if t not in BY_VALUE + (c_void_p,):
                raise AbiError(f"{where}: field {name!r} of {stmt!r} is no scalar and no pointer")
            if n is not None:
                t = t * (consts[n] if n in consts else _int(n, where))
            fields.append((name, t))
    return fields


def parse(text):
    """-> (constants {name: int}, structs {name: Structure class}, signatures {name: (restype, [argtypes])})"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus\n.*?#endif", " ", text, flags=re.S)
    consts, structs, sigs = {}, {}, {}
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)(?:\s+(\S.*?))?\s*", line)
        if m and m.group(2):
            consts[m.group(1)] = _int(m.group(2), m.group(1))
        elif not m and not re.fullmatch(r"\s*#\s*(ifndef\s+\w+|endif)\s*", line):      # a bare #define NAME: the include guard
            raise AbiError(f"preprocessor line not understood: {line.strip()!r}")
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)

    def struct(m):
        if m.group(1) != m.group(3):
            raise AbiError(f"typedef struct {m.group(1)} names {m.group(3)}")
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {
            "_fields_": _fields(m.group(2), consts, m.group(1)), "__doc__": f"include/puflow_hip.h: {m.group(1)}"})
        return " "
    text = re.sub(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
    known, seen = dict(POINTEES, **structs), {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(pf_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not m or m.group(2) in sigs:
            raise AbiError(f"declaration not understood: {' '.join(decl.split())[:120]!r}")
        name = m.group(2)
        res, stars = _type(m.group(1), known, name)
        if (res, stars) == (ctypes.c_char, 1):
            res = ctypes.c_char_p
        elif stars or res not in BY_VALUE:
            raise AbiError(f"{name}: return type {m.group(1)!r}")
        args = m.group(3).strip()
        sigs[name] = (res, [] if args == "void" else [_arg(a, known, name, seen) for a in args.split(",")])
    return consts, structs, sigs


@functools.lru_cache(maxsize=None)
def header():
    """The parse of include/puflow_hip.h, made once per process."""
    with open(HEADER) as f:
        return parse(f.read())
