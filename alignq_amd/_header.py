"""Reader of include/alignq.h for the ctypes binding (_lib.py).  The header is plain C by design - prototypes over pointers and
scalars, two POD argument records, integer #defines - and that is all this reads.  Anything else raises AlignQLibraryError with
the declaration in the message: a header extended beyond that must fail at import, not bind wrongly."""
from __future__ import annotations

import ctypes
import re


class AlignQLibraryError(RuntimeError):
    pass


# the whole scalar vocabulary of the header; anything with a '*' is a c_void_p (a `char*` RETURN: c_char_p)
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "unsigned": ctypes.c_uint32, "uint32_t": ctypes.c_uint32,
           "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
           "double": ctypes.c_double}

_DEFINE = re.compile(r"#\s*define\s+(ALIGNQ_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$")
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_PROTO = re.compile(r"(.+?)\b(\w+)\s*\(([^()]*)\)", re.S)
_DECL = re.compile(r"(.*?)\b(\w+(?:\s*,\s*\w+)*)", re.S)          # type, then one or several plain declarators


def _ctype(text, decl, ret=False):
    words = [w for w in text.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return ctypes.c_char_p if ret and words == ["char", "*"] else ctypes.c_void_p
    if len(words) != 1 or words[0] not in SCALARS:
        raise AlignQLibraryError(f"alignq.h: type {text.strip()!r} is outside the binding's vocabulary in `{decl}`")
    return SCALARS[words[0]]


def _declarators(decl, whole):
    """`float momentum, bn_eps` -> [("momentum", c_float), ("bn_eps", c_float)]"""
    m = _DECL.fullmatch(decl)
    if not m:
        raise AlignQLibraryError(f"alignq.h: cannot read the declaration `{decl}` in `{whole}`")
    ctype = _ctype(m.group(1), decl)
    return [(name, ctype) for name in re.split(r"\s*,\s*", m.group(2))]


def parse(text):
    """(functions, structs, constants): name -> (restype, [argtypes]); typedef name -> [(field, ctype)]; ALIGNQ_X -> int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    lines = text.split("\n")
    constants = {m.group(1): int(m.group(2)) for m in map(_DEFINE.match, map(str.strip, lines)) if m}
    text = "\n".join(ln for ln in lines if not ln.lstrip().startswith("#"))
    structs = {}
    for m in _STRUCT.finditer(text):
        whole = " ".join(m.group(0).split())
        structs[m.group(2)] = [f for d in m.group(1).split(";") if d.strip() for f in _declarators(d.strip(), whole)]
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", _STRUCT.sub("", text), flags=re.S)
    functions = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if not stmt:
            continue
        m = _PROTO.fullmatch(stmt)
        if not m:
            raise AlignQLibraryError(f"alignq.h: cannot read `{stmt}` as a prototype")
        params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
        args = [_declarators(p.strip(), stmt)[0][1] for p in params]          # split at the commas: one declarator each
        functions[m.group(2)] = (_ctype(m.group(1), stmt, ret=True), args)
    return functions, structs, constants


def read(path):
    with open(path) as f:
        return parse(f.read())
