"""Reader of include/factorizer_hip.h, the one statement of the native library's C ABI.

`read()` returns the header's integer constants, descriptor structs and entry points as plain data; _native.py turns them into
the ctypes binding.  The reader is strict: a declaration it has no rule for raises NativeError and names the declaration — a
declaration skipped in silence would reach a kernel as a shifted argument.  The forms it takes are listed at the top of the
header.  No torch import: tests and tools read the header without loading the package's device code.
"""
from __future__ import annotations

import collections
import functools
import os
import re

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = os.path.join(INCLUDE_DIR, "factorizer_hip.h")


class NativeError(RuntimeError):
    pass


CType = collections.namedtuple("CType", "base ptr")            # `const float* const*` is CType("float", 2): const is dropped
Header = collections.namedtuple("Header", "defines structs functions")
# defines {name: int}; structs {name: [(CType, field, array length or 0)]}; functions {name: (CType, [(CType, argument)])}

_RETURNS = (CType("int", 0), CType("int64_t", 0), CType("char", 1))
_SCALARS = {"int", "int64_t", "float", "double"}
_POINTEES = {"void", "char", "int", "float", "double", "int64_t", "uint8_t", "int32_t", "uint32_t"}
_TYPE = r"(?:const\s+)?(?:struct\s+)?(\w+)((?:\s*\*(?:\s*const\b)?)*)"
_NAME = r"(\w+)(?:\s*\[\s*(\d+)\s*\])?"
_DEFINE = re.compile(r"#\s*define\s+(FZ_\w+)\b(.*)")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_HANDLE = re.compile(r"typedef\s+void\s*\*\s*(\w+)")
_FORWARD = re.compile(r"struct\s+(\w+)")
_FIELD = re.compile(rf"{_TYPE}\s*({_NAME}(?:\s*,\s*{_NAME})*)")
_PROTO = re.compile(rf"{_TYPE}\s*\b(fz_\w+)\s*\((.*)\)", re.S)
_PARAM = re.compile(rf"{_TYPE}\s*(\w+)")


def parse(text: str) -> Header:
    """the constants, structs and entry points that the text of a header declares; NativeError for anything else in it"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    defines, code = {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            code.append(line)
        elif m := _DEFINE.match(line.strip()):
            value = re.fullmatch(r"\s*(?:(-?\d+)|\(\s*(-?\d+)\s*\))\s*", m[2])
            if not value:
                raise NativeError(f"#define {m[1]}: `{m[2].strip()}` is not an integer or a parenthesised integer")
            defines[m[1]] = int(value[1] or value[2])
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', " ", "\n".join(code))
    if wrapped and text.rstrip().endswith("}"):
        text = text.rstrip()[:-1]

    bodies = {}
    for m in _STRUCT.finditer(text):
        if m[1] != m[3]:
            raise NativeError(f"typedef struct {m[1]} {{ ... }} {m[3]}: tag and typedef name differ")
        bodies[m[1]] = m[2]
    statements = [s.strip() for s in _STRUCT.sub(" ", text).split(";") if s.strip()]
    handles = {m[1] for s in statements if (m := _HANDLE.fullmatch(s))}

    def ctype(base, stars, where):
        t = CType(base, stars.count("*"))
        known = {0: base in _SCALARS or base in handles, 1: base in _POINTEES or base in bodies,
                 2: base == "void" or base in bodies}
        if not known.get(t.ptr):
            raise NativeError(f"{where}: no rule for the type `{base}{'*' * t.ptr}`")
        return t

    structs = {}
    for name, body in bodies.items():
        structs[name] = fields = []
        for decl in (d.strip() for d in body.split(";") if d.strip()):
            m = _FIELD.fullmatch(decl)
            if not m:
                raise NativeError(f"struct {name}: cannot read the field `{decl}`")
            t = ctype(m[1], m[2], f"struct {name}, field `{decl}`")
            fields += [(t, n, int(k or 0)) for n, k in re.findall(_NAME, m[3])]

    functions = {}
    for s in statements:
        if _HANDLE.fullmatch(s) or ((m := _FORWARD.fullmatch(s)) and m[1] in bodies):
            continue
        m = _PROTO.fullmatch(s)
        if not m or m[3] in functions:
            raise NativeError(f"cannot read the declaration `{' '.join(s.split())}`")
        args = []
        for p in ([] if m[4].strip() == "void" else m[4].split(",")):
            a = _PARAM.fullmatch(p.strip())
            if not a:
                raise NativeError(f"{m[3]}: cannot read the argument `{' '.join(p.split())}`")
            args.append((ctype(a[1], a[2], f"{m[3]}, argument `{a[3]}`"), a[3]))
        ret = ctype(m[1], m[2], f"{m[3]}, return type")
        if ret not in _RETURNS:
            raise NativeError(f"{m[3]}: returns `{m[1]}{'*' * ret.ptr}`, not int, int64_t or const char*")
        functions[m[3]] = (ret, args)
    left = sorted(set(re.findall(r"\b(fz_\w+)\s*\(", text)) - set(functions))
    if left:
        raise NativeError(f"{', '.join(left)}: followed by `(` in the header but not read as an entry point")
    return Header(defines, structs, functions)


@functools.lru_cache(maxsize=None)
def read() -> Header:
    """the parsed include/factorizer_hip.h (read once per process)"""
    with open(HEADER) as f:
        return parse(f.read())
