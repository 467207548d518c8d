"""Reader of include/gcslam.h: the binding's prototypes, structs and constants come from the header.

It accepts exactly the subset of C the header uses and raises RuntimeError, naming the line, on anything
else; nothing is skipped silently except function-like macros, which are skipped by rule.

  prototypes  ``int32_t|const char* gc_NAME(args);`` -> name: (argtypes, restype). Scalars map by name;
              a pointer of any depth and pointee is c_void_p, which takes the raw addresses, byref()
              results and POINTER instances the call sites pass.
  structs     ``typedef struct [tag] { ... } name;`` -> name: a ctypes.Structure with the header's fields.
  constants   object-like ``#define GC_NAME expr`` -> name: value; expr is numeric literals, earlier
              GC_* names, + - * << and parentheses.
"""

from __future__ import annotations

import ast
import ctypes as C
import operator
import os
import re

HEADER_PATH = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "include",
                                            "gcslam.h"))

_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "double": C.c_double,
            "float": C.c_float}
_POINTEES = {"void", "char", "uint8_t", "uint32_t"}  # met behind a * only
_OPS = {ast.Add: operator.add, ast.Sub: operator.sub, ast.Mult: operator.mul, ast.LShift: operator.lshift}


def _evaluate(expr: str, names: dict):
    def ev(n):
        if isinstance(n, ast.Constant) and type(n.value) in (int, float):
            return n.value
        if isinstance(n, ast.Name) and n.id in names:
            return names[n.id]
        if isinstance(n, ast.BinOp) and type(n.op) in _OPS:
            return _OPS[type(n.op)](ev(n.left), ev(n.right))
        if isinstance(n, ast.UnaryOp) and isinstance(n.op, ast.USub):
            return -ev(n.operand)
        raise ValueError(expr)
    return ev(ast.parse(expr.strip(), mode="eval").body)


def parse(text: str, path: str = "<header>"):
    """(prototypes, structs, constants) of a header's text."""
    # comments become blanks of the same shape, so offsets and line numbers stay the header's
    text = re.sub(r"/\*.*?\*/|//[^\n]*", lambda m: re.sub(r"[^\n]", " ", m.group()), text, flags=re.S)
    lines = text.split("\n")

    def fail(pos: int, why: str):
        n = text.count("\n", 0, pos)
        raise RuntimeError(f"{path}:{n + 1}: {why}: {lines[n].strip()}")

    consts = {}
    for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(GC_\w+)(\(?)(.*)$", text, re.M):
        if m.group(2):  # a function-like macro
            continue
        try:
            consts[m.group(1)] = _evaluate(m.group(3), consts)
        except (SyntaxError, ValueError, TypeError):
            fail(m.start(), f"cannot evaluate #define {m.group(1)}")

    struct_re = re.compile(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
    known = set(re.findall(r"\bstruct\s+(\w+)", text)) | {m.group(2) for m in struct_re.finditer(text)} | \
        set(re.findall(r"\btypedef\s+struct\s+\w+\s+(\w+)\s*;", text))

    def ctype(decl: str, pos: int, n_words):
        """The ctypes type of one `type [name]` declaration (a struct member or an argument)."""
        if "[" in decl:
            fail(pos, "array member or argument")
        words = [w for w in re.findall(r"\w+", decl) if w not in ("const", "struct")]
        base = words[0] if len(words) in n_words else None
        if "*" in decl and (base in _SCALARS or base in _POINTEES or base in known):
            return C.c_void_p
        if "*" not in decl and base in _SCALARS:
            return _SCALARS[base]
        fail(pos, "struct by value" if "*" not in decl and base in known else "unknown type token")

    structs = {}
    for m in struct_re.finditer(text):
        fields = []
        for f in re.finditer(r"\s*([^;\s][^;]*);", m.group(1)):
            fields.append((re.findall(r"\w+", f.group(1))[-1], ctype(f.group(1), m.start(1) + f.start(1), (2,))))
        structs[m.group(2)] = type(m.group(2), (C.Structure,), {"_fields_": fields})

    protos = {}
    for m in re.finditer(r"\b(int32_t|const\s+char\s*\*)\s*(gc_\w+)\s*\(([^()]*)\)\s*;", text):
        args, pos = m.group(3), m.start(3)
        argtypes = []
        for a in ([] if args.strip() in ("", "void") else args.split(",")):
            argtypes.append(ctype(a, pos + len(a) - len(a.lstrip()), (1, 2)))
            pos += len(a) + 1
        protos[m.group(2)] = (argtypes, C.c_int32 if m.group(1) == "int32_t" else C.c_char_p)
    for m in re.finditer(r"\b(gc_\w+)\s*\(", text):
        if m.group(1) not in protos:
            fail(m.start(), f"{m.group(1)} is not a prototype this reader binds")
    return protos, structs, consts


def load(path: str = HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"gcslam.h not found at {path}: the binding is derived from the header")
    with open(path) as f:
        return parse(f.read(), path)
