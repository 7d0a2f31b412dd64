"""A strict reader of include/egc_hip.h: the header's constants, structs and prototypes as ctypes objects.

``read_header(text)`` is a function of the header's TEXT.  It recognises exactly the constructs the header uses --
``#define EGC_X <integer expression>``, ``typedef enum``, ``typedef struct``, ``typedef void* handle;`` and prototypes --
and raises ``AbiError`` naming the offending text on anything else: a reader that skipped what it does not understand
would hide exactly the mismatch it exists to prevent.  The type rule is DESIGN.md's section on the binding's one owner.
"""
from __future__ import annotations

import ast
import ctypes as C
import keyword
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32,
           "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
POINTEE_ONLY = ("void", "char")


class AbiError(ValueError):
    pass


class Abi:
    """constants: EGC_X -> int (enum members included); enums: type -> {member: int}; structs: C name -> ctypes class;
    prototypes: name -> (restype, argtypes)."""

    def __init__(self):
        self.constants, self.enums, self.structs, self.handles, self.prototypes = {}, {}, {}, set(), {}


_INT_OPS = (ast.Add, ast.Sub, ast.Mult, ast.LShift, ast.RShift, ast.BitOr, ast.BitAnd)


def _int_expr(expr: str, constants: dict, where: str) -> int:
    def ev(node):
        if isinstance(node, ast.Constant) and type(node.value) is int:
            return node.value
        if isinstance(node, ast.Name) and node.id in constants:
            return constants[node.id]
        if isinstance(node, ast.BinOp) and isinstance(node.op, _INT_OPS):
            a, b = ev(node.left), ev(node.right)
            return {ast.Add: a + b, ast.Sub: a - b, ast.Mult: a * b, ast.LShift: a << b, ast.RShift: a >> b,
                    ast.BitOr: a | b, ast.BitAnd: a & b}[type(node.op)]
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            return -ev(node.operand)
        raise AbiError(f"not an integer expression: '{expr.strip()}' in '{where.strip()}'")
    try:
        return ev(ast.parse(expr.strip(), mode="eval").body)
    except SyntaxError:
        raise AbiError(f"not an integer expression: '{expr.strip()}' in '{where.strip()}'") from None


_DECLARATOR = re.compile(r"((?:\*\s*)*)(\w+)?\s*(?:\[([^\]]*)\])?\s*$")


def _declarations(text: str, abi: Abi, parameter: bool):
    """(name, ctype) of every declarator of ``type a, *b[N]``; ``const`` carries no ABI meaning and is dropped."""
    decl = re.sub(r"\bconst\b", " ", text).strip()
    m = re.match(r"(\w+)\s*(.*)$", decl, re.S)
    if not m:
        raise AbiError(f"not a declaration: '{text.strip()}'")
    base, out = m.group(1), []
    if base not in SCALARS and base not in POINTEE_ONLY and base not in abi.structs and base not in abi.handles:
        raise AbiError(f"unknown type '{base}' in '{text.strip()}'")
    for part in m.group(2).split(","):
        d = _DECLARATOR.match(part.strip())
        if not d:
            raise AbiError(f"not a declarator: '{part.strip()}' in '{text.strip()}'")
        depth, name, dim = d.group(1).count("*"), d.group(2), d.group(3)
        if dim is not None and parameter:                       # name[] / name[N] as a parameter is a pointer
            depth, dim = depth + 1, None
        if depth == 0:
            if base in POINTEE_ONLY:
                raise AbiError(f"'{base}' by value in '{text.strip()}'")
            ctype = C.c_void_p if base in abi.handles else SCALARS.get(base) or abi.structs[base]
        elif depth == 1 and base == "char":
            ctype = C.c_char_p
        elif depth == 1 and parameter and base in abi.structs:
            ctype = C.POINTER(abi.structs[base])
        else:
            ctype = C.c_void_p
        if dim is not None:
            ctype = ctype * _int_expr(dim, abi.constants, text)
        out.append((name, ctype))
    return out


def _struct(c_name: str, body: str, abi: Abi):
    fields = []
    for member in body.split(";")[:-1]:
        for name, ctype in _declarations(member, abi, parameter=False):
            if name is None:
                raise AbiError(f"member without a name: '{member.strip()}' in struct {c_name}")
            fields.append((name + "_" if keyword.iskeyword(name) else name, ctype))
    if body.split(";")[-1].strip():
        raise AbiError(f"unterminated member '{body.split(';')[-1].strip()}' in struct {c_name}")
    py_name = "".join(w.capitalize() for w in c_name.split("_"))
    return type(py_name, (C.Structure,), {"_fields_": fields})


def _enum(body: str, abi: Abi, where: str):
    members, nxt = {}, 0
    for item in body.split(","):
        if not item.strip():
            continue
        name, _, value = (s.strip() for s in item.partition("="))
        if not re.fullmatch(r"EGC_\w+", name):
            raise AbiError(f"not an enumerator: '{item.strip()}' in '{where.strip()}'")
        members[name] = abi.constants[name] = _int_expr(value, abi.constants, item) if value else nxt
        nxt = members[name] + 1
    return members


_CONSTRUCTS = [(kind, re.compile(pat, re.S)) for kind, pat in (
    ("define", r"#define[ \t]+(EGC_\w+)([^\n]*)"),
    ("enum", r"typedef\s+enum\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("struct", r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("handle", r"typedef\s+void\s*\*\s*(\w+)\s*;"),
    ("prototype", r"([\w\s\*]+?[\s\*])(egc_\w+)\s*\(([^(){};]*)\)\s*;"),
)]
_SPACE = re.compile(r"\s*")


def read_header(text: str) -> Abi:
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"\A\s*#ifndef[ \t]+(\w+)\s*\n\s*#define[ \t]+\1[ \t]*\n(.*)#endif\s*\Z", r"\2", text, flags=re.S)
    text = re.sub(r'#ifdef[ \t]+__cplusplus\s*(extern\s+"C"\s*\{|\})\s*#endif', " ", text)
    text = re.sub(r"^[ \t]*#include[ \t]*<[\w./]+>[ \t]*$", " ", text, flags=re.M)
    abi, pos = Abi(), 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            return abi
        for kind, pattern in _CONSTRUCTS:
            m = pattern.match(text, pos)
            if m:
                break
        else:
            raise AbiError(f"cannot read the header at '{text[pos:].splitlines()[0][:80]}'")
        if kind == "define":
            abi.constants[m.group(1)] = _int_expr(m.group(2), abi.constants, m.group(0))
        elif kind == "enum":
            abi.enums[m.group(2)] = _enum(m.group(1), abi, m.group(0))
        elif kind == "struct":
            abi.structs[m.group(2)] = _struct(m.group(2), m.group(1), abi)
        elif kind == "handle":
            abi.handles.add(m.group(1))
        else:
            (_, restype), = _declarations(m.group(1) + " ret", abi, parameter=True)
            params = m.group(3).strip()
            args = [] if params in ("", "void") else [t for p in params.split(",") for _, t in _declarations(p, abi, True)]
            abi.prototypes[m.group(2)] = (restype, args)
        pos = m.end()
