"""Reader of include/pvamd.h: the header is the one definition of the C ABI, and the ctypes binding (_lib.py) is read from it.

Every declaration must map by the rules below; anything else raises, naming the declaration -- none is ever skipped.
"""
import ctypes
import os
import re

# where csrc/Makefile finds it: ../../include/pvamd.h
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pvamd.h")

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "uint8_t": ctypes.c_uint8, "float": ctypes.c_float, "double": ctypes.c_double}
# The host structs, passed with ctypes.byref: (type, parameter name) -> name of the ctypes mirror in _lib.  Every other pointer
# parameter is c_void_p (_lib.call passes addresses and None; its checks read the element type from the parameter records) --
# `grids` and `joints`, device arrays of the same types, included.
HOST_STRUCTS = {("pvamd_grid_t", "grid"): "GridDesc", ("pvamd_mesh_t", "mesh"): "MeshDesc",
                ("pvamd_mesh_plan_t", "plan_out"): "MeshPlan"}

_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\(?)[ \t]*(-?(?:0|[1-9]\d*))[ \t]*(\)?)[ \t]*$", re.M)
_DECLARATION = re.compile(r"(const\s+char\s*\*|\w+)\s*\b(pvamd_\w+)\s*\((.*)\)", re.S)
_PARAMETER = re.compile(r"(const\s+)?(\w+)(\s*\*\s*|\s+)(\w+)")


def _statements(text):
    """(defines, statements) of a header given as a string: the #defines the reader keeps, and (name, return type, parameters) of
    every declaration in header order, each parameter as (name, base type, is a pointer, is const).  Raises on anything that is not
    `type pvamd_name(parameters);` with parameters `[const] type[*] name`."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {name: int(value) for name, left, value, right in _DEFINE.findall(text) if bool(left) == bool(right)}
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", "", text, flags=re.M)  # preprocessor lines, continuations included
    body = re.sub(r"\btypedef\s+struct\s+\w*\s*\{[^{}]*\}\s*\w+\s*;", "", text)
    body = re.sub(r'\bextern\s+"C"\s*\{(.*)\}', r"\1", body, flags=re.S)
    statements, names = [], set()
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        m = _DECLARATION.fullmatch(statement)
        if m is None:
            raise ValueError(f"pvamd.h: not a declaration this reader knows: {' '.join(statement.split())!r}")
        ret, name, params = m.groups()
        if name in names:
            raise ValueError(f"pvamd.h: {name} is declared twice")
        if "(" in params:
            raise ValueError(f"pvamd.h: {name}: function-pointer parameters are not supported")
        records = []
        for param in ([] if params.strip() == "void" else params.split(",")):
            p = _PARAMETER.fullmatch(param.strip())
            if p is None:
                raise ValueError(f"pvamd.h: {name}: parameter {' '.join(param.split())!r} is not `[const] type[*] name`")
            const, ctype, sep, pname = p.groups()
            records.append((pname, ctype, "*" in sep, const is not None))
        names.add(name)
        statements.append((name, ret, records))
    missed = set(re.findall(r"\b(pvamd_\w+)\s*\(", text)) - names
    if missed:
        raise ValueError(f"pvamd.h: {sorted(missed)} look like entry points but were not read as declarations")
    return defines, statements


def parse(text, mirrors):
    """(declarations, defines) of a header given as a string.  declarations: name -> (restype, argtypes), in header order;
    defines: name -> value of every object-like #define whose body is one decimal integer, bare or in parentheses.
    mirrors: name -> ctypes.Structure for the names HOST_STRUCTS maps to."""
    defines, statements = _statements(text)
    declarations = {}
    for name, ret, records in statements:
        restype = ctypes.c_char_p if ret.endswith("*") else SCALARS.get(ret)
        if restype is None:
            raise ValueError(f"pvamd.h: {name}: unknown return type {ret!r}")
        argtypes = []
        for pname, ctype, pointer, _ in records:
            if pointer:
                mirror = HOST_STRUCTS.get((ctype, pname))
                argtypes.append(ctypes.POINTER(mirrors[mirror]) if mirror else ctypes.c_void_p)
            elif ctype in SCALARS:
                argtypes.append(SCALARS[ctype])
            else:
                raise ValueError(f"pvamd.h: {name}: unknown type {ctype!r} of parameter {pname!r}")
        declarations[name] = (restype, argtypes)
    return declarations, defines


def parameters(text):
    """What argtypes no longer tells of the same declarations: name -> [(parameter name, base type, is a pointer, is const)], in
    header order."""
    return {name: records for name, _, records in _statements(text)[1]}


def read(mirrors):
    """parse() of the header file."""
    with open(HEADER_PATH) as f:
        return parse(f.read(), mirrors)


def read_parameters():
    """parameters() of the header file."""
    with open(HEADER_PATH) as f:
        return parameters(f.read())
