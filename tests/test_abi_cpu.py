"""The C ABI has two hand-written copies: the prototypes of include/flairhip.h (the compiler holds every definition
to them: csrc/ffa_common.h includes the header) and the ctypes table flairhip.lib.SIGNATURES.  This compares the two,
type by type.  No GPU, and the library is not loaded."""
import copy
import ctypes as C
import os
import re

from helpers import ROOT
from flairhip import lib as L

STRUCTS = {"ffa_tile_t": L.Tile, "ffa_window_t": L.Window, "FfaCrs": L.Crs}
SCALARS = {"int": C.c_int, "long long": C.c_longlong, "int64_t": C.c_longlong, "float": C.c_float, "double": C.c_double,
           "ffa_stream_t": C.c_void_p}
# c_longlong.__name__ is "c_long" where the two are one class: print the names the table is written in
NAMES = {C.c_int: "c_int", C.c_longlong: "c_longlong", C.c_float: "c_float", C.c_double: "c_double",
         C.c_void_p: "c_void_p", C.c_char_p: "c_char_p"}


def nm(t):
    return NAMES.get(t, t.__name__)


def ctype_of(decl, is_return):
    """ctypes type of one C declarator with its parameter name already removed, e.g. 'const float*'"""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if words[-1] != "*":
        return SCALARS[" ".join(words)]
    base = " ".join(words[:-1])
    if base == "char" and is_return:
        return C.c_char_p
    return C.POINTER(STRUCTS[base]) if base in STRUCTS else C.c_void_p


def header_signatures():
    text = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)     # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    text = re.sub(r"typedef\s+struct[^{;]*\{[^}]*\}[^;]*;", " ", text)  # struct bodies
    text = re.sub(r"typedef[^;{]*;", " ", text)
    sigs = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\n\*]*?)\b(ffa_\w+)\s*\(([^()]*)\)\s*;", text):
        params = " ".join(params.split())
        args = []
        if params != "void":
            for p in params.split(","):
                decl = re.sub(r"\w+\s*$", "", p.strip())  # drop the parameter's name
                assert decl.strip(), f"{name}: unnamed parameter '{p.strip()}'"
                args.append(ctype_of(decl, False))
        assert name not in sigs, f"{name} is declared twice"
        sigs[name] = (ctype_of(ret, True), args)
    return sigs


def mismatches(header, table):
    """every difference between the header's prototypes and a ctypes table, as text"""
    out = [f"{n}: declared in include/flairhip.h, no ctypes signature" for n in sorted(set(header) - set(table))]
    out += [f"{n}: ctypes signature without a declaration" for n in sorted(set(table) - set(header))]
    for n in sorted(set(header) & set(table)):
        (hret, hargs), (tret, targs) = header[n], table[n]
        if hret is not tret:
            out.append(f"{n}: returns {nm(hret)}, table says {nm(tret)}")
        for i in range(max(len(hargs), len(targs))):
            h = hargs[i] if i < len(hargs) else None
            t = targs[i] if i < len(targs) else None
            if h is not t:
                out.append(f"{n}: argument {i} is {nm(h) if h else 'absent'}, table says {nm(t) if t else 'absent'}")
    return out


def test_ctypes_table_equals_the_header():
    header = header_signatures()
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", re.sub(r"/\*.*?\*/", "", open(
        os.path.join(ROOT, "include", "flairhip.h")).read(), flags=re.S))), "the parser missed a prototype"
    assert len(header) >= 137  # 149 before the twelve per-layout packing entries left the ABI
    assert mismatches(header, L.SIGNATURES) == []


def test_a_planted_mismatch_is_reported():
    header = header_signatures()
    name = "ffa_slice_grid"  # (..., ffa_tile_t* out, long long capacity): the last argument is the table's _ll
    ret, args = L.SIGNATURES[name]
    assert args[-1] is C.c_longlong
    narrowed = copy.copy(L.SIGNATURES)
    narrowed[name] = (ret, args[:-1] + [C.c_int])
    assert mismatches(header, narrowed) == [f"{name}: argument {len(args) - 1} is c_longlong, table says c_int"]
    dropped = copy.copy(L.SIGNATURES)
    dropped[name] = (ret, args[:-1])
    assert mismatches(header, dropped) == [f"{name}: argument {len(args) - 1} is c_longlong, table says absent"]
    wrong_ret = copy.copy(L.SIGNATURES)
    wrong_ret[name] = (C.c_int, args)
    assert mismatches(header, wrong_ret) == [f"{name}: returns c_longlong, table says c_int"]
