"""The C ABI has two hand-written copies: the prototypes of include/flairhip.h (the compiler holds every definition
to them: csrc/ffa_common.h includes the header) and the ctypes table flairhip.lib.SIGNATURES.  This compares the two,
type by type -- and, for the convolution call descriptor and its route, the structs field by field: a descriptor laid
out differently on the two sides hands kernels wrong pointers.  No GPU, and the library is not loaded."""
import copy
import ctypes as C
import os
import re

from helpers import ROOT
from flairhip import lib as L

STRUCTS = {"ffa_tile_t": L.Tile, "ffa_window_t": L.Window, "FfaCrs": L.Crs, "ffa_conv_call_t": L.ConvCall,
           "ffa_conv_route_t": L.ConvRoute}
FIELD_CHECKED = ("ffa_conv_call_t", "ffa_conv_route_t")
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


def header_text():
    text = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)          # comments
    return re.sub(r"//[^\n]*", " ", text)


def header_fields(struct):
    """[(name, ctypes type)] of a typedef'd struct of the header, in declaration order"""
    (body,) = re.findall(r"typedef\s+struct[^{;]*\{([^}]*)\}\s*%s\s*;" % struct, header_text())
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            kind = re.sub(r"\w+\s*$", "", first.strip())  # drop the first declarator's name
            fields += [(n.strip().split()[-1].lstrip("*"), ctype_of(kind, False)) for n in [first] + more]
    return fields


def field_mismatches(struct, fields):
    """every difference between a struct of the header and a ctypes _fields_ list, as text"""
    header = header_fields(struct)
    out = []
    for i in range(max(len(header), len(fields))):
        h = header[i] if i < len(header) else None
        t = tuple(fields[i]) if i < len(fields) else None
        if h != t:
            show = [f"{nm(x[1])} {x[0]}" if x else "absent" for x in (h, t)]
            out.append(f"{struct}: field {i} is {show[0]}, ctypes says {show[1]}")
    return out


def header_signatures():
    text = header_text()
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
    # 149 before the twelve per-layout packing entries left the ABI; 137 before the seventeen entries that ran or
    # described a convolution in one particular form left it for ffa_conv_route / ffa_conv_run and two small queries
    assert len(header) == 124
    assert mismatches(header, L.SIGNATURES) == []


def test_ctypes_structs_equal_the_header_field_by_field():
    for struct in FIELD_CHECKED:
        assert field_mismatches(struct, STRUCTS[struct]._fields_) == []
    assert len(L.ConvCall._fields_) == 31 and len(L.ConvRoute._fields_) == 9


def test_a_planted_field_mismatch_is_reported():
    fields = list(L.ConvCall._fields_)
    i = [n for n, _ in fields].index("out")
    assert [n for n, _ in fields[i:i + 2]] == ["out", "out2"]  # both void*: swapping them keeps every offset
    swapped = fields[:i] + [fields[i + 1], fields[i]] + fields[i + 2:]
    assert field_mismatches("ffa_conv_call_t", swapped) == [
        "ffa_conv_call_t: field %d is c_void_p out, ctypes says c_void_p out2" % i,
        "ffa_conv_call_t: field %d is c_void_p out2, ctypes says c_void_p out" % (i + 1)]
    j = [n for n, _ in fields].index("bn_shift")
    assert fields[j + 1][0] == "co_rows"  # a pointer and an int swapped: names and types both differ
    swapped = fields[:j] + [fields[j + 1], fields[j]] + fields[j + 2:]
    assert field_mismatches("ffa_conv_call_t", swapped) == [
        "ffa_conv_call_t: field %d is c_void_p bn_shift, ctypes says c_int co_rows" % j,
        "ffa_conv_call_t: field %d is c_int co_rows, ctypes says c_void_p bn_shift" % (j + 1)]
    assert field_mismatches("ffa_conv_route_t", L.ConvRoute._fields_[:-1]) == [
        "ffa_conv_route_t: field 8 is c_int grid, ctypes says absent"]


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
