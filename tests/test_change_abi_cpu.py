"""The land-cover change entry points are declared in include/flairhip_change.h (brought along by include/flairhip.h)
and bound by flairhip.lib.CHANGE_SIGNATURES.  This holds the pair to the comparison tests/test_abi_cpu.py makes for the
main header and its table -- that module's own parser and mismatch report, pointed at the other file, as
tests/test_zonestats_abi_cpu.py does --, checks that the main header includes the file inside its extern "C" block and
that the table shares no name with the seven others.  No GPU."""
import os
import re

import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L

CHANGE_HEADER = os.path.join(ROOT, "include", "flairhip_change.h")
NAMES = ["ffa_change_code_u8", "ffa_zone_change_u8"]


def change_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(CHANGE_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def change_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", change_header_text)
    return abi.header_signatures()


def test_change_table_equals_the_change_header(monkeypatch):
    header = change_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", change_header_text())), "the parser missed a prototype"
    assert sorted(header) == NAMES
    assert abi.mismatches(header, L.CHANGE_SIGNATURES) == []


def test_the_zone_tables_of_both_entry_points_have_one_signature(monkeypatch):
    """ffa_zone_change_u8 takes ffa_zone_stats_u8's arguments with one more raster in front"""
    _, change = L.CHANGE_SIGNATURES["ffa_zone_change_u8"]
    _, stats = L.ZONESTATS_SIGNATURES["ffa_zone_stats_u8"]
    assert change[1:] == stats


def test_change_table_is_disjoint_from_the_other_tables():
    others = (L.SIGNATURES, L.EVAL_SIGNATURES, L.GATHER_SIGNATURES, L.SERIES_SIGNATURES, L.CALIB_SIGNATURES,
              L.OBJECT_SIGNATURES, L.ZONESTATS_SIGNATURES)
    assert len(others) == 7
    for other in others:
        assert not set(L.CHANGE_SIGNATURES) & set(other)


def test_a_planted_mismatch_is_reported(monkeypatch):
    header = change_header_signatures(monkeypatch)
    ret, args = L.CHANGE_SIGNATURES["ffa_change_code_u8"]
    i = 2  # long long n
    assert args[i] is abi.C.c_longlong
    narrowed = dict(L.CHANGE_SIGNATURES, ffa_change_code_u8=(ret, args[:i] + [abi.C.c_int] + args[i + 1:]))
    assert abi.mismatches(header, narrowed) == ["ffa_change_code_u8: argument 2 is c_longlong, table says c_int"]


def test_the_main_header_includes_the_change_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_change\.h"$', main, flags=re.M)
    at = main.index('#include "flairhip_change.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index('#include "flairhip_zonestats.h"') < at  # the zone tables and FFA_ZONE_STATS_* are that file's
    # the comment above the include names no entry point: the export check scans the main header with its comments
    assert not re.search(r"ffa_(zone_change|change_code)\w*\s*\(", main)


def test_the_python_constants_equal_the_header():
    from flairhip import ops
    from flair_zonal_detection import change
    text = open(CHANGE_HEADER).read()
    K = int(re.search(r"#define FFA_CHANGE_MAX_CLASSES (\d+)", text).group(1))
    assert K == ops.CHANGE_MAX_CLASSES == change.MAX_CLASSES == 32
    assert 2 * 4 * (K + 1) ** 2 * 4 == 34848 <= 64 * 1024  # two uint32 tables per wave, four waves: static LDS
