"""The zonal-statistics entry points are declared in include/flairhip_zonestats.h (brought along by include/flairhip.h)
and bound by flairhip.lib.ZONESTATS_SIGNATURES.  This holds the pair to the comparison tests/test_abi_cpu.py makes for
the main header and its table -- that module's own parser and mismatch report, pointed at the other file --, checks that
the main header really includes the file, so that every definition is still compiled against its prototype, and that
the table shares no name with the six others.  No GPU."""
import os
import re

import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L

ZONESTATS_HEADER = os.path.join(ROOT, "include", "flairhip_zonestats.h")
NAMES = ["ffa_zone_stats_u8", "ffa_zone_stats_workspace_bytes"]


def zonestats_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(ZONESTATS_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def zonestats_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", zonestats_header_text)
    return abi.header_signatures()


def test_zonestats_table_equals_the_zonestats_header(monkeypatch):
    header = zonestats_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", zonestats_header_text())), "the parser missed a prototype"
    assert sorted(header) == NAMES
    assert abi.mismatches(header, L.ZONESTATS_SIGNATURES) == []


def test_zonestats_table_is_disjoint_from_the_other_tables():
    others = (L.SIGNATURES, L.EVAL_SIGNATURES, L.GATHER_SIGNATURES, L.SERIES_SIGNATURES, L.CALIB_SIGNATURES,
              L.OBJECT_SIGNATURES)
    assert len(others) == 6
    for other in others:
        assert not set(L.ZONESTATS_SIGNATURES) & set(other)


def test_a_planted_mismatch_is_reported(monkeypatch):
    header = zonestats_header_signatures(monkeypatch)
    ret, args = L.ZONESTATS_SIGNATURES["ffa_zone_stats_u8"]
    i = 6  # long long n_vertices
    assert args[i] is abi.C.c_longlong
    narrowed = dict(L.ZONESTATS_SIGNATURES, ffa_zone_stats_u8=(ret, args[:i] + [abi.C.c_int] + args[i + 1:]))
    assert abi.mismatches(header, narrowed) == ["ffa_zone_stats_u8: argument 6 is c_longlong, table says c_int"]
    dropped = {k: v for k, v in L.ZONESTATS_SIGNATURES.items() if k != "ffa_zone_stats_workspace_bytes"}
    assert abi.mismatches(header, dropped) == [
        "ffa_zone_stats_workspace_bytes: declared in include/flairhip.h, no ctypes signature"]


def test_the_main_header_includes_the_zonestats_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_zonestats\.h"$', main, flags=re.M)
    # inside the extern "C" block and after the types the prototypes use
    at = main.index('#include "flairhip_zonestats.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index("typedef struct ihipStream_t* ffa_stream_t;") < at


def test_the_python_constants_equal_the_header():
    from flairhip import ops
    text = open(ZONESTATS_HEADER).read()
    assert int(re.search(r"#define FFA_ZONE_STATS_CHUNK_WORDS (\d+)", text).group(1)) == ops.ZONE_STATS_CHUNK_WORDS
    assert int(re.search(r"#define FFA_ZONE_STATS_NARROW_WORDS (\d+)", text).group(1)) == ops.ZONE_STATS_NARROW_WORDS
    assert 255 * 32 * ops.ZONE_STATS_CHUNK_WORDS < 2 ** 32
