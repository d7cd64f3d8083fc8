"""The sample-store entry points are declared in include/flairhip_gather.h (brought along by include/flairhip.h) and
bound by flairhip.lib.GATHER_SIGNATURES.  This holds the pair to the comparison tests/test_abi_cpu.py makes for the main
header and its table -- that module's own parser and mismatch report, pointed at the other file -- and checks that the
main header really includes the file, so that every definition is still compiled against its prototype.  No GPU."""
import os
import re

import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L

GATHER_HEADER = os.path.join(ROOT, "include", "flairhip_gather.h")


def gather_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(GATHER_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def gather_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", gather_header_text)
    return abi.header_signatures()


def test_gather_table_equals_the_gather_header(monkeypatch):
    header = gather_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", gather_header_text())), "the parser missed a prototype"
    assert sorted(header) == ["ffa_gather_labels_u8", "ffa_gather_layout"]
    assert abi.mismatches(header, L.GATHER_SIGNATURES) == []
    assert not set(L.GATHER_SIGNATURES) & (set(L.SIGNATURES) | set(L.EVAL_SIGNATURES))


def test_a_planted_mismatch_is_reported(monkeypatch):
    header = gather_header_signatures(monkeypatch)
    ret, args = L.GATHER_SIGNATURES["ffa_gather_layout"]
    i = 5  # int N
    assert args[i] is abi.C.c_int
    widened = dict(L.GATHER_SIGNATURES, ffa_gather_layout=(ret, args[:i] + [abi.C.c_longlong] + args[i + 1:]))
    assert abi.mismatches(header, widened) == ["ffa_gather_layout: argument 5 is c_int, table says c_longlong"]
    dropped = {k: v for k, v in L.GATHER_SIGNATURES.items() if k != "ffa_gather_labels_u8"}
    assert abi.mismatches(header, dropped) == [
        "ffa_gather_labels_u8: declared in include/flairhip.h, no ctypes signature"]


def test_the_main_header_includes_the_gather_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_gather\.h"$', main, flags=re.M)
    at = main.index('#include "flairhip_gather.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index("typedef struct ihipStream_t* ffa_stream_t;") < at
    assert main.index("#define FFA_SRC_F32 3") < at  # the sample kinds the prototypes speak of


def test_the_elevation_modes_agree_between_header_and_python():
    from flairhip import ops
    text = open(GATHER_HEADER).read()
    for name, value in (("NONE", ops.ELEV_NONE), ("DIFF", ops.ELEV_DIFF), ("STACK", ops.ELEV_STACK)):
        assert re.search(r"^#define FFA_ELEV_%s %d\b" % (name, value), text, flags=re.M)
