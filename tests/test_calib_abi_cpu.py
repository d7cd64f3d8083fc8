"""The calibration entry points are declared in include/flairhip_calib.h (brought along by include/flairhip.h) and bound
by flairhip.lib.CALIB_SIGNATURES.  This holds the pair to the comparison tests/test_abi_cpu.py makes for the main header
and its table -- that module's own parser and mismatch report, pointed at the other file --, checks that the main header
really includes the file, so that every definition is still compiled against its prototype, and that the table shares
no name with the four others.  No GPU."""
import os
import re

import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L

CALIB_HEADER = os.path.join(ROOT, "include", "flairhip_calib.h")
NAMES = ["ffa_calib_hist", "ffa_predict_thresholded_u8", "ffa_tta_predict_thresholded_u8"]


def calib_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(CALIB_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def calib_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", calib_header_text)
    return abi.header_signatures()


def test_calib_table_equals_the_calib_header(monkeypatch):
    header = calib_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", calib_header_text())), "the parser missed a prototype"
    assert sorted(header) == NAMES
    assert abi.mismatches(header, L.CALIB_SIGNATURES) == []


def test_calib_table_is_disjoint_from_the_other_tables():
    for other in (L.SIGNATURES, L.EVAL_SIGNATURES, L.GATHER_SIGNATURES, L.SERIES_SIGNATURES):
        assert not set(L.CALIB_SIGNATURES) & set(other)


def test_a_planted_mismatch_is_reported(monkeypatch):
    header = calib_header_signatures(monkeypatch)
    ret, args = L.CALIB_SIGNATURES["ffa_calib_hist"]
    i = 3  # long long npix
    assert args[i] is abi.C.c_longlong
    narrowed = dict(L.CALIB_SIGNATURES, ffa_calib_hist=(ret, args[:i] + [abi.C.c_int] + args[i + 1:]))
    assert abi.mismatches(header, narrowed) == ["ffa_calib_hist: argument 3 is c_longlong, table says c_int"]
    dropped = {k: v for k, v in L.CALIB_SIGNATURES.items() if k != "ffa_tta_predict_thresholded_u8"}
    assert abi.mismatches(header, dropped) == [
        "ffa_tta_predict_thresholded_u8: declared in include/flairhip.h, no ctypes signature"]


def test_the_main_header_includes_the_calib_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_calib\.h"$', main, flags=re.M)
    # inside the extern "C" block and after the types the prototypes use
    at = main.index('#include "flairhip_calib.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index("typedef struct ihipStream_t* ffa_stream_t;") < at
