"""The evaluation entry points are declared in include/flairhip_eval.h (brought along by include/flairhip.h) and bound
by flairhip.lib.EVAL_SIGNATURES.  This holds the pair to the comparison tests/test_abi_cpu.py makes for the main header
and its table -- that module's own parser and mismatch report, pointed at the other file -- and checks that the main
header really includes the file, so that every definition is still compiled against its prototype.  No GPU."""
import os
import re

import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L

EVAL_HEADER = os.path.join(ROOT, "include", "flairhip_eval.h")


def eval_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(EVAL_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def eval_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", eval_header_text)
    return abi.header_signatures()


def test_eval_table_equals_the_eval_header(monkeypatch):
    header = eval_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", eval_header_text())), "the parser missed a prototype"
    assert sorted(header) == ["ffa_eval_stats", "ffa_eval_stats_workspace_bytes"]
    assert abi.mismatches(header, L.EVAL_SIGNATURES) == []
    assert not set(L.EVAL_SIGNATURES) & set(L.SIGNATURES)


def test_a_planted_mismatch_is_reported(monkeypatch):
    header = eval_header_signatures(monkeypatch)
    ret, args = L.EVAL_SIGNATURES["ffa_eval_stats"]
    i = 3  # long long npix
    assert args[i] is abi.C.c_longlong
    narrowed = dict(L.EVAL_SIGNATURES, ffa_eval_stats=(ret, args[:i] + [abi.C.c_int] + args[i + 1:]))
    assert abi.mismatches(header, narrowed) == ["ffa_eval_stats: argument 3 is c_longlong, table says c_int"]
    dropped = {k: v for k, v in L.EVAL_SIGNATURES.items() if k != "ffa_eval_stats_workspace_bytes"}
    assert abi.mismatches(header, dropped) == [
        "ffa_eval_stats_workspace_bytes: declared in include/flairhip.h, no ctypes signature"]


def test_the_main_header_includes_the_eval_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_eval\.h"$', main, flags=re.M)
    # inside the extern "C" block and after the types the prototypes use
    at = main.index('#include "flairhip_eval.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index("typedef struct ihipStream_t* ffa_stream_t;") < at
