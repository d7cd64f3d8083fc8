"""What a convolution call will run, asked without a GPU.

1. The public queries of flairhip.ops -- upcat_supported, pro_supported, conv_stat_rows, conv_is_persistent -- give the
   answers recorded in tests/golden/conv_routes.json by tests/golden/gen_conv_routes.py at the last commit at which
   each of them was a separate rule (several of them written twice, in C++ and in Python); the file's "recorded" field
   names it.  This module uses only Python calls that exist unchanged there.  The file is never re-recorded for a change
   of the call path: a statistics buffer sized by one answer and written by a kernel that tiles differently is an
   out-of-bounds write.
2. ffa_conv_route refuses what the entries it replaced refused, with the same code and text of the same kind."""
import ctypes as C
import json
import os

import pytest
import torch

from flairhip import lib as L, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")
BF16, F32 = torch.bfloat16, torch.float32
SWITCHES = ("FFA_RING", "FFA_RING_GRID", "FFA_RING_CFG", "FFA_THIN", "FFA_THIN_GRID", "FFA_STEM", "FFA_STEM_GRID",
            "FFA_CONV_PERSIST", "FFA_CONV_PERSIST_MIN", "FFA_CONV_PERSIST_GRID")
SIZES = [(n, n) for n in (8, 16, 24, 32, 40, 128)] + [(24, 40)]
BATCHES = (1, 3)
PERSIST_ENVS = {"default": {}, "off": {"FFA_CONV_PERSIST": "0"}, "min": {"FFA_CONV_PERSIST_MIN": "10000"},
                "grid8": {"FFA_CONV_PERSIST_GRID": "8"}}
SPLITS = range(0, 513, 16)


def _name(dtype) -> str:
    return "bf16" if dtype == BF16 else "f32"


def unet_operands() -> dict:
    """{key: (dtype, PackedWeight without data)} for every conv operand of the U-Net (ResNet-34 encoder, 5 input
    channels, 19 classes): both dtypes, forward and transposed, each (ring, thin) request HipConv2d.packed is called
    with.  Planned as ops.pack_conv_weight plans, minus the packing launch."""
    from flairhip import nn as hnn
    from flairhip.unet import UnetResNet34
    lib = L.load()
    out = {}
    for m in UnetResNet34(5, 19).modules():
        if not isinstance(m, hnn.HipConv2d):
            continue
        for dtype in (BF16, F32):
            for transpose in (False, True):
                for request in ((True, True), (False, True), (False, False)):
                    ring, thin, stem = m.allow(*request)
                    k, o, i = m.kernel_size, m.out_channels, m.in_channels
                    rows_real, stride = (i, 1) if transpose else (o, m.stride)
                    pitch = m.out_pitch if transpose else m.in_pitch
                    plain = not (transpose and m.stride != 1)
                    bco = lib.ffa_conv_plan(ops._dtype_id(dtype), k, k, stride, rows_real, pitch,
                                            (1 if ring and plain else 0) | (2 if thin and plain else 0) |
                                            (4 if stem and not transpose and i <= 8 else 0))
                    if bco <= 0:  # (the transposed 7x7: no such operand exists)
                        continue
                    blk = bco & 0xFFF
                    pw = ops.PackedWeight(torch.empty(0, dtype=dtype), (rows_real + blk - 1) // blk * blk, rows_real,
                                          pitch, bco, k, k, stride, o if transpose else i)
                    out[f"{_name(dtype)}/k{k}s{stride}/rows{pw.rows}of{rows_real}/pitch{pitch}of{pw.ch_real}/"
                        f"bco{bco:#x}"] = (dtype, pw)
    return out


def _bits(flags) -> str:
    return "".join("1" if f else "0" for f in flags)


def answers() -> dict:
    """every recorded answer; the environment switches are cleared and set here (the library reads them per call)"""
    for name in SWITCHES:
        os.environ.pop(name, None)
    got = {"upcat_supported": {_name(d): [_bits(ops.upcat_supported(c1, c2, d) for c2 in SPLITS) for c1 in SPLITS]
                               for d in (BF16, F32)}, "operands": {}}
    cases = [(b, h, w) for b in BATCHES for h, w in SIZES]
    operands = unet_operands()
    for key, (dtype, pw) in operands.items():
        got["operands"][key] = {"pro_supported": _bits(ops.pro_supported(pw, dtype, up) for up in (False, True)),
                                "conv_stat_rows": [ops.conv_stat_rows(b, h, w, pw) for b, h, w in cases],
                                "conv_is_persistent": {}}
    got["conv_stat_rows_default"] = [ops.conv_stat_rows(b, h, w) for b, h, w in cases]
    for env, values in PERSIST_ENVS.items():
        os.environ.update(values)
        for key, (dtype, pw) in operands.items():
            got["operands"][key]["conv_is_persistent"][env] = _bits(
                ops.conv_is_persistent(dtype, b, h, w, pw) for b, h, w in cases)
        for name in values:
            del os.environ[name]
    return got


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


def test_public_queries_give_the_recorded_answers(clean_env):
    with open(GOLDEN) as f:
        golden = json.load(f)["answers"]
    got = json.loads(json.dumps(answers()))
    assert got["upcat_supported"] == golden["upcat_supported"]
    assert got["conv_stat_rows_default"] == golden["conv_stat_rows_default"]
    assert sorted(got["operands"]) == sorted(golden["operands"])
    assert len(got["operands"]) > 60
    layouts = {int(k.rsplit("bco", 1)[1], 16) & (L.BCO_RING | L.BCO_THIN | L.BCO_STEM) for k in got["operands"]}
    assert layouts == {0, L.BCO_RING, L.BCO_THIN, L.BCO_STEM}
    wrong = [(k, q) for k, a in got["operands"].items() for q in a if a[q] != golden["operands"][k][q]]
    assert not wrong, wrong


# ---- refusals -------------------------------------------------------------------------------------------------------

def _call(**kw):
    """a plain 3x3 stride-1 pad-1 bf16 call on a conv_igemm operand, 2 x 16 x 16 x 64 -> 64, with fields replaced"""
    fields = dict(dtype=L.BF16, form=L.CONV_PLAIN, co_rows=64, bco=64, B=2, Hi=16, Wi=16, Ci=64, Ho=16, Wo=16, Co=64,
                  kh=3, kw=3, stride=1, pad=1, dil=1)
    fields.update(kw)
    return L.ConvCall(**fields)


SOME = 1  # the router reads only whether an optional pointer is null
REFUSALS = ("ring operand with dil = 2", "thin operand with C2 != 0", "stem operand with a residual",
            "prologue on a conv_igemm operand", "pooled form with a bias", "thin pooled form with a bias",
            "Ci % 16 != 0", "input of 2 GiB", "f32 two-source call on a thin operand",
            "two-source call whose rows are not whole blocks", "pooled form on a ring operand")


def _refusal(case: str):
    """(fields replaced in _call(), code, text) -- what the entry that took this call before answered"""
    thin32 = dict(bco=32 | L.BCO_THIN | 0x4000, co_rows=32, Ci=32, Co=32)  # (0x4000: the operand multiplies 32-channel pixels)
    return {
        REFUSALS[0]: (dict(bco=64 | L.BCO_RING, dil=2), -1, b"ring-layout operand serves plain"),
        REFUSALS[1]: (dict(form=L.CONV_UPCAT, c1=16, **thin32), -2, b"thin-layout operand takes the skip-less form only"),
        REFUSALS[2]: (dict(bco=64 | L.BCO_STEM, kh=7, kw=7, stride=2, pad=3, Hi=32, Wi=32, Ci=16, residual=SOME), -1,
                      b"stem-layout operand serves"),
        REFUSALS[3]: (dict(pro_scale=SOME, pro_shift=SOME), -2, b"no prologue kernel"),
        REFUSALS[4]: (dict(form=L.CONV_POOLED, c1=64, bias=SOME), -1, b"pooled form has a plain epilogue"),
        REFUSALS[5]: (dict(form=L.CONV_POOLED, c1=32, bias=SOME, **thin32), -1, b"pooled form has a plain epilogue"),
        REFUSALS[6]: (dict(Ci=24), -1, b"channel pitch must be a multiple of 16"),
        REFUSALS[7]: (dict(B=64, Hi=512, Wi=512, Ho=512, Wo=512), -1, b"smaller than 2 GiB"),
        REFUSALS[8]: (dict(form=L.CONV_UPCAT, c1=32, dtype=L.F32, **thin32), -2, b"takes the skip-less form only"),
        REFUSALS[9]: (dict(form=L.CONV_UPCAT, Ci=128, c1=64, co_rows=96), -2, b"not a multiple of block"),
        REFUSALS[10]: (dict(form=L.CONV_POOLED, c1=64, bco=64 | L.BCO_RING), -2, b"serves the plain form only"),
    }[case]


@pytest.mark.parametrize("case", REFUSALS)
def test_route_refuses_what_the_entries_refused(lib, clean_env, case):
    fields, code, text = _refusal(case)
    route = L.ConvRoute()
    assert lib.ffa_conv_route(C.byref(_call()), C.byref(route)) == 0  # the call the case is derived from is fine
    assert (route.th, route.tw, route.ntiles) == (16, 16, 2)
    without = {k: v for k, v in fields.items() if k not in ("bias", "residual")}
    if without != fields:  # the same call without the offending pointer is served
        assert lib.ffa_conv_route(C.byref(_call(**without)), C.byref(route)) == 0
    assert lib.ffa_conv_route(C.byref(_call(**fields)), C.byref(route)) == code
    assert text in lib.ffa_last_error()


def test_route_and_size_of_the_largest_input_below_2_gib(lib, clean_env):
    """one element less than the refused 2 GiB input: accepted, and the tile count is the one the kernel walks"""
    route = L.ConvRoute()
    assert lib.ffa_conv_route(C.byref(_call(B=63, Hi=512, Wi=512, Ho=512, Wo=512)), C.byref(route)) == 0
    assert (route.th, route.tw, route.tiles_x, route.tiles_y, route.ntiles) == (8, 32, 16, 64, 63 * 16 * 64)


def test_calls_with_a_virtual_tensor_of_2_gib_are_served_when_their_stored_tensors_are_smaller(lib, clean_env):
    """The 2 GiB limit is on what a kernel addresses.  The two-source form reads two sources (conv_igemm: each below
    2 GiB; thin skip-less: 64-bit offsets), a dil = 2 call a quarter-size input: calls the training decoder makes at
    large batches, whose statistics buffers the composites of flairhip.ops size from the route of the same call."""
    route = L.ConvRoute()
    big = dict(B=128, Hi=256, Wi=256, Ho=256, Wo=256, Ci=128)  # 128 * 256 * 256 * 128 * 2 bytes = 2 GiB, virtual
    assert lib.ffa_conv_route(C.byref(_call(**big)), C.byref(route)) == -1  # stored: refused in the plain form
    assert lib.ffa_conv_route(C.byref(_call(form=L.CONV_UPCAT, c1=64, stats=SOME, **big)), C.byref(route)) == 0
    assert (route.kernel, route.th, route.tw, route.ntiles) == (0, 8, 32, 128 * 8 * 32)
    thin = dict(bco=32 | L.BCO_THIN | 0x4000, co_rows=32, Ci=32, Co=32, B=128, Hi=512, Wi=512, Ho=512, Wo=512)
    assert lib.ffa_conv_route(C.byref(_call(**thin)), C.byref(route)) == -1
    assert lib.ffa_conv_route(C.byref(_call(form=L.CONV_UPCAT, c1=32, stats=SOME, **thin)), C.byref(route)) == 0
    assert (route.kernel, route.th, route.tw, route.ntiles) == (4, 8, 32, 128 * 64 * 16)
    assert lib.ffa_conv_route(C.byref(_call(dil=2, B=64, Hi=256, Wi=256, Ho=512, Wo=512)), C.byref(route)) == 0
    assert route.ntiles == 64 * 64 * 16
    # the same through the query the composites of flairhip.ops use
    pw = ops.PackedWeight(torch.empty(0, dtype=BF16), 64, 64, 128, 64, 3, 3, 1, 128)
    call = ops._operand_call(L.BF16, pw, 128, 256, 256, form=L.CONV_UPCAT, c1=64, stats=True)
    assert ops._conv_route(call, "two-source").ntiles == 128 * 8 * 32
