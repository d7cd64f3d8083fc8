"""Every convolution route at the smallest shapes that still have tile edges, held to the float64 rounding bound.

The in-situ tests (tests/test_insitu_*.py) compare every call of a step element by element with float64 -- but only at
the shapes the models produce; the stand-alone kernel tests reach ragged shapes -- but under one number per tensor
(max|ref| * 2^-7 for bf16), which passes a kernel that rounds the partial sum of each half of the input channels to bf16
(tests/test_insitu_checker.py keeps that on file).  This module calls flairhip.ops directly under
insitu.Recorder(mode="full", chunk=1), so the references and bounds are those of tests/insitu.py
(|o - r| <= ulp_stored(r) + 2^-16 a, f32 sums 2^-16 a, pad channels exactly zero); it brings no tolerance of its own.

Shapes (output tiles: 8 x 32 where Wo >= 32, else 16 x 16; thin 8 / 16 x 32; weight gradient 4 / 8 x 32 and 8 / 16 x 16):
9 x 33 (2 x 2 wide tiles, ragged by one row and one column), 17 x 17 and 17 x 31 (narrow tiles ragged by 1 and by 15),
3 x 5 and 1 x 1 (below a tile: the bottom of a 96 x 160 and of a 32 x 32 U-Net), stride-2 inputs of both parities in each
dimension (17 x 35 / 18 x 34; stem 18 x 66 / 19 x 35) with the dil = 2 input gradient asked for each of those sizes, and
the two-source / pooled forms at lo 5 x 17 and 9 x 9.  B = 3: the tile count is never a multiple of 8, so the grid's
rounding to eights leaves idle blocks.  Each case runs with the default grids and with every grid cap at 8, where 12
tiles are walked by 8 blocks.

Each call asks ops._conv_route what the library runs for it and compares with the case table; the last two tests hold
the union of the reached routes / weight-gradient plans to the listed sets, so a router change that moves a case is
noticed.  There is no route query for the weight gradient: its cases state which branch of wgrad_plan / launch_wgrad
(csrc/conv_wgrad.hip) they satisfy and why, and the slab count -- which decides the reduce kernel -- is derived from
ffa_conv_wgrad_workspace_bytes and the block sizes stated."""
import os
import time
import zlib
from collections import Counter

import pytest
import torch

from insitu import Recorder

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
B = 3
GRID_CAPS = ("FFA_RING_GRID", "FFA_THIN_GRID", "FFA_STEM_GRID", "FFA_CONV_PERSIST_GRID")
SWITCHES = GRID_CAPS + ("FFA_RING", "FFA_RING_CFG", "FFA_THIN", "FFA_STEM", "FFA_CONV_PERSIST", "FFA_CONV_PERSIST_MIN",
                        "FFA_THIN_WGRAD", "FFA_WGRAD64", "FFA_STEM_WGRAD8", "FFA_WG_REDUCE_V1")
KERNELS = {0: "igemm", 1: "persist", 2: "ring", 3: "ring16", 4: "thin", 5: "stem"}
MOM, EPS = 0.1, 1e-5

S1_SHAPES = ((9, 33), (17, 17), (17, 31), (3, 5))
S2_SHAPES = ((17, 35), (18, 34))
STEM_SHAPES = ((18, 66), (19, 35))
LO_SHAPES = ((5, 17), (9, 9))


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _cdiv(a, b):
    return (a + b - 1) // b


def _gen(*parts):
    return torch.Generator().manual_seed(zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF)


# --------------------------------------------------------------------------------------------------
# case tables.  A route is "kernel:variant:THxTW" (variant: conv_igemm's halo depth in 32-byte channel groups, the ring
# kernels' tile configuration); per direction the pair (route where the output is >= 32 wide, route where narrower).

def _layer(name, dtype, cin, cout, routes, k=3, stride=1, pad=1, cip=None, cop=None, env=None, ring=True, thin=True,
           one=False, dres=False, epi=False, bias=False):
    return dict(name=name, dtype=dtype, cin=cin, cout=cout, k=k, stride=stride, pad=pad, cip=cip or _cdiv(cin, 16) * 16,
                cop=cop or _cdiv(cout, 16) * 16, env=env or {}, ring=ring, thin=thin, one=one, dres=dres, epi=epi,
                bias=bias, routes=routes)


NO_PERSIST = {"FFA_CONV_PERSIST": "0"}
# 3 x 3 stride 1 pad 1.  one: also at 1 x 1 (the routes with >= 64 channels); dres: the dgrad also with a residual;
# epi: bias + residual + ReLU and conv2d_bn_stats (one case per layout).
S1_CASES = [
    _layer("thin16_16-16", BF16, 16, 16, {"fwd": ("thin:0:16x32",) * 2, "dgrad": ("thin:0:16x32",) * 2}),
    _layer("thin32_32-32", BF16, 32, 32, {"fwd": ("thin:0:8x32",) * 2, "dgrad": ("thin:0:8x32",) * 2}, dres=True, epi=True),
    # 19 classes stored at pitch 32, 30 real input channels at pitch 32
    _layer("thin32_30-19", BF16, 30, 19, {"fwd": ("thin:0:8x32",) * 2, "dgrad": ("thin:0:8x32",) * 2}, cop=32),
    # its dgrad is the thin operand 19 -> 16 that reads a pitch of 32
    _layer("thin_16-19", BF16, 16, 19, {"fwd": ("thin:0:16x32",) * 2, "dgrad": ("thin:0:8x32",) * 2}, cop=32),
    _layer("ring16_64-64", BF16, 64, 64, {"fwd": ("ring16:1:8x32", "ring16:2:16x16"),
                                          "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, one=True, dres=True, epi=True),
    # 96 channels: three 64-byte chunks, the halo buffers swap roles between tiles
    _layer("ring16_96-64", BF16, 96, 64, {"fwd": ("ring16:1:8x32", "ring16:2:16x16"),
                                          "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, one=True),
    _layer("ring16_192-128", BF16, 192, 128, {"fwd": ("ring16:1:8x32", "ring16:2:16x16"),
                                              "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, one=True),
    # cfg 4 (128 rows per block, eight waves) exists for wide maps; narrow ones fall back to cfg 2
    _layer("ring16cfg4_128-128", BF16, 128, 128, {"fwd": ("ring16:4:8x32", "ring16:2:16x16"),
                                                  "dgrad": ("ring16:4:8x32", "ring16:2:16x16")},
           env={"FFA_RING_CFG": "4"}, one=True),
    # 48 channels = three 32-byte groups: halo depth 1, the plain conv_igemm_kernel in both directions
    _layer("igemm1_48-48", BF16, 48, 48, {"fwd": ("igemm:1:8x32", "igemm:1:16x16"),
                                          "dgrad": ("igemm:1:8x32", "igemm:1:16x16")}),
    # fewer than 64 rows: no ring operand; six / four 32-byte groups: halo depth 2 / 4.  Their dgrads are 32 -> 96 / 64
    # convolutions over ONE 64-byte chunk on the ring16 kernel
    _layer("igemm2_96-32", BF16, 96, 32, {"fwd": ("persist:2:8x32", "persist:2:16x16"),
                                          "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, one=True),
    _layer("igemm4_64-32", BF16, 64, 32, {"fwd": ("persist:4:8x32", "persist:4:16x16"),
                                          "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, one=True, epi=True),
    _layer("igemm2np_96-32", BF16, 96, 32, {"fwd": ("igemm:2:8x32", "igemm:2:16x16"),
                                            "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, env=NO_PERSIST, one=True),
    _layer("igemm4np_64-32", BF16, 64, 32, {"fwd": ("igemm:4:8x32", "igemm:4:16x16"),
                                            "dgrad": ("ring16:1:8x32", "ring16:2:16x16")}, env=NO_PERSIST, one=True),
    # the same operands kept off the ring layout: the dgrad side of the conv_igemm 3 x 3 kernels (halo depth 2 and 4 of
    # a 32- and a 64-channel gradient), persistent and not
    _layer("igemm_noring_64-64", BF16, 64, 64, {"fwd": ("persist:4:8x32", "persist:4:16x16"),
                                                "dgrad": ("persist:4:8x32", "persist:4:16x16")}, ring=False, one=True,
           dres=True),
    _layer("igemm_noring_np_96-32", BF16, 96, 32, {"fwd": ("igemm:2:8x32", "igemm:2:16x16"),
                                                   "dgrad": ("igemm:2:8x32", "igemm:2:16x16")}, env=NO_PERSIST, ring=False),
    # f32: 32-byte groups of 8 channels -- 16 -> depth 2, 32 -> depth 4, 48 -> depth 2
    _layer("f32_16-16", F32, 16, 16, {"fwd": ("persist:2:8x32", "persist:2:16x16"),
                                      "dgrad": ("persist:2:8x32", "persist:2:16x16")}),
    _layer("f32_32-64", F32, 32, 64, {"fwd": ("persist:4:8x32", "persist:4:16x16"),
                                      "dgrad": ("persist:4:8x32", "persist:4:16x16")}, dres=True, epi=True),
    _layer("f32_48-32", F32, 48, 32, {"fwd": ("persist:2:8x32", "persist:2:16x16"),
                                      "dgrad": ("persist:4:8x32", "persist:4:16x16")}),
    _layer("f32ring_64-64", F32, 64, 64, {"fwd": ("ring:1:8x32", "ring:2:16x16"), "dgrad": ("ring:1:8x32", "ring:2:16x16")},
           env={"FFA_RING": "1"}, one=True, dres=True, epi=True),
]

IG = ("igemm:1:8x32", "igemm:1:16x16")
# a transposed 3 x 3 operand is a stride-1 one: deep halo over the 128 / 512 channels of dy
IG4 = ("igemm:4:8x32", "igemm:4:16x16")
# stride 2 (3 x 3 pad 1, 1 x 1 pad 0, 7 x 7 pad 3) and the 1 x 1 stride-1 layer with a bias; every one in bf16 and f32.
# The input gradient of a stride-2 layer is the dil = 2 call (conv_igemm only); a transposed 7 x 7 operand does not
# exist (the stem is the first layer): pack_conv_weight refuses it.
S2_CASES = [
    _layer(f"{_name(dt)}_{tag}", dt, cin, cout, routes(dt), k=k, stride=s, pad=p, **kw)
    for dt in (BF16, F32)
    for tag, cin, cout, k, s, p, routes, kw in (
        ("3x3s2_64-128", 64, 128, 3, 2, 1, lambda dt: {"fwd": IG, "dgrad_dil2": IG4}, dict(epi=True)),
        ("3x3s2_256-512", 256, 512, 3, 2, 1, lambda dt: {"fwd": IG, "dgrad_dil2": IG4}, {}),
        ("1x1s2_64-128", 64, 128, 1, 2, 0, lambda dt: {"fwd": IG, "dgrad_dil2": IG}, {}),
        ("1x1s1_128-64", 128, 64, 1, 1, 0, lambda dt: {"fwd": IG, "dgrad": IG}, dict(bias=True)),
        # 5 channels at pitch 16: the stem layout in bf16 (16 x 32 output tiles), conv_igemm<7, 7, 2> in f32
        ("7x7s2_5-64", 5, 64, 7, 2, 3,
         lambda dt: {"fwd": ("stem:0:16x32",) * 2 if dt == BF16 else IG, "dgrad_dil2": "refused"},
         dict(epi=True)),
        # more than 8 input channels: no stem operand
        ("7x7s2_12-64", 12, 64, 7, 2, 3, lambda dt: {"fwd": IG, "dgrad_dil2": "refused"}, {}),
    )
]


def _up(dtype, c1, c2, cout, fwd, pooled, wgrad=True, supported=True):
    return dict(name=f"{_name(dtype)}_{c1}+{c2}-{cout}", dtype=dtype, c1=c1, c2=c2, cout=cout, fwd=fwd, pooled=pooled,
                wgrad=wgrad, supported=supported)


# conv over cat(nearest_x2(lo), skip) and its gradients.  Operands are packed with the ring layout off, as the decoder
# packs them.  "refused": the library has no kernel for the split, the op returns None and the caller materialises.
UP_CASES = [
    _up(BF16, 128, 64, 64, ("igemm:4:8x32", "igemm:4:16x16"), ("igemm:4:8x32", "igemm:4:16x16")),
    _up(BF16, 64, 64, 32, ("igemm:4:8x32", "igemm:4:16x16"), ("igemm:2:8x32", "igemm:2:16x16")),
    _up(BF16, 32, 0, 16, ("thin:0:8x32",) * 2, ("thin:0:16x32",) * 2),   # skip-less: the thin layout, both directions
    # 48 channels = three 32-byte groups: no deep halo, no two-source loader; 32 is neither a 64-row block of the pooled
    # form nor a 64-channel block of the weight gradient
    _up(BF16, 32, 16, 32, "refused", "refused", wgrad=False, supported=False),
    _up(F32, 128, 64, 64, ("igemm:4:8x32", "igemm:4:16x16"), ("igemm:4:8x32", "igemm:4:16x16")),
    _up(F32, 64, 64, 32, ("igemm:4:8x32", "igemm:4:16x16"), ("igemm:4:8x32", "igemm:4:16x16")),
    _up(F32, 32, 0, 16, ("igemm:4:8x32", "igemm:4:16x16"), ("igemm:2:8x32", "igemm:2:16x16")),
    # f32: six 32-byte groups (depth 2) and 32-channel weight-gradient blocks take the split; the pooled form does not
    # (48 rows are one 64-row block)
    _up(F32, 32, 16, 32, ("igemm:2:8x32", "igemm:2:16x16"), "refused"),
]


def _wg(name, dtype, cin, cout, plan, blocks, why, reduces, k=3, stride=1, pad=1, cip=None, cop=None, shapes=S1_SHAPES,
        one=False, acc=True):
    return dict(name=name, dtype=dtype, cin=cin, cout=cout, plan=plan, blocks=blocks, why=why, reduces=set(reduces), k=k,
                stride=stride, pad=pad, cip=cip or _cdiv(cin, 16) * 16, cop=cop or _cdiv(cout, 16) * 16, shapes=shapes,
                one=one, acc=acc)


R32, R4, R3X3_32, R3X3_4 = "wgrad_reduce<32>", "wgrad_reduce<4>", "wgrad_reduce3x3<32>", "wgrad_reduce3x3<4>"
# Weight gradients.  plan: the branch of wgrad_plan / launch_wgrad the case satisfies; blocks: the (Co, Ci) channels of
# one block = 32 * (wco, wci) of that branch (None: the thin kernel, whole tensors), from which the padded slab size and
# so the slab count follow; reduces: the reduce kernels its shapes reach at B = 3 and B = 1 (more than 8 slabs: <32>,
# else <4>; 3 x 3 with Co_real * ceil(ceil(Ci_real / 4) / (8 or 64)) >= 512 blocks: wgrad_reduce3x3_kernel).
WG_CASES = [
    _wg("thin_16-16", BF16, 16, 16, "thin", None, "bf16 3x3 s1, both pitches 16", {R32, R4}),
    _wg("thin_32-32", BF16, 32, 32, "thin", None, "bf16 3x3 s1, both pitches 32", {R32, R4}),
    _wg("thin_30-19", BF16, 30, 19, "thin", None, "bf16 3x3 s1, both pitches 32 (19 and 30 real)", {R32, R4}, cop=32),
    _wg("wgrad64_64-64", BF16, 64, 64, "wgrad64", (64, 64), "Co, Ci > 32 -> 2 x 2 waves, wk 2; both % 64 == 0, pad 1",
        {R32, R4}, one=True),
    _wg("wgrad64_128-64", BF16, 128, 64, "wgrad64", (64, 64), "as 64 -> 64 with two input-channel blocks", {R32, R4},
        one=True),
    _wg("wgrad64_128-128", BF16, 128, 128, "wgrad64", (64, 64), "128 * ceil(32 / 8) = 512 reduce blocks at > 8 slabs",
        {R3X3_32, R4}, one=True),
    _wg("general222_64-96", BF16, 64, 96, "general(2,2,2)", (64, 64), "2 x 2 waves, but Co = 96 is no multiple of 64",
        {R32, R4}, one=True),
    _wg("general212_32-64", BF16, 32, 64, "general(2,1,2)", (64, 32), "Co > 32, Ci <= 32 -> wk = 4 / 2", {R32, R4}),
    _wg("general122_64-32", BF16, 64, 32, "general(1,2,2)", (32, 64), "Co <= 32, Ci > 32 -> wk = 4 / 2", {R32, R4}),
    _wg("general114_32-24", BF16, 32, 24, "general(1,1,4)", (32, 32), "both <= 32 and a dy pitch of 24: not thin, wk 4",
        {R32, R4}, cop=24),
    _wg("f32_211_32-64", F32, 32, 64, "f32(2,1,1)", (64, 32), "f32: one ci plane per block, Co > 32", {R32, R4}),
    _wg("f32_111_16-16", F32, 16, 16, "f32(1,1,1)", (32, 32), "f32, Co <= 32", {R32, R4}),
] + [
    _wg(f"{_name(dt)}_{tag}", dt, cin, cout, f"{_name(dt)} {tag.split('_')[0]}", (64, 64 if dt == BF16 else 32), why,
        red(dt), k=k, stride=s, pad=p, shapes=S2_SHAPES, acc=acc)
    for dt in (BF16, F32)
    for tag, cin, cout, k, s, p, why, red, acc in (
        ("3x3s2_64-128", 64, 128, 3, 2, 1, "strided kernels: 4 x 16 tiles, 2 x (2 | f32: 1) waves",
         lambda dt: {R32, R4}, True),
        ("3x3s2_256-512", 256, 512, 3, 2, 1,
         "512 * ceil(64 / 64) = 512 reduce blocks at <= 8 slabs (f32: 64 tile blocks, so 8 slabs at B = 3 too)",
         lambda dt: {R3X3_32, R3X3_4} if dt == BF16 else {R3X3_4}, False),
        ("1x1s2_64-128", 64, 128, 1, 2, 0, "strided kernels", lambda dt: {R32, R4}, True),
        ("1x1s1_128-64", 128, 64, 1, 1, 0, "1 x 1 stride 1: 4 x 16 tiles, more than 8 slabs even at B = 1",
         lambda dt: {R32}, True),
    )
] + [
    _wg("stem8_5-64", BF16, 5, 64, "stem_wgrad8", (64, 16), "bf16 7x7, <= 8 real channels at pitch 16, Co = 64, pad 3",
        {R32, R4}, k=7, stride=2, pad=3, shapes=STEM_SHAPES),
    _wg("stem_12-64", BF16, 12, 64, "stem_wgrad", (64, 16), "bf16 7x7, pitch 16 but more than 8 real channels", {R32, R4},
        k=7, stride=2, pad=3, shapes=STEM_SHAPES),
    _wg("f32_7x7_5-64", F32, 5, 64, "f32 7x7", (64, 32), "conv_wgrad_kernel<7, 7, 2>, one launch row per kernel row",
        {R32, R4}, k=7, stride=2, pad=3, shapes=STEM_SHAPES),
    _wg("f32_7x7_12-64", F32, 12, 64, "f32 7x7", (64, 32), "as 5 -> 64", {R32, R4}, k=7, stride=2, pad=3,
        shapes=STEM_SHAPES, acc=False),
]

# the listed sets: (dtype, direction, route) of every forward / input-gradient route named in the case tables ...
ROUTES = {
    ("bf16", "fwd", "thin:0:16x32"), ("bf16", "fwd", "thin:0:8x32"), ("bf16", "dgrad", "thin:0:16x32"),
    ("bf16", "dgrad", "thin:0:8x32"),
    ("bf16", "fwd", "ring16:1:8x32"), ("bf16", "fwd", "ring16:2:16x16"), ("bf16", "fwd", "ring16:4:8x32"),
    ("bf16", "dgrad", "ring16:1:8x32"), ("bf16", "dgrad", "ring16:2:16x16"), ("bf16", "dgrad", "ring16:4:8x32"),
    ("bf16", "fwd", "igemm:1:8x32"), ("bf16", "fwd", "igemm:1:16x16"), ("bf16", "dgrad", "igemm:1:8x32"),
    ("bf16", "dgrad", "igemm:1:16x16"),
    ("bf16", "fwd", "persist:2:8x32"), ("bf16", "fwd", "persist:2:16x16"), ("bf16", "fwd", "persist:4:8x32"),
    ("bf16", "fwd", "persist:4:16x16"), ("bf16", "dgrad", "persist:4:8x32"), ("bf16", "dgrad", "persist:4:16x16"),
    ("bf16", "fwd", "igemm:2:8x32"), ("bf16", "fwd", "igemm:2:16x16"), ("bf16", "fwd", "igemm:4:8x32"),
    ("bf16", "fwd", "igemm:4:16x16"), ("bf16", "dgrad", "igemm:2:8x32"), ("bf16", "dgrad", "igemm:2:16x16"),
    ("bf16", "fwd", "stem:0:16x32"), ("bf16", "dgrad_dil2", "igemm:1:8x32"), ("bf16", "dgrad_dil2", "igemm:4:8x32"),
    ("bf16", "upcat", "igemm:4:8x32"), ("bf16", "upcat", "igemm:4:16x16"), ("bf16", "upcat", "thin:0:8x32"),
    ("bf16", "pooled", "igemm:4:8x32"), ("bf16", "pooled", "igemm:4:16x16"), ("bf16", "pooled", "igemm:2:8x32"),
    ("bf16", "pooled", "igemm:2:16x16"), ("bf16", "pooled", "thin:0:16x32"),
    ("f32", "fwd", "persist:2:8x32"), ("f32", "fwd", "persist:2:16x16"), ("f32", "fwd", "persist:4:8x32"),
    ("f32", "fwd", "persist:4:16x16"), ("f32", "dgrad", "persist:2:8x32"), ("f32", "dgrad", "persist:2:16x16"),
    ("f32", "dgrad", "persist:4:8x32"), ("f32", "dgrad", "persist:4:16x16"),
    ("f32", "fwd", "ring:1:8x32"), ("f32", "fwd", "ring:2:16x16"), ("f32", "dgrad", "ring:1:8x32"),
    ("f32", "dgrad", "ring:2:16x16"),
    ("f32", "fwd", "igemm:1:8x32"), ("f32", "fwd", "igemm:1:16x16"), ("f32", "dgrad", "igemm:1:8x32"),
    ("f32", "dgrad_dil2", "igemm:1:8x32"), ("f32", "dgrad_dil2", "igemm:4:8x32"),
    ("f32", "upcat", "igemm:4:8x32"), ("f32", "upcat", "igemm:4:16x16"), ("f32", "upcat", "igemm:2:8x32"),
    ("f32", "upcat", "igemm:2:16x16"), ("f32", "pooled", "igemm:4:8x32"), ("f32", "pooled", "igemm:4:16x16"),
    ("f32", "pooled", "igemm:2:8x32"), ("f32", "pooled", "igemm:2:16x16"),
}
# ... and (plan, reduce kernel) of every weight-gradient plan with each reduce kernel its cases reach
WG_PLANS = {(c["plan"], r) for c in WG_CASES for r in c["reduces"]}
WG_PLAN_NAMES = {"thin", "wgrad64", "general(2,2,2)", "general(2,1,2)", "general(1,2,2)", "general(1,1,4)", "f32(2,1,1)",
                 "f32(1,1,1)", "bf16 3x3s2", "bf16 1x1s2", "bf16 1x1s1", "f32 3x3s2", "f32 1x1s2", "f32 1x1s1", "stem_wgrad8",
                 "stem_wgrad", "f32 7x7"}


# --------------------------------------------------------------------------------------------------
# one context per test: asks the route of every call, and -- with a recorder -- makes the call

class Ctx:
    """rec = None: routes and plans only (no tensor, no launch: the coverage tests), operands planned as
    ops.pack_conv_weight plans them; with a Recorder: the same, and every call is made on `dev` under it."""

    def __init__(self, rec=None, dev=None):
        from flairhip import lib as L, ops
        self.ops, self.L, self.rec, self.dev = ops, L, rec, dev
        self.run = rec is not None
        self.made = []        # ops names of the calls made, in order
        self.reached = set()  # (dtype, direction, route)
        self.wg_reached = set()  # (plan, reduce kernel)
        self._operands = {}

    # ---- operands ----------------------------------------------------------------------------------

    def weight(self, lay):
        g = _gen(lay["name"], "w")
        w = torch.randn(lay["cout"], lay["cin"], lay["k"], lay["k"], generator=g) * (lay["cin"] * lay["k"] ** 2) ** -0.5
        return w.to(self.dev)

    def operand(self, lay, transpose):
        """the layer's forward / transposed operand (None: the library has none), packed once per test and registered"""
        key = (lay["name"], transpose)
        if key in self._operands:
            return self._operands[key]
        ops, lib = self.ops, self.L.load()
        O, I, k, stride, pad, dtype = lay["cout"], lay["cin"], lay["k"], lay["stride"], lay["pad"], lay["dtype"]
        ring, thin, stem = lay["ring"] and pad == 1, lay["thin"] and pad == 1, pad == 3  # HipConv2d.allow
        pitch = lay["cop"] if transpose else lay["cip"]
        rows_real, use_stride = (I, 1) if transpose else (O, stride)
        plain = not (transpose and stride != 1)
        bco = lib.ffa_conv_plan(ops._dtype_id(dtype), k, k, use_stride, rows_real, pitch,
                                (1 if ring and plain else 0) | (2 if thin and plain else 0) |
                                (4 if stem and not transpose and I <= 8 else 0))
        pw = None
        if bco > 0:
            blk = bco & 0xFFF
            pw = ops.PackedWeight(torch.empty(0, dtype=dtype), _cdiv(rows_real, blk) * blk, rows_real, pitch, bco, k, k,
                                  use_stride, O if transpose else I)
        if self.run:
            w = lay.get("w")
            if w is None:
                w = lay["w"] = self.weight(lay)
            if pw is None:
                with pytest.raises(self.L.FlairHipError):
                    ops.pack_conv_weight(w, dtype, stride, pitch, transpose=transpose, allow_ring=ring, allow_thin=thin,
                                         allow_stem=stem)
            else:
                real = ops.pack_conv_weight(w, dtype, stride, pitch, transpose=transpose, allow_ring=ring, allow_thin=thin,
                                            allow_stem=stem)
                assert (real.rows, real.rows_real, real.ci_pitch, real.bco, real.stride, real.ch_real) == \
                    (pw.rows, pw.rows_real, pw.ci_pitch, pw.bco, pw.stride, pw.ch_real)
                pw = self.rec.register_operand(real, w, transpose=transpose, stride=stride, padding=pad, name=lay["name"])
        self._operands[key] = pw
        return pw

    # ---- routes ------------------------------------------------------------------------------------

    def route(self, form, dtype, pw, geom, pad, dil=1, c1=0, relu=False, bias=False, residual=False, stats=False):
        call = self.ops._conv_call(form, self.ops._dtype_id(dtype), pw, geom, pad, dil, relu, c1)
        call.bias, call.residual, call.stats = (1 if bias else None), (1 if residual else None), (1 if stats else None)
        r = self.ops._conv_route(call)  # (the router reads only whether an optional pointer is null)
        return "refused" if r is None else f"{KERNELS[r.kernel]}:{r.variant}:{r.th}x{r.tw}"

    def expect(self, name, dtype, direction, want, out_w, got):
        if not isinstance(want, str):
            want = want[0] if out_w >= 32 else want[1]
        assert got == want, f"{name} {direction} at output width {out_w}: routed to {got}, the case table says {want}"
        if got != "refused":
            self.reached.add((_name(dtype), direction, got))
        return got

    # ---- tensors -----------------------------------------------------------------------------------

    def act(self, g, b, h, w, c, pitch, dtype):
        t = torch.zeros(b, h, w, pitch)
        t[..., :c] = torch.randn(b, h, w, c, generator=g)
        return t.to(dtype).to(self.dev)

    def vec(self, g, c, pitch, scale=1.0, shift=0.0):
        v = torch.zeros(pitch)
        v[:c] = torch.randn(c, generator=g) * scale + shift
        return v.to(self.dev)

    def bn(self, g, C):
        return (self.vec(g, C, C, 0.25, 1.0), self.vec(g, C, C, 0.1), self.vec(g, C, C, 0.1),
                (torch.rand(C, generator=g) + 0.5).to(self.dev))

    # ---- calls -------------------------------------------------------------------------------------

    def fwd(self, lay, hw, bias=False, residual=False, relu=False, stats=False):
        ops, dt = self.ops, lay["dtype"]
        H, W = hw
        Ho, Wo = (ops.conv_out_size(v, lay["k"], lay["stride"], lay["pad"]) for v in hw)
        pw = self.operand(lay, False)
        got = self.route(self.L.CONV_PLAIN, dt, pw, (B, H, W, Ho, Wo, lay["cop"]), lay["pad"], relu=relu, bias=bias,
                         residual=residual, stats=stats)
        self.expect(lay["name"], dt, "fwd", lay["routes"]["fwd"], Wo, got)
        if not self.run:
            return
        g = _gen(lay["name"], "fwd", hw, bias, residual, relu, stats)
        x = self.act(g, B, H, W, lay["cin"], lay["cip"], dt)
        if stats:
            gamma, beta, rm, rv = self.bn(g, lay["cop"])
            ops.conv2d_bn_stats(x, pw, lay["pad"], lay["cop"], gamma, beta, rm, rv, MOM, EPS)
            self.made.append("conv2d_bn_stats")
            return
        bd = self.vec(g, lay["cout"], lay["cop"]) if bias else None
        rd = self.act(g, B, Ho, Wo, lay["cout"], lay["cop"], dt) if residual else None
        ops.conv2d(x, pw, lay["pad"], lay["cop"], bias=bd, residual=rd, relu=relu)
        self.made.append("conv2d")

    def dgrad(self, lay, hw, residual=False):
        """the input gradient of the layer for an input of size hw: dil = stride, out_hw = hw"""
        ops, dt, k, s = self.ops, lay["dtype"], lay["k"], lay["stride"]
        H, W = hw
        Ho, Wo = (ops.conv_out_size(v, k, s, lay["pad"]) for v in hw)
        direction = "dgrad_dil2" if s == 2 else "dgrad"
        pw = self.operand(lay, True)
        if pw is None:  # refused where the operand is planned (checked there)
            assert lay["routes"][direction] == "refused", f"{lay['name']}: no transposed operand"
            return
        got = self.route(self.L.CONV_PLAIN, dt, pw, (B, Ho, Wo, H, W, lay["cip"]), k - 1 - lay["pad"], dil=s,
                         residual=residual)
        self.expect(lay["name"], dt, direction, lay["routes"][direction], W, got)
        if not self.run:
            return
        g = _gen(lay["name"], "dgrad", hw, residual)
        dy = self.act(g, B, Ho, Wo, lay["cout"], lay["cop"], dt)
        rd = self.act(g, B, H, W, lay["cin"], lay["cip"], dt) if residual else None
        ops.conv2d(dy, pw, k - 1 - lay["pad"], lay["cip"], residual=rd, dil=s, out_hw=(H, W))
        self.made.append("conv2d")

    def upcat(self, case, lay, lo_hw, bias=False, relu=False, stats=False):
        ops, dt, c1, c2 = self.ops, case["dtype"], case["c1"], case["c2"]
        Hl, Wl = lo_hw
        H, W = 2 * Hl, 2 * Wl
        pw = self.operand(lay, False)
        got = self.route(self.L.CONV_UPCAT, dt, pw, (B, H, W, H, W, lay["cop"]), 1, c1=c1, relu=relu, bias=bias, stats=stats)
        self.expect(lay["name"], dt, "upcat", case["fwd"], W, got)
        if not self.run:
            return
        g = _gen(lay["name"], "upcat", lo_hw, bias, relu, stats)
        lo = self.act(g, B, Hl, Wl, c1, c1, dt)
        skip = self.act(g, B, H, W, c2, c2, dt) if c2 else None
        if stats:
            gamma, beta, rm, rv = self.bn(g, lay["cop"])
            if got == "refused":
                with pytest.raises(self.L.FlairHipError):
                    ops.conv2d_upcat_bn_stats(lo, skip, pw, lay["cop"], gamma, beta, rm, rv, MOM, EPS)
                return
            ops.conv2d_upcat_bn_stats(lo, skip, pw, lay["cop"], gamma, beta, rm, rv, MOM, EPS)
            self.made.append("conv2d_upcat_bn_stats")
            return
        bd = self.vec(g, lay["cout"], lay["cop"]) if bias else None
        y = ops.conv2d_upcat(lo, skip, pw, lay["cop"], bias=bd, relu=relu)
        self.made.append("conv2d_upcat")
        assert (y is None) == (got == "refused"), f"{lay['name']}: conv2d_upcat returned {type(y).__name__}, route {got}"

    def pooled(self, case, lay, lo_hw):
        ops, dt, c1, c2 = self.ops, case["dtype"], case["c1"], case["c2"]
        H, W = 2 * lo_hw[0], 2 * lo_hw[1]
        pwt = self.operand(lay, True)
        got = self.route(self.L.CONV_POOLED, dt, pwt, (B, H, W, H, W, c1 + c2), 1, c1=c1)
        self.expect(lay["name"], dt, "pooled", case["pooled"], W, got)
        if not self.run:
            return
        dy = self.act(_gen(lay["name"], "pooled", lo_hw), B, H, W, lay["cout"], lay["cop"], dt)
        pair = ops.conv2d_dgrad_upcat(dy, pwt, c1, c2)
        self.made.append("conv2d_dgrad_upcat")
        assert (pair is None) == (got == "refused"), f"{lay['name']}: conv2d_dgrad_upcat / route {got}"

    def wgrad_upcat(self, case, lay, lo_hw):
        if not self.run:
            return
        ops, dt, c1, c2 = self.ops, case["dtype"], case["c1"], case["c2"]
        Hl, Wl = lo_hw
        g = _gen(lay["name"], "wgrad_upcat", lo_hw)
        lo = self.act(g, B, Hl, Wl, c1, c1, dt)
        skip = self.act(g, B, 2 * Hl, 2 * Wl, c2, c2, dt) if c2 else None
        dy = self.act(g, B, 2 * Hl, 2 * Wl, lay["cout"], lay["cop"], dt)
        dw = ops.conv_wgrad_upcat(lo, skip, dy, lay["cout"])
        self.made.append("conv_wgrad_upcat")
        assert (dw is None) == (not case["wgrad"]), f"{lay['name']}: conv_wgrad_upcat returned {type(dw).__name__}"

    def wgrad(self, c, hw, batch, accumulate=False):
        ops, lib, dt, k, s = self.ops, self.L.load(), c["dtype"], c["k"], c["stride"]
        H, W = hw
        Ho, Wo = (ops.conv_out_size(v, k, s, c["pad"]) for v in hw)
        # slabs: the workspace is slabs * CoT * k * k * CiT floats, CoT / CiT the pitches padded to whole blocks
        need = lib.ffa_conv_wgrad_workspace_bytes(ops._dtype_id(dt), k, k, s, c["cop"], c["cip"], batch, Ho, Wo)
        assert need > 0, f"{c['name']}: no weight-gradient kernel"
        if c["blocks"] is None:  # conv3x3_thin_wgrad_kernel: one slab per persistent block, one block per 8 x 32 tile
            assert dt == BF16 and k == 3 and s == 1 and c["cop"] in (16, 32) and c["cip"] in (16, 32), c["why"]
            slabs = min(batch * _cdiv(Wo, 32) * _cdiv(Ho, 8), 512)
        else:
            bo, bi = c["blocks"]
            cot, cit = _cdiv(c["cop"], bo) * bo, _cdiv(c["cip"], bi) * bi
            if c["plan"].startswith("stem_wgrad"):  # 64 output channels per block, 16-channel slabs
                cot, cit = c["cop"], 16
            slabs, rest = divmod(need, cot * k * k * cit * 4)
            assert rest == 0 and slabs >= 1, \
                f"{c['name']}: workspace of {need} bytes is no whole number of {cot} x {cit} slabs"
        blocks = c["cout"] * _cdiv(_cdiv(c["cin"], 4), 8 if slabs > 8 else 64)
        self.wg_reached.add((c["plan"], ("wgrad_reduce3x3" if k == 3 and blocks >= 512 else "wgrad_reduce") +
                             ("<32>" if slabs > 8 else "<4>")))
        if not self.run:
            return
        g = _gen(c["name"], "wgrad", hw, batch, accumulate)
        x = self.act(g, batch, H, W, c["cin"], c["cip"], dt)
        dy = self.act(g, batch, Ho, Wo, c["cout"], c["cop"], dt)
        if not accumulate:
            ops.conv_wgrad(x, dy, c["cout"], c["cin"], k, k, s, c["pad"])
            self.made.append("conv_wgrad")
            return
        before = torch.randn(c["cout"], c["cin"], k, k, generator=g).to(self.dev)
        first = ops.conv_wgrad(x, dy, c["cout"], c["cin"], k, k, s, c["pad"], out=before.clone(), accumulate=True)
        second = ops.conv_wgrad(x, dy, c["cout"], c["cin"], k, k, s, c["pad"], out=before.clone(), accumulate=True)
        self.made += ["conv_wgrad", "conv_wgrad"]
        assert torch.equal(first, second), f"{c['name']}: accumulate=True is not deterministic"


# ---- what each case calls (the tests with a recorder, the coverage tests without) -------------------

def s1_calls(ctx, lay):
    for hw in S1_SHAPES + (((1, 1),) if lay["one"] else ()):
        ctx.fwd(lay, hw)
        ctx.dgrad(lay, hw)
        if lay["dres"]:
            ctx.dgrad(lay, hw, residual=True)
        if lay["epi"]:
            ctx.fwd(lay, hw, bias=True, residual=True, relu=True)
            ctx.fwd(lay, hw, stats=True)


def s2_calls(ctx, lay):
    stem = lay["k"] == 7
    for hw in (STEM_SHAPES if stem else S2_SHAPES):
        ctx.fwd(lay, hw, bias=lay["bias"])
        ctx.dgrad(lay, hw)
        if not stem:
            ctx.dgrad(lay, hw, residual=True)
        if lay["epi"]:  # (the stem layout takes no residual input)
            ctx.fwd(lay, hw, bias=True, residual=not stem, relu=True)
            ctx.fwd(lay, hw, stats=True)


def up_layer(case):
    c = case["c1"] + case["c2"]
    return _layer(case["name"], case["dtype"], c, case["cout"], {}, ring=False)


def up_calls(ctx, case):
    lay = up_layer(case)
    assert ctx.ops.upcat_supported(case["c1"], case["c2"], case["dtype"]) == case["supported"]
    for lo_hw in LO_SHAPES:
        ctx.upcat(case, lay, lo_hw)
        ctx.upcat(case, lay, lo_hw, bias=True, relu=True)
        ctx.upcat(case, lay, lo_hw, stats=True)
        ctx.pooled(case, lay, lo_hw)
        ctx.wgrad_upcat(case, lay, lo_hw)


def wg_calls(ctx, c):
    shapes = c["shapes"] + (((1, 1),) if c["one"] else ())
    before, ctx.wg_reached = ctx.wg_reached, set()
    for batch in (B, 1):
        for hw in shapes:
            ctx.wgrad(c, hw, batch)
    if c["acc"]:
        ctx.wgrad(c, shapes[0], B, accumulate=True)
    got = {r for _, r in ctx.wg_reached}
    ctx.wg_reached |= before
    assert got == c["reduces"], f"{c['name']}: reduce kernels {sorted(got)}, the case table says {sorted(c['reduces'])}"


# ---- the tests ---------------------------------------------------------------------------------------

def _env(monkeypatch, env, grid):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if grid == "cap8":
        for k in GRID_CAPS:
            monkeypatch.setenv(k, "8")


def _checked(cuda, monkeypatch, env, grid, calls, case, label):
    t0 = time.perf_counter()
    _env(monkeypatch, env, grid)
    case = dict(case)  # (the master weight is kept in the copy)
    with Recorder(mode="full", chunk=1) as rec:
        ctx = Ctx(rec, cuda)
        calls(ctx, case)
        torch.cuda.synchronize()
    print(f"\n[{label}, {grid} grids] {len(rec.calls)} checked calls, FFA_* environment: "
          f"{ {k: v for k, v in os.environ.items() if k.startswith('FFA_')} or 'none'}\n{rec.table()}\n"
          f"wall time {time.perf_counter() - t0:.2f} s")
    fails = rec.failures()
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])
    assert ctx.made and Counter(c["op"] for c in rec.calls) == Counter(ctx.made), \
        f"calls made {dict(Counter(ctx.made))}, calls checked {dict(Counter(c['op'] for c in rec.calls))}"


GRIDS = ("default", "cap8")


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("lay", S1_CASES, ids=[c["name"] for c in S1_CASES])
def test_3x3_stride1_forward_and_dgrad(cuda, monkeypatch, lay, grid):
    _checked(cuda, monkeypatch, lay["env"], grid, s1_calls, lay, lay["name"])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("lay", S2_CASES, ids=[c["name"] for c in S2_CASES])
def test_stride2_1x1_and_7x7_forward_and_dgrad(cuda, monkeypatch, lay, grid):
    _checked(cuda, monkeypatch, lay["env"], grid, s2_calls, lay, lay["name"])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("case", UP_CASES, ids=[c["name"] for c in UP_CASES])
def test_two_source_and_pooled_forms(cuda, monkeypatch, case, grid):
    _checked(cuda, monkeypatch, {}, grid, up_calls, case, case["name"])


@pytest.mark.parametrize("case", WG_CASES, ids=[c["name"] for c in WG_CASES])
def test_weight_gradient(cuda, monkeypatch, case):
    """(the weight-gradient kernels read none of the grid caps: one run per case)"""
    _checked(cuda, monkeypatch, {}, "default", wg_calls, case, case["name"])


def test_union_of_reached_routes_is_the_listed_set(monkeypatch):
    """the routes of every call of the case tables, asked again without tensors: exactly the listed ones"""
    reached = set()
    for grid in GRIDS:
        for cases, calls in ((S1_CASES, s1_calls), (S2_CASES, s2_calls), (UP_CASES, up_calls)):
            for case in cases:
                with monkeypatch.context() as m:
                    _env(m, case.get("env", {}), grid)
                    ctx = Ctx()
                    calls(ctx, case)
                    reached |= ctx.reached
    assert reached == ROUTES, f"not reached: {sorted(ROUTES - reached)}; not listed: {sorted(reached - ROUTES)}"


def test_union_of_reached_weight_gradient_plans_is_the_listed_set(monkeypatch):
    _env(monkeypatch, {}, "default")
    ctx = Ctx()
    for case in WG_CASES:
        wg_calls(ctx, case)
    assert ctx.wg_reached == WG_PLANS
    assert {p for p, _ in ctx.wg_reached} == WG_PLAN_NAMES
    assert {r for _, r in ctx.wg_reached} == {R32, R4, R3X3_32, R3X3_4}
