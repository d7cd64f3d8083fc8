"""The bytes of every weight-operand layout (GPU): conv_igemm, ring (bf16 and f32), thin and stem operands packed one by
one (ops.pack_conv_weight) and re-packed in a batch (ops.PackBatch.run into operands first packed from zeros) hash to
the sha256 digests of tests/golden/pack_digests.json.

The digests were recorded by tests/golden/gen_pack_digests.py on an MI355X at the last commit that had one set of
packing kernels per layout and per call form (the file's "recorded" field names it); this module uses only Python calls
that exist unchanged there, so it runs as it is in a checkout of that commit.  A digest that differs means the packer is
wrong: the file is never re-recorded for a change of the packing code.

Cases are the smallest at which a packer can go wrong -- row and channel tails, one and several blocks / tiles, the
vector and the scalar load path of the ring16 packer, a column block of a fusion weight -- each as the forward operand,
the transposed (dgrad) operand where the kernel is 3x3, and the forward operand with a per-row scale (one-off only:
PackBatch re-packs training weights, which have none).  The bco the planner returned is recorded beside each digest,
and the forward form of a case must land in the layout it is listed under."""
import hashlib
import json
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")
BF16, F32 = torch.bfloat16, torch.float32
SWITCHES = ("FFA_RING", "FFA_THIN", "FFA_STEM")  # ffa_conv_plan reads them per call

# layout -> (dtypes, environment, [(O, I, k, stride, pitch forward, pitch transposed, pack_conv_weight keywords)])
GROUPS = {
    "igemm": ((BF16, F32), {}, [
        (19, 5, 3, 1, 16, 32, {"allow_thin": False}),   # one 32-row block, row and channel tails
        (70, 40, 3, 2, 48, 80, {}),                     # two 64-row blocks (fragment order), stride 2
        (96, 200, 1, 1, 208, None, {}),                 # 1x1, 13 chunks
        (64, 5, 7, 2, 16, None, {"allow_stem": False}), # 7x7: row groups of one kernel row
        (128, 64, 3, 1, 64, 128, {"allow_ring": False}),
    ]),
    "ring16": ((BF16,), {}, [
        (64, 64, 3, 1, 64, 64, {}),    # 16-byte loads throughout
        (70, 60, 3, 1, 64, 96, {}),    # row tail; the last slot of a row is scalar beside vector ones
        (64, 62, 3, 1, 64, 64, {}),    # row stride of the master not a multiple of 4 floats: all scalar
        (70, 72, 3, 1, 96, 96, {}),    # both operands in the ring layout with row and channel tails, three chunks
    ]),
    "ring_f32": ((F32,), {"FFA_RING": "1"}, [
        (64, 64, 3, 1, 64, 64, {}),
        (70, 48, 3, 1, 48, 80, {}),
    ]),
    "thin": ((BF16,), {}, [
        (16, 16, 3, 1, 16, 16, {}),    # one tile
        (12, 5, 3, 1, 16, 16, {}),
        (32, 32, 3, 1, 32, 32, {}),    # two tiles
        (19, 20, 3, 1, 32, 32, {}),
        (32, 9, 3, 1, 16, 32, {}),
    ]),
    "stem": ((BF16,), {}, [
        (64, 5, 7, 2, 16, None, {}),
        (64, 8, 7, 2, 16, None, {}),
    ]),
}
COLS = (64, 48, 16, 24)  # the column block W[:, 16:40] of a 64 x 48 1x1 fusion weight (conv_igemm layout, both dtypes)


def _sha(pw) -> str:
    return hashlib.sha256(pw.data.view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _name(dtype) -> str:
    return "bf16" if dtype == BF16 else "f32"


def _inputs(key: str, O: int, I: int, k: int, dev):
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    w = torch.randn(O, I, k, k, generator=g)
    scale = torch.rand(O, generator=g) + 0.5
    return w.to(dev), scale.to(dev)


def pack_group(layout: str, dev):
    """{key: (bco, sha256 of the one-off pack, sha256 of the batched pack or None)} for one layout; the caller has set
    the group's environment"""
    from flairhip import lib as L, ops
    bits = {"igemm": 0, "ring16": L.BCO_RING, "ring_f32": L.BCO_RING, "thin": L.BCO_THIN, "stem": L.BCO_STEM}[layout]
    dtypes, _, cases = GROUPS[layout]
    out = {}
    for dtype in dtypes:
        entries, keys = [], []
        for O, I, k, stride, pitch_f, pitch_t, kw in cases:
            case = f"{layout}/{_name(dtype)}/{O}x{I}k{k}s{stride}"
            w, scale = _inputs(case, O, I, k, dev)
            for form in ("forward", "transposed", "scaled"):
                if form == "transposed" and (k != 3 or layout == "stem"):
                    continue
                tr = form == "transposed"
                args = dict(transpose=tr, **kw)
                one = ops.pack_conv_weight(w, dtype, stride, pitch_t if tr else pitch_f,
                                           scale=scale if form == "scaled" else None, **args)
                if not tr:
                    assert one.bco & (L.BCO_RING | L.BCO_THIN | L.BCO_STEM) == bits, (case, form, hex(one.bco))
                out[f"{case}/{form}"] = [one.bco, _sha(one), None]
                if form != "scaled":
                    dst = ops.pack_conv_weight(torch.zeros_like(w), dtype, stride, pitch_t if tr else pitch_f, **args)
                    assert dst.bco == one.bco and _sha(dst) != _sha(one)
                    entries.append((w, dst, tr))
                    keys.append(f"{case}/{form}")
        if layout == "igemm":
            O, I, off, c = COLS
            case = f"igemm/{_name(dtype)}/{O}x{I}k1s1[{off}:{off + c}]"
            w, scale = _inputs(case, O, I, 1, dev)
            block = w[:, off:off + c].contiguous()  # the one-off pack reads a copy, the batched one the whole tensor
            for form in ("forward", "transposed", "scaled"):
                tr = form == "transposed"
                pitch = ops.pad_channels(O if tr else c)
                one = ops.pack_conv_weight(block, dtype, 1, pitch, transpose=tr, scale=scale if form == "scaled" else None)
                assert one.bco & (L.BCO_RING | L.BCO_THIN | L.BCO_STEM) == 0
                out[f"{case}/{form}"] = [one.bco, _sha(one), None]
                if form != "scaled":
                    dst = ops.pack_conv_weight(torch.zeros_like(block), dtype, 1, pitch, transpose=tr)
                    entries.append((w, dst, tr, (off, c)))
                    keys.append(f"{case}/{form}")
        ops.PackBatch(entries, dtype).run()
        torch.cuda.synchronize()
        for key, e in zip(keys, entries):
            out[key][2] = _sha(e[1])
    return out


@pytest.mark.parametrize("layout", sorted(GROUPS))
def test_packed_operand_bytes_match_the_recorded_digests(cuda, monkeypatch, layout):
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in GROUPS[layout][1].items():
        monkeypatch.setenv(name, value)
    got = pack_group(layout, cuda)
    assert sorted(got) == sorted(k for k in golden if k.split("/")[0] == layout)
    wrong = []
    for key, (bco, one, batched) in got.items():
        want = golden[key]
        if bco != want["bco"]:
            wrong.append((key, "bco", hex(bco), hex(want["bco"])))
        if one != want["sha256"]:
            wrong.append((key, "one-off"))
        if batched is not None and batched != want["sha256"]:
            wrong.append((key, "batched"))
    assert not wrong, wrong
