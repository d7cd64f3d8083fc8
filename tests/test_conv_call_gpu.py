"""Every form of forward / input-gradient convolution call (GPU), through the public functions of flairhip.ops only:
the sha256 of every output tensor over its full pitch, and of the statistics partials over exactly
ops.conv_stat_rows rows, equals tests/golden/conv_call_digests.json.

The digests were recorded by tests/golden/gen_conv_call_digests.py on an MI355X at the last commit at which each form
had an ABI entry of its own (the file's "recorded" field names it); this module uses only Python calls that exist
unchanged there, so it runs as it is in a checkout of that commit.  All reductions of these kernels are fixed-order, so
a digest that differs means a call reaches another kernel, another tile or grid, or hands a kernel another argument:
the file is never re-recorded for a change of the call path.  The generator was run twice there and gave equal tables,
so no call leaves a byte it hashes unwritten.

B = 2 throughout; 24 x 40 gives the 8 x 32 tile with partial tiles on both edges, 16 x 16 the 16 x 16 tile (W < 32).
Each group sets the environment switches it names; the routers read them per call."""
import hashlib
import json
import os
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_call_digests.json")
BF16, F32 = torch.bfloat16, torch.float32
SWITCHES = ("FFA_RING", "FFA_RING_GRID", "FFA_RING_CFG", "FFA_THIN", "FFA_THIN_GRID", "FFA_STEM", "FFA_STEM_GRID",
            "FFA_CONV_PERSIST", "FFA_CONV_PERSIST_MIN", "FFA_CONV_PERSIST_GRID")
B = 2
SIZES = ((24, 40), (16, 16))
IGEMM = {"allow_ring": False, "allow_thin": False, "allow_stem": False}


def _name(dtype) -> str:
    return "bf16" if dtype == BF16 else "f32"


def _sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


class Case:
    """Seeded CPU inputs of one case, and the digests it leaves under ``key/<name>``"""

    def __init__(self, out: dict, key: str, dev):
        self.out, self.key, self.dev = out, key, dev
        self.g = torch.Generator().manual_seed(zlib.crc32(key.encode()))

    def act(self, h: int, w: int, c_real: int, dtype, pitch=None) -> torch.Tensor:
        from flairhip import ops
        pitch = pitch or ops.pad_channels(c_real)
        x = torch.zeros(B, h, w, pitch)
        x[..., :c_real] = torch.randn(B, h, w, c_real, generator=self.g)
        return x.to(dtype).to(self.dev)

    def weight(self, o: int, i: int, k: int) -> torch.Tensor:
        return (torch.randn(o, i, k, k, generator=self.g) / (i * k * k) ** 0.5).to(self.dev)

    def vec(self, n: int, lo: float = -0.5) -> torch.Tensor:
        return (torch.rand(n, generator=self.g) + lo).to(self.dev)

    def stats(self, h: int, w: int, pw, pitch: int):
        from flairhip import ops
        rows = ops.conv_stat_rows(B, h, w, pw)
        return torch.full((rows * 2 * pitch,), float("nan"), device=self.dev), rows

    def put(self, name: str, t) -> None:
        k = f"{self.key}/{name}"
        assert k not in self.out, k
        self.out[k] = "none" if t is None else _sha(t)


def _epilogues(c: Case, h: int, w: int, pw, pitch: int, dtype, call) -> None:
    """call(**keywords of ops.conv2d) plain, then with bias + residual + relu and statistics"""
    c.put("plain", call())
    st, rows = c.stats(h, w, pw, pitch)
    res = c.act(h, w, pitch, dtype)
    c.put("full", call(bias=c.vec(pitch), residual=res, relu=True, stats=st))
    c.put("full_stats", st[:rows * 2 * pitch])


def _igemm_cases(out: dict, dev, dtypes=(BF16, F32), shapes=None) -> None:
    from flairhip import lib as L, ops
    # (name, O, I, k, stride, pad, dil, transposed operand, explicit out_hw)
    shapes = shapes or (
        [(f"3x3s1_p{i}_r{o}", o, i, 3, 1, 1, 1, False, False) for i in (16, 32, 64) for o in (32, 64)] +
        [("3x3s2", 64, 32, 3, 2, 1, 1, False, False), ("1x1s1", 64, 48, 1, 1, 0, 1, False, False),
         ("1x1s2", 64, 48, 1, 2, 0, 1, False, False), ("7x7s2", 64, 5, 7, 2, 3, 1, False, False),
         ("3x3dil2", 32, 64, 3, 2, 1, 2, True, False), ("3x3pad0", 64, 32, 3, 1, 0, 1, False, True)])
    for dtype in dtypes:
        for name, o, i, k, stride, pad, dil, tr, explicit in shapes:
            if k == 7 and dtype != F32:
                continue
            for h, w in SIZES:
                c = Case(out, f"igemm/{_name(dtype)}/{name}/{h}x{w}", dev)
                wt = c.weight(o, i, k)
                cin, cout = (o, i) if tr else (i, o)  # channels of the call's input / output
                pw = ops.pack_conv_weight(wt, dtype, stride, ops.pad_channels(cin), transpose=tr, **IGEMM)
                assert not pw.bco & (L.BCO_RING | L.BCO_THIN | L.BCO_STEM)
                hi, wi = (h // 2, w // 2) if dil == 2 else (h, w)  # dil = 2: the output has the size h x w
                x = c.act(hi, wi, cin, dtype)
                ho = ops.conv_out_size(2 * hi if dil == 2 else hi, k, pw.stride, pad)
                wo = ops.conv_out_size(2 * wi if dil == 2 else wi, k, pw.stride, pad)
                pitch = ops.pad_channels(cout)
                kw = {"dil": dil}
                if explicit:
                    kw["out_hw"] = (ho, wo)
                _epilogues(c, ho, wo, pw, pitch, dtype, lambda **e: ops.conv2d(x, pw, pad, pitch, **kw, **e))


def _persist_cases(out: dict, dev) -> None:
    from flairhip import ops
    for dtype in (BF16, F32):
        for h, w in SIZES:
            c = Case(out, f"{_name(dtype)}/{h}x{w}", dev)
            pw = ops.pack_conv_weight(c.weight(64, 64, 3), dtype, 1, 64, **IGEMM)
            x = c.act(h, w, 64, dtype)
            c.put("persistent", torch.tensor([int(ops.conv_is_persistent(dtype, B, h, w, pw))]))
            _epilogues(c, h, w, pw, 64, dtype, lambda **e: ops.conv2d(x, pw, 1, 64, **e))


def _ring_cases(out: dict, dev, dtype) -> None:
    from flairhip import lib as L, ops
    for o in (64, 128):
        for h, w in SIZES:
            c = Case(out, f"{_name(dtype)}/64to{o}/{h}x{w}", dev)
            pw = ops.pack_conv_weight(c.weight(o, 64, 3), dtype, 1, 64)
            assert pw.bco & L.BCO_RING
            x = c.act(h, w, 64, dtype)
            _epilogues(c, h, w, pw, o, dtype, lambda **e: ops.conv2d(x, pw, 1, o, **e))
            st, rows = c.stats(h, w, pw, o)
            c.put("direct", ops.conv3x3_ring(x, pw, o, bias=c.vec(o), relu=True, stats=st))
            c.put("direct_stats", st[:rows * 2 * o])
            if dtype == BF16:
                sc, sh = c.vec(64, 0.5), c.vec(64)
                assert ops.pro_supported(pw, dtype)
                st, rows = c.stats(h, w, pw, o)
                c.put("pro", ops.conv2d_pro(x, pw, o, sc, sh))
                c.put("pro_full", ops.conv2d_pro(x, pw, o, sc, sh, bias=c.vec(o), residual=c.act(h, w, o, dtype),
                                                 relu=True, stats=st))
                c.put("pro_full_stats", st[:rows * 2 * o])
                c.put("pro_direct", ops.conv3x3_ring(x, pw, o, pro_scale=sc, pro_shift=sh))


def _thin_cases(out: dict, dev) -> None:
    from flairhip import lib as L, ops
    for i in (16, 32):
        for o in (16, 32):
            for h, w in SIZES:
                c = Case(out, f"p{i}_r{o}/{h}x{w}", dev)
                wt = c.weight(o, i, 3)
                pw = ops.pack_conv_weight(wt, BF16, 1, i)
                assert pw.bco & L.BCO_THIN and pw.rows == o
                x = c.act(h, w, i, BF16)
                _epilogues(c, h, w, pw, o, BF16, lambda **e: ops.conv2d(x, pw, 1, o, **e))
                lo = c.act(h // 2, w // 2, i, BF16)
                st, rows = c.stats(h, w, pw, o)
                c.put("up", ops.conv2d_upcat(lo, None, pw, o))
                c.put("up_full", ops.conv2d_upcat(lo, None, pw, o, stats=st, bias=c.vec(o), relu=True))
                c.put("up_full_stats", st[:rows * 2 * o])
                sc, sh = c.vec(i, 0.5), c.vec(i)
                for up, src in ((False, x), (True, lo)):
                    assert ops.pro_supported(pw, BF16, up)
                    st, rows = c.stats(h, w, pw, o)
                    tag = "pro_up" if up else "pro"
                    c.put(tag, ops.conv2d_pro(src, pw, o, sc, sh, up=up))
                    c.put(tag + "_full", ops.conv2d_pro(src, pw, o, sc, sh, bias=c.vec(o), relu=True, stats=st, up=up))
                    c.put(tag + "_full_stats", st[:rows * 2 * o])
                # pooled form: the input gradient of the skip-less two-source convolution, 2 x 2 sums
                pwt = ops.pack_conv_weight(wt, BF16, 1, o, transpose=True)
                assert pwt.bco & L.BCO_THIN
                pair = ops.conv2d_dgrad_upcat(c.act(h, w, o, BF16), pwt, i, 0)
                assert pair is not None and pair[1] is None
                c.put("pooled", pair[0])


def _stem_cases(out: dict, dev) -> None:
    from flairhip import lib as L, ops
    c = Case(out, "bf16/5to64/32x48", dev)
    pw = ops.pack_conv_weight(c.weight(64, 5, 7), BF16, 2, 16)
    assert pw.bco & L.BCO_STEM
    x = c.act(32, 48, 5, BF16)
    st, rows = c.stats(16, 24, pw, 64)
    c.put("plain", ops.conv2d(x, pw, 3, 64))
    c.put("relu", ops.conv2d(x, pw, 3, 64, bias=c.vec(64), relu=True))
    c.put("stats", ops.conv2d(x, pw, 3, 64, stats=st))
    c.put("stats_rows", st[:rows * 2 * 64])
    st, rows = c.stats(16, 24, pw, 64)
    c.put("relu_stats", ops.conv2d(x, pw, 3, 64, bias=c.vec(64), relu=True, stats=st))
    c.put("relu_stats_rows", st[:rows * 2 * 64])


def _upcat_cases(out: dict, dev) -> None:
    from flairhip import ops
    for dtype, c1, c2 in [(d, a, b) for d in (BF16, F32) for a, b in ((64, 64), (32, 32), (128, 0))] + [(BF16, 16, 48)]:
        for h, w in SIZES:
            c = Case(out, f"{_name(dtype)}/{c1}+{c2}/{h}x{w}", dev)
            ci, co = c1 + c2, 64
            wt = c.weight(co, ci, 3)
            pw = ops.pack_conv_weight(wt, dtype, 1, ci, **IGEMM)
            lo = c.act(h // 2, w // 2, c1, dtype)
            skip = c.act(h, w, c2, dtype) if c2 else None
            st, rows = c.stats(h, w, pw, co)
            c.put("supported", torch.tensor([int(ops.upcat_supported(c1, c2, dtype))]))
            c.put("fwd", ops.conv2d_upcat(lo, skip, pw, co))
            y = ops.conv2d_upcat(lo, skip, pw, co, stats=st, bias=c.vec(co), relu=True)
            c.put("fwd_full", y)
            if y is not None:
                c.put("fwd_full_stats", st[:rows * 2 * co])
            pwt = ops.pack_conv_weight(wt, dtype, 1, co, transpose=True, **IGEMM)
            pair = ops.conv2d_dgrad_upcat(c.act(h, w, co, dtype), pwt, c1, c2)
            c.put("dlo", None if pair is None else pair[0])
            c.put("dskip", None if pair is None else pair[1])
            if (c1, c2) == (16, 48):  # the refused split: None from both, as the callers expect
                assert y is None and pair is None


def _bnbwd_cases(out: dict, dev) -> None:
    from flairhip import ops
    for dtype in (BF16, F32):
        for name, stride, dil in (("3x3s1", 1, 1), ("3x3dil2", 2, 2)):
            for h, w in SIZES:
                c = Case(out, f"{_name(dtype)}/{name}/{h}x{w}", dev)
                pwt = ops.pack_conv_weight(c.weight(64, 32, 3), dtype, stride, 64, transpose=True, **IGEMM)
                hi, wi = (h // 2, w // 2) if dil == 2 else (h, w)
                dy = c.act(hi, wi, 64, dtype)
                bnx = c.act(h, w, 32, dtype)
                res = c.act(h, w, 32, dtype)
                got, part, rows = ops.conv2d_bnbwd(dy, pwt, 1, 32, bnx, c.vec(32, 0.5), c.vec(32), residual=res, dil=dil)
                assert rows == ops.conv_stat_rows(B, h, w)
                c.put("dy", got)
                c.put("partials", part[:rows * 2 * 32])


# group -> (environment, cases)
GROUPS = {
    "igemm": ({}, _igemm_cases),
    "igemm_one_tile": ({"FFA_CONV_PERSIST": "0"}, lambda out, dev: _igemm_cases(
        out, dev, shapes=[(f"3x3s1_p{i}_r64", 64, i, 3, 1, 1, 1, False, False) for i in (32, 64)])),
    "persist": ({"FFA_CONV_PERSIST_GRID": "8"}, _persist_cases),
    "ring16": ({"FFA_RING_GRID": "8"}, lambda out, dev: _ring_cases(out, dev, BF16)),
    "ring_f32": ({"FFA_RING": "1", "FFA_RING_GRID": "8"}, lambda out, dev: _ring_cases(out, dev, F32)),
    "thin": ({"FFA_THIN_GRID": "2"}, _thin_cases),
    "stem": ({}, _stem_cases),
    "upcat": ({}, _upcat_cases),
    "bnbwd": ({}, _bnbwd_cases),
}


def run_group(group: str, dev) -> dict:
    """{group/key: sha256} of one group; the caller has set the group's environment"""
    out = {}
    GROUPS[group][1](out, dev)
    torch.cuda.synchronize()
    return {f"{group}/{k}": v for k, v in out.items()}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_conv_calls_match_the_recorded_digests(cuda, monkeypatch, group):
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in GROUPS[group][0].items():
        monkeypatch.setenv(name, value)
    got = run_group(group, cuda)
    assert sorted(got) == sorted(k for k in golden if k.split("/")[0] == group)
    wrong = [k for k in sorted(got) if got[k] != golden[k]]
    assert not wrong, wrong


def test_a_statistics_buffer_is_held_to_the_tiles_of_the_call_that_writes_it(cuda, monkeypatch):
    """one float short of rows * 2 * pitch is refused before anything is launched, the exact size runs: for the plain,
    the two-source and the skip-less prologue call, each sized by the route of that very call"""
    from flairhip import ops
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    c = Case({}, "stats_size", cuda)
    h, w = SIZES[0]
    pw = ops.pack_conv_weight(c.weight(64, 128, 3), BF16, 1, 128, **IGEMM)
    thin = ops.pack_conv_weight(c.weight(16, 16, 3), BF16, 1, 16)
    lo, skip, x = c.act(h // 2, w // 2, 64, BF16), c.act(h, w, 64, BF16), c.act(h, w, 128, BF16)
    lo16, sc, sh = c.act(h // 2, w // 2, 16, BF16), c.vec(16, 0.5), c.vec(16)
    calls = [(pw, 64, lambda st: ops.conv2d(x, pw, 1, 64, stats=st)),
             (pw, 64, lambda st: ops.conv2d_upcat(lo, skip, pw, 64, stats=st)),
             (thin, 16, lambda st: ops.conv2d_pro(lo16, thin, 16, sc, sh, stats=st, up=True))]
    for operand, pitch, call in calls:
        need = ops.conv_stat_rows(B, h, w, operand) * 2 * pitch
        with pytest.raises(ValueError, match="statistics buffer too small"):
            call(torch.zeros(need - 1, device=cuda))
        assert call(torch.zeros(need, device=cuda)) is not None
    torch.cuda.synchronize()
