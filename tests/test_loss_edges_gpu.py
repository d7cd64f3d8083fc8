"""The kernels of csrc/resample_loss.hip at the shapes, types and inputs where they can go wrong, held to float64.

nearest x2 upsample + concat (forward, backward), the bilinear resize (forward, backward), the weighted softmax
cross-entropy (ce_weight_sum_kernel, softmax_ce_kernel, softmax_ce_tiled_kernel with and without the per-class sums, the
finalisers), predict_u8's three modes, onehot_to_index, the confusion matrix and scale_inplace.  Every call goes through
flairhip.ops under insitu.Recorder(mode="full", chunk=1): the references and bounds are those of tests/insitu.py
(|o - r| <= ulp_stored(r) + 2^-16 a, f32 sums 2^-16 a, pad channels exactly zero, uint8 bands under the HALF_OPEN /
OPEN_MAX_SHARE rule); this module brings no tolerance of its own.  What it asserts beside the Recorder's verdicts is
exact: labels equal to the first maximum, bytes equal between two runs, a declined output that is None.

softmax_ce runs as the plain kernel (FFA_CE_TILED=0, upstream gradient 1), the tiled kernel (0.37) and the tiled kernel
with the per-class sums (-2.5).  Pixel counts: 1, 63, 255, 256, 257 (a lane, a ragged wave, a ragged tile, a full tile,
two tiles), 4099 (several blocks) and 2 x 363 x 363, the smallest batch of squares above the grid cap of 1024 blocks x
256 threads, where a block walks more than one tile and requests the next tile's pieces while the LDS tile is in use.
K / pitch: 1/8, 5/8, 13/16, 19/24, 19/32, 32/32: in bf16 1, 1, 2, 3, 4, 4 sixteen-byte pieces per pixel, in f32 2, 2, 4,
6, 8, 8; pitch 24 (3 / 6 pieces) declines the sums.

The wide-logit table is the one that exposed a defect: the kernels took the target's term of the loss as
log(exp(z_t - m)), which is -inf once the target's logit lies about 87 below the maximum, so ONE confidently wrong pixel
made the training loss +inf.  They now keep z_t - m (as eval_stats_kernel does)."""
import functools
import time
import zlib
from collections import Counter

import pytest
import torch
import torch.nn.functional as F

from insitu import HALF_OPEN, OPEN_MAX_SHARE, Recorder, first_max

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DTYPES = [BF16, F32]
DT_IDS = ["bf16", "f32"]
BIG = 2 * 363 * 363
NPIX = [1, 63, 255, 256, 257, 4099, BIG]
CLASSES = [(1, 8), (5, 8), (13, 16), (19, 24), (19, 32), (32, 32)]
GARBAGE = (float("nan"), float("inf"), float("-inf"), 1e30)
# upstream gradients of the three softmax_ce runs of a case: (FFA_CE_TILED, want_sums, grad_scale)
RUNS = (("0", False, None), (None, False, 0.37), (None, True, -2.5))

# the ops names each test reaches: _finish holds a test's Recorder to its entry, the last test holds the union to LISTED
CALLS = {
    "softmax_ce": {"softmax_ce"},
    "predict_u8": {"predict_u8"},
    "upsample2x_concat": {"upsample2x_concat_fwd", "upsample2x_concat_bwd"},
    "bilinear": {"bilinear_fwd", "bilinear_bwd"},
    "confusion": {"confusion_matrix_update"},
    "onehot_to_index": {"onehot_to_index"},
    "scale_inplace": {"scale_inplace"},
}
LISTED = {"softmax_ce", "predict_u8", "upsample2x_concat_fwd", "upsample2x_concat_bwd", "bilinear_fwd", "bilinear_bwd",
          "confusion_matrix_update", "onehot_to_index", "scale_inplace"}


def _gen(*parts):
    return torch.Generator().manual_seed(zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF)


def same(a, b):
    """equal type, shape and bytes (NaN payloads and the sign of zero included)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _shape(npix):
    return (2, 363, 363) if npix == BIG else (1, 1, npix)


def _finish(rec, group, expected_calls, label, t0):
    """the Recorder saw exactly the calls the test made, every one had a reference, and none failed"""
    torch.cuda.synchronize()
    print(f"\n[{label}] {len(rec.calls)} checked calls\n{rec.table()}\nwall time {time.perf_counter() - t0:.2f} s")
    fails = rec.failures()
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    got = Counter(c["op"] for c in rec.calls)
    assert got == Counter(expected_calls), f"calls made {dict(Counter(expected_calls))}, calls checked {dict(got)}"
    assert set(got) == CALLS[group], f"{group}: reached {sorted(got)}, the table says {sorted(CALLS[group])}"
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])


# --------------------------------------------------------------------------------------------------
# softmax_ce: inputs

def class_weights(K, dev):
    """0.5 .. 2.0 over the classes, class 2 with weight zero (K >= 5)"""
    w = torch.linspace(0.5, 2.0, K, dtype=F32) if K > 1 else torch.tensor([0.75])
    if K >= 5:
        w[2] = 0.0
    return w.to(dev)


def _targets(g, npix, K, cp):
    """class K - 1 never occurs (K > 1); about 3 % are 255, about 2 % the index of a pad channel; pixel 0 counts"""
    t = torch.randint(0, max(K - 1, 1), (npix,), generator=g).to(torch.uint8)
    r = torch.rand(npix, generator=g)
    t[r < 0.03] = 255
    if cp > K:
        pad = torch.randint(K, cp, (npix,), generator=g).to(torch.uint8)
        t = torch.where((r >= 0.03) & (r < 0.05), pad, t)
    t[0] = 0
    return t


def _plant_ties(g, z, K, dtype, share=50):
    """two distinct classes share the pixel's maximum, as stored, on npix / share pixels (at least one)"""
    npix = z.shape[0]
    n_tie = max(1, npix // share)
    rows = torch.randperm(npix, generator=g)[:n_tie]
    a = torch.randint(0, K, (n_tie,), generator=g)
    b = (a + 1 + torch.randint(0, K - 1, (n_tie,), generator=g)) % K
    top = (z[rows, :K].float().max(-1).values + 1.0).to(dtype)
    z[rows, a] = top
    z[rows, b] = top
    return z


@functools.lru_cache(maxsize=None)
def ce_case(npix, K, cp, dtype):
    """logits (3 * randn as stored, pad channels zero, planted ties), targets, weights and the float64 label, on the
    GPU, built once and shared: nobody writes to them"""
    dev = torch.device("cuda:0")
    g = _gen("ce", npix, K, cp, str(dtype))
    z = torch.zeros(npix, cp)
    z[:, :K] = 3.0 * torch.randn(npix, K, generator=g)
    z = z.to(dtype)
    if K > 1:
        z = _plant_ties(g, z, K, dtype)
    t = _targets(g, npix, K, cp)
    shape = _shape(npix)
    z, t = z.reshape(*shape, cp).to(dev), t.reshape(shape).to(dev)
    z64 = z[..., :K].to(F64)
    ref = {"pred": first_max(z64).to(torch.uint8),
           "ties": int(((z64 == z64.max(-1, keepdim=True).values).sum(-1) > 1).sum())}
    return z, t, class_weights(K, dev), ref


def ce_runs(monkeypatch, ops, z, t, w, K, ref_pred=None, scales=None):
    """the three runs of a case -> [(loss, wsum, dlogits, pred, sums or None)]; the label is held to the first maximum
    and a pitch of 3 / 6 pieces must decline the sums, every other pitch provide them"""
    cp = z.shape[-1]
    pieces = cp * z.element_size() // 16
    outs = []
    for i, (tiled, want_sums, gs) in enumerate(RUNS):
        if scales is not None:
            gs = scales[i]
        if tiled is None:
            monkeypatch.delenv("FFA_CE_TILED", raising=False)
        else:
            monkeypatch.setenv("FFA_CE_TILED", tiled)
        scale = None if gs is None else torch.tensor([gs], dtype=F32, device=z.device)
        out = ops.softmax_ce(z, t, w, K, grad_scale=scale, want_grad=True, want_pred=True, want_sums=want_sums)
        assert len(out) == (5 if want_sums else 4)
        if want_sums:
            if 256 % pieces:
                assert out[4] is None, f"pitch {cp}: {pieces} pieces per pixel cannot give the sums in the same pass"
            else:
                assert out[4] is not None and out[4].shape == (cp,) and out[4].dtype == F32
        if ref_pred is not None:
            assert torch.equal(out[3], ref_pred), "pred is not the first maximum"
        outs.append(tuple(out) + (None,) * (5 - len(out)))
    monkeypatch.delenv("FFA_CE_TILED", raising=False)
    return outs


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", CLASSES)
@pytest.mark.parametrize("npix", NPIX)
def test_softmax_ce_against_float64(cuda, monkeypatch, npix, K, cp, dtype):
    from flairhip import ops
    t0 = time.perf_counter()
    z, t, w, ref = ce_case(npix, K, cp, dtype)
    if K > 1:
        assert ref["ties"] >= 1  # the planted ties are there
        assert not bool((t == K - 1).any())  # and the absent class is absent
    with Recorder(mode="full", chunk=1) as rec:
        outs = ce_runs(monkeypatch, ops, z, t, w, K, ref["pred"])
        assert same(outs[0][0], outs[1][0]) and same(outs[0][1], outs[1][1])  # plain and tiled: the same loss bytes
        _finish(rec, "softmax_ce", ["softmax_ce"] * 3, f"softmax_ce {npix} px K {K}/{cp} {dtype}", t0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", [(5, 8), (19, 32)])
@pytest.mark.parametrize("npix", [255, 4099])
def test_softmax_ce_targets_at_an_odd_address(cuda, monkeypatch, npix, K, cp, dtype):
    """a contiguous slice starting one byte into a buffer: ce_weight_sum_kernel takes its byte loop for every target.
    Same bounds as the aligned run; no bit equality of wsum / dlogits with it, the summation order differs."""
    from flairhip import ops
    t0 = time.perf_counter()
    z, t, w, ref = ce_case(npix, K, cp, dtype)
    buf = torch.full((t.numel() + 1,), 7, dtype=torch.uint8, device=cuda)
    buf[1:] = t.reshape(-1)
    off = buf[1:].reshape(t.shape)
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    with Recorder(mode="full", chunk=1) as rec:
        ce_runs(monkeypatch, ops, z, off, w, K, ref["pred"])
        _finish(rec, "softmax_ce", ["softmax_ce"] * 3, f"softmax_ce odd target address {npix} px K {K}/{cp} {dtype}", t0)
    assert bool((buf[0] == 7).item())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", [(1, 8), (5, 8), (13, 16), (19, 24), (19, 32)])
def test_softmax_ce_ignores_garbage_in_the_pad_channels(cuda, monkeypatch, K, cp, dtype):
    """one input set with NaN, +inf, -inf and 1e30 in the logits' pad channels and with zeros there: every output byte
    for byte the same, the gradient's pad channels exactly zero"""
    from flairhip import ops
    t0 = time.perf_counter()
    z, t, w, ref = ce_case(4099, K, cp, dtype)
    dirty = z.clone()
    fill = torch.tensor(GARBAGE, dtype=F32, device=cuda).to(dtype)
    idx = torch.arange(z[..., K:].numel(), device=cuda).reshape(z[..., K:].shape) % len(GARBAGE)
    dirty[..., K:] = fill[idx]
    assert bool(dirty[..., K:].isnan().any()) and bool(dirty[..., K:].isinf().any())
    with Recorder(mode="full", chunk=1) as rec:
        clean_outs = ce_runs(monkeypatch, ops, z, t, w, K, ref["pred"])
        dirty_outs = ce_runs(monkeypatch, ops, dirty, t, w, K, ref["pred"])
        for a, b in zip(clean_outs, dirty_outs):
            for x, y in zip(a, b):
                assert (x is None and y is None) or same(x, y)
            assert not bool((b[2][..., K:] != 0).any())
        _finish(rec, "softmax_ce", ["softmax_ce"] * 6, f"softmax_ce pad garbage K {K}/{cp} {dtype}", t0)


# ---- wide logits ---------------------------------------------------------------------------------

SPREADS = (0, 80, 88, 100, 176, 1000)
# The upstream gradient of a spread, chosen so that no reference gradient value falls into the denormal range of f32 /
# bf16, (2^-150, 2^-126), where a kernel may flush: the class at -S/2 has the gradient f * exp(-S) / se with
# f = grad_scale * w / wsum (w in [0.5, 2], wsum about 3000 .. 5000) and se in [1, K].  At grad_scale 1 that is
# 5e-39 .. 1e-38 for S = 80 and about 1e-42 for S = 88, both inside the range: 1024 (a loss scale) lifts S = 80 to
# 1e-37 and above, 2^-20 puts S = 88 at 4e-48 and below.  S >= 100: below 2^-150 at grad_scale 1.
WIDE_SCALE = {0: 1.0, 80: 1024.0, 88: 2.0 ** -20, 100: 1.0, 176: 1.0, 1000: 1.0}
WIDE_NPIX = 4099


@functools.lru_cache(maxsize=None)
def wide_case(S, variant, K, cp, dtype, offset=0.0, device="cuda:0"):
    """4099 pixels of 3 * randn + 6; on about 5 % the maximum class sits at +S/2, the other classes within 10 below it
    (S = 0: all classes equal) and one class at -S/2: in variant "target" that class is the target on one half of the
    planted pixels (confidently wrong) and the maximum is the target on the other half (confidently right); in
    variant "other" the class at -S/2 is never the target.  offset: added to all classes of a planted pixel."""
    dev = torch.device(device)
    g = _gen("wide", S, variant, K, cp, str(dtype), offset)
    npix = WIDE_NPIX
    z = torch.zeros(npix, cp)
    z[:, :K] = 3.0 * torch.randn(npix, K, generator=g) + 6.0
    t = _targets(g, npix, K, cp)
    n = npix // 20
    rows = 1 + torch.randperm(npix - 1, generator=g)[:n]  # (pixel 0 keeps its plain target)
    a = torch.randint(0, K - 1, (n,), generator=g)          # the maximum; class K - 1 stays absent as a target
    b = (a + 1 + torch.randint(0, K - 2, (n,), generator=g)) % (K - 1)   # the class at -S/2, != a
    c = (b + 1 + torch.randint(0, K - 2, (n,), generator=g)) % (K - 1)   # a target that is not b
    planted = S / 2.0 - 10.0 * torch.rand(n, K, generator=g) if S else torch.zeros(n, K)
    ar = torch.arange(n)
    planted[ar, a] = S / 2.0
    planted[ar, b] = -S / 2.0
    z[rows, :K] = planted + offset
    wrong = ar % 2 == 0
    t[rows] = (torch.where(wrong, b, a) if variant == "target" else torch.where(wrong, c, a)).to(torch.uint8)
    z = z.to(dtype)
    return (z.reshape(1, 1, npix, cp).to(dev), t.reshape(1, 1, npix).to(dev), class_weights(K, dev),
            rows.to(dev), wrong.to(dev))


def wide_preconditions(z, t, w, K, scales):
    """the two conditions that keep the Checker's bounds meaningful for f32 arithmetic, on the float64 reference alone:
    (a) every pixel of weight != 0 has |lse| + |z_t| >= 1, so that REL * (|lse| + |z_t|) covers the absolute f32 error
    of log(se), se in [1, 32]; (b) no reference gradient value lies in (2^-150, 2^-126).  -> (lse - z_t, weight)"""
    z64 = z[..., :K].to(F64).reshape(-1, K)
    tl = t.reshape(-1).long()
    tc = tl.clamp(max=K - 1)
    wp = w.to(F64)[tc] * (tl < K)
    lse = torch.logsumexp(z64, -1)
    zt = z64.gather(1, tc[:, None])[:, 0]
    counted = wp != 0
    assert bool((lse.abs() + zt.abs())[counted].min() >= 1.0), "(a): a counted pixel with |lse| + |z_t| < 1"
    grad = (wp / wp.sum())[:, None] * (torch.softmax(z64, -1) - F.one_hot(tc, K).to(F64))
    for gs in scales:
        mag = (grad * (1.0 if gs is None else gs)).abs()
        inside = (mag > 2.0 ** -150) & (mag < 2.0 ** -126)
        assert not bool(inside.any()), f"(b): {int(inside.sum())} reference gradient values in the denormal range " \
                                       f"at grad_scale {gs}: {mag[inside][:4].tolist()}"
    return lse - zt, wp


def wide_run(cuda, monkeypatch, S, variant, K, cp, dtype, offset, scales, label):
    from flairhip import ops
    t0 = time.perf_counter()
    z, t, w, rows, wrong = wide_case(S, variant, K, cp, dtype, offset)
    nll, wp = wide_preconditions(z, t, w, K, scales)
    if variant == "target" and S:  # the input is what it claims: counted pixels whose target lies S below the maximum
        hard = nll[rows[wrong]][wp[rows[wrong]] != 0]
        spread = S if not offset else 0.9 * S  # (an offset rounds the planted values of a bf16 tensor)
        assert hard.numel() >= 20 and bool((hard >= spread).all())
    ref_pred = first_max(z[..., :K].to(F64)).to(torch.uint8)
    with Recorder(mode="full", chunk=1) as rec:
        outs = ce_runs(monkeypatch, ops, z, t, w, K, ref_pred, scales=scales)
        print("loss", [o[0].item() for o in outs])
        _finish(rec, "softmax_ce", ["softmax_ce"] * 3, label, t0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", [(5, 8), (19, 32)])
@pytest.mark.parametrize("variant", ["target", "other"])
@pytest.mark.parametrize("S", SPREADS)
def test_softmax_ce_wide_logits(cuda, monkeypatch, S, variant, K, cp, dtype):
    """a target far below the maximum costs lse - z_t, about S: a finite loss, and the gradient of that pixel is the
    one-hot difference (-f on the target, +f on the maximum)"""
    gs = WIDE_SCALE[S]
    wide_run(cuda, monkeypatch, S, variant, K, cp, dtype, 0.0, (gs, gs, -gs),
             f"softmax_ce wide logits S {S} {variant} K {K}/{cp} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", [(5, 8), (19, 32)])
def test_softmax_ce_wide_logits_with_a_common_offset(cuda, monkeypatch, K, cp, dtype):
    """S = 100 on top of +3e4 (f32) / +3e3 (bf16, where the stored values are multiples of 16) on all classes of a pixel"""
    offset = 3e4 if dtype == F32 else 3e3
    wide_run(cuda, monkeypatch, 100, "target", K, cp, dtype, offset, (1.0, 1.0, -1.0),
             f"softmax_ce wide logits S 100 + {offset} K {K}/{cp} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_softmax_ce_weight_sum_of_zero(cuda, monkeypatch, dtype):
    """257 pixels, all of a class of weight zero: what the library does, against F.cross_entropy in float64 on the CPU
    -- wsum exactly 0 and a NaN loss (0 / 0, as in torch), the label still right, the gradient's pad channels zero.
    Nothing else is asserted about the gradient.  (Checker.softmax_ce takes a weight sum of zero the same way.)"""
    from flairhip import ops
    t0 = time.perf_counter()
    K, cp, npix = 19, 32, 257
    z, _, w, ref = ce_case(npix, K, cp, dtype)
    t = torch.full((1, 1, npix), 2, dtype=torch.uint8, device=cuda)
    assert w[2].item() == 0.0
    torch_loss = F.cross_entropy(z[..., :K].reshape(npix, K).to(F64).cpu(), t.reshape(-1).long().cpu(), weight=w.to(F64).cpu())
    assert bool(torch_loss.isnan())
    with Recorder(mode="full", chunk=1) as rec:
        outs = ce_runs(monkeypatch, ops, z, t, w, K, ref["pred"])
        for loss, wsum, dlogits, pred, _ in outs:
            assert wsum.item() == 0.0 and bool(loss.isnan().all())
            assert not bool((dlogits[..., K:] != 0).any())
        _finish(rec, "softmax_ce", ["softmax_ce"] * 3, f"softmax_ce weight sum 0 {dtype}", t0)


# --------------------------------------------------------------------------------------------------
# predict_u8

PB = 3
TILES = [(5, 7), (17, 33)]
PRED_CLASSES = [(1, 8), (5, 8), (19, 24), (19, 32), (32, 32)]


def crops(H, W):
    return [(0, 0, 1, 1), (H - 1, W - 1, 1, 1), (0, 0, H, W), (1, 2, H - 3, W - 4)]


def predict_logits(kind, H, W, K, cp, dtype, dev):
    """"plain": 4 * randn with two-way ties at the maximum on 2 % of the pixels; "wide<S>": one class at +S/2 and the
    others at -S/2 and up to 5 below, so that every band is exactly 0 or 255"""
    g = _gen("predict", kind, H, W, K, cp, str(dtype))
    npix = PB * H * W
    z = torch.zeros(npix, cp)
    if kind == "plain":
        z[:, :K] = 4.0 * torch.randn(npix, K, generator=g)
        z = z.to(dtype)
        if K > 1:
            z = _plant_ties(g, z, K, dtype)
        # a one-pixel crop has 3 K bands, of which not one may be left open (OPEN_MAX_SHARE): the corner pixels are
        # drawn again until the float64 bands of the stored values keep 10 * HALF_OPEN away from every half-integer
        for b in range(PB):
            for pix in (b * H * W, (b + 1) * H * W - 1):
                for _ in range(1000):
                    p = 255.0 * torch.softmax(z[pix, :K].to(F64), -1)
                    if bool(((p - p.floor() - 0.5).abs() > 10 * HALF_OPEN).all()):
                        break
                    z[pix, :K] = (4.0 * torch.randn(K, generator=g)).to(dtype)
    else:
        S = float(kind[4:])
        z[:, :K] = -S / 2.0 - 5.0 * torch.rand(npix, K, generator=g)
        z[torch.arange(npix), torch.randint(0, K, (npix,), generator=g)] = S / 2.0
        z = z.to(dtype)
    return z.reshape(PB, H, W, cp).to(dev)


def open_share(z, K, crop, top_only):
    """share of the float64 bands (of the confidence: their maximum) within HALF_OPEN of a half-integer"""
    y0, x0, h, w = crop
    p = 255.0 * torch.softmax(z[:, y0:y0 + h, x0:x0 + w, :K].to(F64), -1)
    if top_only:
        p = p.max(-1).values
    return float(((p - p.floor() - 0.5).abs() <= HALF_OPEN).double().mean())


def predict_calls(ops, z, K, garbage_twin=None):
    """the three modes over the four crops; argmax_conf must be the other two outputs byte for byte -> calls made"""
    H, W = z.shape[1:3]
    made = 0
    for crop in crops(H, W):
        for top_only in (False, True):  # decided on the reference, before the call
            assert open_share(z, K, crop, top_only) <= OPEN_MAX_SHARE
        lab = ops.predict_u8(z, K, "argmax", crop)
        bands = ops.predict_u8(z, K, "class_prob", crop)
        both = ops.predict_u8(z, K, "argmax_conf", crop)
        made += 3
        assert lab.shape == (PB, crop[2], crop[3]) and bands.shape == (PB, K, crop[2], crop[3])
        assert same(both[:, 0], lab) and same(both[:, 1], bands.max(1).values)
        if garbage_twin is not None:
            for mode, clean in (("argmax", lab), ("class_prob", bands), ("argmax_conf", both)):
                assert same(ops.predict_u8(garbage_twin, K, mode, crop), clean)
            made += 3
    return made


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("K,cp", PRED_CLASSES)
@pytest.mark.parametrize("H,W", TILES)
def test_predict_u8_against_float64(cuda, H, W, K, cp, dtype):
    """labels exactly the first maximum (planted ties included), bands and confidence under the half-integer rule; the
    same logits with NaN, +inf, -inf and 1e30 in the pad channels give the same bytes"""
    from flairhip import ops
    t0 = time.perf_counter()
    z = predict_logits("plain", H, W, K, cp, dtype, cuda)
    twin = None
    if cp > K:
        twin = z.clone()
        fill = torch.tensor(GARBAGE, dtype=F32, device=cuda).to(dtype)
        twin[..., K:] = fill[torch.arange(twin[..., K:].numel(), device=cuda).reshape(twin[..., K:].shape) % len(GARBAGE)]
    with Recorder(mode="full", chunk=1) as rec:
        made = predict_calls(ops, z, K, twin)
        if K > 1:
            assert rec.ties["predict_u8"] >= 1  # labels were checked at an exact tie
        _finish(rec, "predict_u8", ["predict_u8"] * made, f"predict_u8 {H}x{W} K {K}/{cp} {dtype}", t0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("S", [100, 1000])
def test_predict_u8_wide_logits_give_bands_of_0_and_255(cuda, S, dtype):
    from flairhip import ops
    t0 = time.perf_counter()
    H, W, K, cp = 17, 33, 19, 32
    z = predict_logits(f"wide{S}", H, W, K, cp, dtype, cuda)
    with Recorder(mode="full", chunk=1) as rec:
        made = predict_calls(ops, z, K)
        bands = ops.predict_u8(z, K, "class_prob")
        want = F.one_hot(first_max(z[..., :K].to(F64)), K).permute(0, 3, 1, 2).to(torch.uint8) * 255
        assert torch.equal(bands, want)
        _finish(rec, "predict_u8", ["predict_u8"] * (made + 1), f"predict_u8 wide logits S {S} {dtype}", t0)


# --------------------------------------------------------------------------------------------------
# nearest x2 + concat, bilinear

RB = 3
LO_SIZES = [(1, 1), (3, 5), (9, 17)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C1,C2", [(8, 0), (8, 8), (24, 40), (64, 64)])
def test_upsample2x_concat_forward_and_backward(cuda, C1, C2, dtype):
    """the forward is a copy (exact); dlo, the sum of the four children, is held to ulp_stored(r) + REL * sum |child|,
    dskip to the bytes of dcat's channel slice, as a copy and as a view"""
    from flairhip import ops
    t0 = time.perf_counter()
    made = []
    with Recorder(mode="full", chunk=1) as rec:
        for Hl, Wl in LO_SIZES:
            g = _gen("up2", C1, C2, Hl, Wl, str(dtype))
            lo = torch.randn(RB, Hl, Wl, C1, generator=g).to(dtype).to(cuda)
            skip = torch.randn(RB, 2 * Hl, 2 * Wl, C2, generator=g).to(dtype).to(cuda) if C2 else None
            out = ops.upsample2x_concat_fwd(lo, skip)
            assert out.shape == (RB, 2 * Hl, 2 * Wl, C1 + C2)
            dcat = torch.randn(RB, 2 * Hl, 2 * Wl, C1 + C2, generator=g).to(dtype).to(cuda)
            dlo, dskip = ops.upsample2x_concat_bwd(dcat, C1)
            dlo_v, dskip_v = ops.upsample2x_concat_bwd(dcat, C1, skip_as_view=True)
            made += ["upsample2x_concat_fwd", "upsample2x_concat_bwd", "upsample2x_concat_bwd"]
            assert same(dlo, dlo_v)
            if C2:
                assert dskip.is_contiguous() and dskip_v.data_ptr() == dcat[..., C1:].data_ptr() and same(dskip, dskip_v)
            else:
                assert dskip is None and dskip_v is None
        _finish(rec, "upsample2x_concat", made, f"upsample2x_concat {C1}+{C2} {dtype}", t0)


# what tests/test_kernels_gpu.py::test_bilinear lacks: B = 3, 8 and 24 channels, N -> 1 and 1 -> N in one dimension only,
# and the ratio 64 -> 3 in both dimensions
RESIZES = [(8, (7, 1), (1, 9)), (24, (7, 1), (1, 9)), (8, (1, 5), (6, 1)), (24, (1, 5), (6, 1)), (8, (64, 64), (3, 3))]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("C,src,dst", RESIZES, ids=[f"{c}ch_{s[0]}x{s[1]}-{d[0]}x{d[1]}" for c, s, d in RESIZES])
def test_bilinear_forward_and_backward(cuda, C, src, dst, dtype):
    from flairhip import ops
    t0 = time.perf_counter()
    g = _gen("bilinear", C, src, dst, str(dtype))
    x = torch.randn(RB, *src, C, generator=g).to(dtype).to(cuda)
    dy = torch.randn(RB, *dst, C, generator=g).to(dtype).to(cuda)
    with Recorder(mode="full", chunk=1) as rec:
        y = ops.bilinear_fwd(x, dst)
        dx = ops.bilinear_bwd(dy, src)
        assert y.shape == (RB, *dst, C) and dx.shape == (RB, *src, C)
        _finish(rec, "bilinear", ["bilinear_fwd", "bilinear_bwd"], f"bilinear {src} -> {dst} C {C} {dtype}", t0)


# --------------------------------------------------------------------------------------------------
# confusion matrix, onehot_to_index, scale_inplace

@functools.lru_cache(maxsize=None)
def label_pair(n, K):
    """(pred, target) uint8 on the GPU, each one byte into its buffer and at its start: values below K, some in
    [K, K + 3] and some 255"""
    dev = torch.device("cuda:0")
    g = _gen("confusion", n, K)

    def labels():
        v = torch.randint(0, K, (n,), generator=g)
        r = torch.rand(n, generator=g)
        v = torch.where(r < 0.04, torch.randint(K, K + 4, (n,), generator=g), v)
        v = torch.where(r > 0.97, torch.full_like(v, 255), v).to(torch.uint8)
        buf = torch.zeros(n + 1, dtype=torch.uint8)
        buf[1:] = v
        return v.to(dev), buf.to(dev)[1:]

    (p, p_off), (t, t_off) = labels(), labels()
    if n >= 15:
        assert bool(((p >= K) | (t >= K)).any())
    assert p_off.data_ptr() % 16 == 1 and t_off.data_ptr() % 16 == 1 and p_off.is_contiguous()
    return p, p_off, t, t_off


@pytest.mark.parametrize("K", [1, 13, 32])
@pytest.mark.parametrize("n", [1, 15, 17, 4099, BIG])
def test_confusion_matrix_update(cuda, n, K):
    """aligned operands (16 labels per pair of loads and the ragged tail) and either one a byte off (the byte loop),
    from a non-zero matrix; a second call accumulates exactly; labels >= K contribute nothing"""
    from flairhip import ops
    t0 = time.perf_counter()
    p, p_off, t, t_off = label_pair(n, K)
    shape = _shape(n)
    start = (torch.arange(K * K, dtype=torch.int64, device=cuda).reshape(K, K) * 3 + 1)
    with Recorder(mode="full", chunk=1) as rec:
        results = []
        for pp, tt in ((p, t), (p_off, t), (p, t_off), (p_off, t_off)):
            cm = start.clone()
            ops.confusion_matrix_update(cm, pp.reshape(shape), tt.reshape(shape))
            once = cm.clone()
            ops.confusion_matrix_update(cm, pp.reshape(shape), tt.reshape(shape))
            assert torch.equal(cm - once, once - start)
            results.append(once)
        assert all(torch.equal(results[0], r) for r in results[1:])
        valid = (p < K) & (t < K)
        assert int((results[0] - start).sum()) == int(valid.sum())
        _finish(rec, "confusion", ["confusion_matrix_update"] * 8, f"confusion n {n} K {K}", t0)


@pytest.mark.parametrize("K", [1, 19, 255])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (3, 33, 47)])
def test_onehot_to_index(cuda, B, H, W, K):
    """a true one-hot map, and a map of few distinct values with ties everywhere: the first maximum"""
    from flairhip import ops
    t0 = time.perf_counter()
    g = _gen("onehot", B, H, W, K)
    idx = torch.randint(0, K, (B, H, W), generator=g)
    onehot = F.one_hot(idx, K).permute(0, 3, 1, 2).float().contiguous().to(cuda)
    ties = torch.randint(-1, 3, (B, K, H, W), generator=g).float().to(cuda)
    with Recorder(mode="full", chunk=1) as rec:
        assert torch.equal(ops.onehot_to_index(onehot).cpu().long(), idx)
        got = ops.onehot_to_index(ties)
        assert got.dtype == torch.uint8 and torch.equal(got.long(), first_max(ties.permute(0, 2, 3, 1).to(F64)))
        _finish(rec, "onehot_to_index", ["onehot_to_index"] * 2, f"onehot_to_index {B}x{H}x{W} K {K}", t0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [8, 8 * 4099])
def test_scale_inplace(cuda, n, dtype):
    from flairhip import ops
    t0 = time.perf_counter()
    x0 = torch.randn(n, generator=_gen("scale", n, str(dtype))).to(dtype).to(cuda)
    with Recorder(mode="full", chunk=1) as rec:
        for s in (1.0, 0.25, -3.0):
            x = x0.clone()
            out = ops.scale_inplace(x, torch.tensor([s], dtype=F32, device=cuda))
            assert out.data_ptr() == x.data_ptr()
            if s == 1.0:
                assert same(x, x0)  # the bytes are untouched
        _finish(rec, "scale_inplace", ["scale_inplace"] * 3, f"scale_inplace {n} {dtype}", t0)


def test_the_ops_this_module_reaches_are_the_listed_ones():
    """every test holds its Recorder to its entry of CALLS (_finish); the union of the entries is the listed set, and
    each name is a function of flairhip.ops with an adapter in the Recorder: a rename cannot drop a case silently"""
    import inspect
    from flairhip import ops
    reached = set().union(*CALLS.values())
    assert reached == LISTED, f"not reached: {sorted(LISTED - reached)}; not listed: {sorted(reached - LISTED)}"
    for name in sorted(LISTED):
        assert inspect.isfunction(getattr(ops, name, None)), f"flairhip.ops has no function {name}"
        assert callable(getattr(Recorder, "_op_" + name, None)), f"the Recorder has no reference for {name}"
