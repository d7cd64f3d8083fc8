"""Test-time augmentation kernels (csrc/tta.hip: ffa_tta_accumulate, ffa_tta_predict_u8, ffa_tta_probabilities) through
their operators.  The oracle is flairhip.augment.tta_mean_probabilities, the float64 definition; the views handed to the
kernels are made with augment.apply_code on the host.

Shapes: the smallest that cross the seams of the 16 x 16 tiles and leave partial tiles (H = W in 40, 64, 33), two
samples, pitches 8 and 24 with K below and at the pitch, bf16 and f32 logits, the whole tile or an asymmetric window.
"""
import numpy as np
import pytest
import torch

from flairhip import augment

pytestmark = pytest.mark.gpu

WINDOW = (3, 5, 17, 30)  # y0, x0, h, w
# K, Cp, n, crop
SHAPES = [(19, 24, 40, None), (19, 24, 40, WINDOW), (3, 8, 64, WINDOW), (3, 8, 33, None), (24, 24, 33, None),
          (24, 24, 64, WINDOW)]
SHAPE_IDS = [f"K{k}cp{cp}n{n}{'win' if c else 'full'}" for k, cp, n, c in SHAPES]
DTYPES = [torch.bfloat16, torch.float32]
DTYPE_IDS = ["bf16", "f32"]
MODES = ("argmax", "class_prob", "argmax_conf")
B = 2


def to_nhwc(z_nchw, dtype, dev, cp):
    """[B,K,n,n] numpy / torch -> NHWC device tensor at pitch cp; garbage in the pad channels must be ignored"""
    z = torch.as_tensor(np.asarray(z_nchw), dtype=torch.float32)
    b, k, h, w = z.shape
    out = torch.full((b, h, w, cp), 7.0, dtype=torch.float32)
    out[..., :k] = z.permute(0, 2, 3, 1)
    return out.to(dtype).to(dev).contiguous()


def crop_of(a, crop):
    if crop is None:
        return a
    y0, x0, h, w = crop
    return a[..., y0:y0 + h, x0:x0 + w]


def window(n, crop):
    return (n, n) if crop is None else crop[2:]


def bf16_values(a):
    """round to bf16-representable float64 values: both logit dtypes then hold the oracle's inputs exactly"""
    return torch.as_tensor(a, dtype=torch.float32).to(torch.bfloat16).double().numpy()


# ---- 1. geometry, exact ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K,cp,n,crop", SHAPES, ids=SHAPE_IDS)
def test_every_code_comes_back_to_the_tile_frame(cuda, K, cp, n, crop):
    """a near-one-hot map (margin 20) whose class at (i, j) of sample b is (7 i + 3 j + 11 b) % K: the view of every
    code, accumulated alone, must give the untransformed class map over the crop -- any frame mix-up fails"""
    from flairhip import ops
    b, i, j = np.meshgrid(np.arange(B), np.arange(n), np.arange(n), indexing="ij")
    cls = (7 * i + 3 * j + 11 * b) % K
    z = np.zeros((B, K, n, n))
    np.put_along_axis(z, cls[:, None], 20.0, axis=1)
    want = torch.as_tensor(crop_of(cls, crop).astype(np.uint8))
    h, w = window(n, crop)
    for dtype in DTYPES:
        acc = ops.tta_buffer(B, K, h, w, cuda, cp=cp)
        for code in range(16):
            view = to_nhwc(augment.apply_code(z, code), dtype, cuda, cp)
            ops.tta_accumulate_(acc, view, K, code, crop=crop, first=True)
            got = ops.tta_predict_u8(acc, "argmax", 1)
            assert got.shape == (B, h, w) and got.dtype == torch.uint8
            assert torch.equal(got.cpu(), want), (dtype, code)


# ---- 2. one identity view is ffa_predict_u8, bit for bit ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("K,cp,n,crop", SHAPES, ids=SHAPE_IDS)
def test_one_identity_view_equals_predict_u8(cuda, dtype, K, cp, n, crop):
    """modes 1 and 2: the same arithmetic, operation for operation (acc / 1.f is exact).  Mode 0: the maximum logit's
    expf(z - m) is exactly 1 and another class reaches 1 only when its logit equals the maximum, so the first maximum
    of the probabilities is the first maximum of the logits."""
    from flairhip import ops
    g = torch.Generator().manual_seed(K * 1000 + n)
    z = torch.randn(B, K, n, n, generator=g) * 3
    y0, x0, h, w = crop if crop is not None else (0, 0, n, n)
    z[0, :, y0, x0] = 1.25                            # all classes tie: lowest index, confidence rint(255 / K)
    z[-1, :, y0 + h // 2, x0 + w // 2] = -40.0
    z[-1, K - 1, y0 + h // 2, x0 + w // 2] = 40.0      # a saturated pixel: confidence 255
    zd = to_nhwc(z, dtype, cuda, cp)
    acc = ops.tta_buffer(B, K, h, w, cuda, cp=cp)
    acc.fill_(float("nan"))  # first=True stores: what the buffer held does not matter
    assert ops.tta_accumulate_(acc, zd, K, 0, crop=crop, first=True) is acc
    for mode in MODES:
        got, want = ops.tta_predict_u8(acc, mode, 1), ops.predict_u8(zd, K, mode, crop)
        assert got.shape == want.shape and got.dtype == torch.uint8
        assert torch.equal(got, want), mode
    both = ops.tta_predict_u8(acc, "argmax_conf", 1).cpu()
    assert both[0, 0, 0, 0] == 0 and both[0, 1, 0, 0] == int(np.rint(255.0 / K))
    assert both[-1, 0, h // 2, w // 2] == K - 1 and both[-1, 1, h // 2, w // 2] == 255
    assert not acc[..., K:].any()  # pad channels hold 0
    prob = ops.tta_probabilities(acc, 1)
    assert prob.shape == (B, K, h, w) and prob.dtype == torch.float32
    assert torch.equal(prob, acc[..., :K].permute(0, 3, 1, 2))


# ---- 3. several views against float64 -------------------------------------------------------------------------------------

def probability_bound(K, V):
    return (K + V + 24) * 2.0 ** -24


@pytest.mark.parametrize("name", ["flips", "d4"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("K,cp,n,crop", SHAPES, ids=SHAPE_IDS)
def test_views_against_float64(cuda, name, dtype, K, cp, n, crop):
    """Logits N(0, 2) rounded to bf16 values, drawn independently per view; every output against
    augment.tta_mean_probabilities.

    Bound on the probabilities, with u = 2^-24 the unit roundoff of f32 and |z - m| < 16:
      * z - m of two bf16 values is exact unless z is below 2^-13 in magnitude; then its error is at most half an ulp
        of a number below 16, 2^-21 = 8 u, and that is also the relative error it causes in exp(z - m);
      * expf: at most 2 u (its documented accuracy is 1 ulp); so each e_k is within 10 u, relative;
      * se: the K - 1 additions add (K - 1) u to the 10 u of the terms; e / se one more: a view's probability is
        within (20 + K) u;
      * the V - 1 additions of the accumulator and the division by V: V u more.
    Every term is positive, so the relative errors carry over to the mean: |p - p64| <= (K + V + 20) u p64, tested
    with (K + V + 24) u for the second-order terms.  That is at most 56 * 2^-24 = 3.4e-6 of p64 <= 1 here, 8.6e-4 of
    a uint8 code.  Hence the rules for the uint8
    outputs: a band may differ from rint(255 p64) only where 255 p64 is within 1e-3 of a half-integer, and then by 1; a
    label may differ only where the float64 top-two gap is below 1e-5.  Each exclusion set may hold at most 1 % of the
    values, which is asserted on the float64 oracle alone, before the GPU result is looked at (the shares are about
    0.2 % and 0.1 % for these inputs).
    """
    from flairhip import ops
    codes = augment.TTA_VIEWS[name]
    V = len(codes)
    g = np.random.default_rng(K * 100 + n + V)
    views = [bf16_values(g.normal(0.0, 2.0, (B, K, n, n))) for _ in codes]
    p64 = crop_of(augment.tta_mean_probabilities(views, codes), crop)
    h, w = window(n, crop)

    # the oracle's own exclusion sets, capped before the GPU result is looked at
    scaled = 255.0 * p64
    band_open = np.abs(scaled - np.floor(scaled) - 0.5) <= 1e-3
    top2 = np.sort(p64, axis=1)[:, -2:]
    label_open = (top2[:, 1] - top2[:, 0]) < 1e-5
    for what, open_ in (("band", band_open), ("label", label_open)):
        print(f"{name} K={K} n={n}: {what} exclusion share {open_.mean():.4%}")
        assert open_.mean() <= 0.01, what

    devs = [to_nhwc(v, dtype, cuda, cp) for v in views]
    acc = ops.tta_buffer(B, K, h, w, cuda, cp=cp)
    for v, (code, view) in enumerate(zip(codes, devs)):
        ops.tta_accumulate_(acc, view, K, code, crop=crop, first=v == 0)
    again = ops.tta_buffer(B, K, h, w, cuda, cp=cp)
    for v, (code, view) in enumerate(zip(codes, devs)):
        ops.tta_accumulate_(again, view, K, code, crop=crop, first=v == 0)
    assert torch.equal(acc, again)  # deterministic: byte-identical accumulators

    prob = ops.tta_probabilities(acc, V).double().cpu().numpy()
    err = (np.abs(prob - p64) / p64).max()
    print(f"{name} K={K} n={n}: max relative probability error {err:.3e} (bound {probability_bound(K, V):.3e})")
    assert err <= probability_bound(K, V)

    want_label = p64.argmax(axis=1)
    want_bands = np.rint(scaled)
    label = ops.tta_predict_u8(acc, "argmax", V).cpu().numpy()
    bands = ops.tta_predict_u8(acc, "class_prob", V).cpu().numpy()
    both = ops.tta_predict_u8(acc, "argmax_conf", V).cpu().numpy()
    assert label.shape == (B, h, w) and bands.shape == (B, K, h, w) and both.shape == (B, 2, h, w)
    assert not ((label != want_label) & ~label_open).any()
    d = bands.astype(np.int64) - want_bands.astype(np.int64)
    assert not (d != 0)[~band_open].any() and np.abs(d).max() <= 1
    assert np.array_equal(both[:, 0], label)
    assert np.array_equal(both[:, 1], bands.max(axis=1))  # bit for bit the largest mode-1 band


# ---- 4. arguments ---------------------------------------------------------------------------------------------------------

def test_arguments_are_checked_on_the_host(cuda, lib):
    """every check happens before a launch: nothing here reaches the device"""
    from flairhip import lib as L
    from flairhip import ops
    K, cp, n = 19, 24, 40
    z = torch.zeros(B, n, n, cp, device=cuda)
    acc = ops.tta_buffer(B, K, n, n, cuda, cp=cp)
    with pytest.raises(ValueError):  # a non-square tile
        ops.tta_accumulate_(ops.tta_buffer(B, K, n, 48, cuda, cp=cp), torch.zeros(B, n, 48, cp, device=cuda), K, 0,
                            first=True)
    for crop in ((0, 0, n + 1, n), (30, 0, 17, 30), (-1, 0, 5, 5), (0, 0, 0, 5)):  # a crop outside the tile
        with pytest.raises(ValueError):
            ops.tta_accumulate_(acc, z, K, 0, crop=crop, first=True)
    with pytest.raises(ValueError):  # the accumulator is not the crop's
        ops.tta_accumulate_(acc, z, K, 0, crop=WINDOW, first=True)
    with pytest.raises(ValueError):  # K > Cp
        ops.tta_accumulate_(acc, z, 25, 0, first=True)
    with pytest.raises(ValueError):
        ops.tta_buffer(B, 25, n, n, cuda, cp=24)
    for code in (16, -1, 1.0, True):
        with pytest.raises(ValueError):
            ops.tta_accumulate_(acc, z, K, code, first=True)
    with pytest.raises(ValueError):  # an unknown mode
        ops.tta_predict_u8(acc, "softmax", 1)
    for views in (0, -1, 1.5):  # views < 1
        with pytest.raises(ValueError):
            ops.tta_predict_u8(acc, "argmax", views)
        with pytest.raises(ValueError):
            ops.tta_probabilities(acc, views)
    with pytest.raises(ValueError):  # an unknown tta name
        augment.tta_views("rot")

    # the library's own checks, behind the operators'
    out = torch.empty(B * K * n * n, dtype=torch.float32, device=cuda)
    s = torch.cuda.current_stream().cuda_stream
    a, zp, op = acc.data_ptr(), z.data_ptr(), out.data_ptr()
    assert lib.ffa_tta_accumulate(L.F32, zp, a, B, n, 48, K, cp, 0, 0, n, n, 0, 1, s) == L.ERR_UNSUPPORTED
    assert b"square" in lib.ffa_last_error()
    for args in ((B, n, n, K, cp, 30, 0, 17, 30, 0, 1),    # crop outside the tile
                 (B, n, n, 25, cp, 0, 0, n, n, 0, 1),      # K > Cp
                 (B, n, n, K, 20, 0, 0, n, n, 0, 1),       # pitch not a multiple of 8
                 (B, n, n, K, cp, 0, 0, n, n, 16, 1)):     # code outside 0..15
        assert lib.ffa_tta_accumulate(L.F32, zp, a, *args, s) == -1, args
    assert lib.ffa_tta_predict_u8(3, a, op, B, K, cp, n, n, 1, s) == -1
    assert lib.ffa_tta_predict_u8(0, a, op, B, K, cp, n, n, 0, s) == -1
    assert lib.ffa_tta_predict_u8(0, a, op, B, 25, cp, n, n, 1, s) == -1
    assert lib.ffa_tta_probabilities(a, op, B, K, cp, n, n, 0, s) == -1
    with pytest.raises(L.FlairHipError):
        L.check(lib.ffa_tta_probabilities(a, None, B, K, cp, n, n, 1, s), "tta_probabilities")
    torch.cuda.synchronize()
