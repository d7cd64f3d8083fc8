"""ffa_predict_thresholded_u8 and ffa_tta_predict_thresholded_u8 (csrc/calibration.hip): labels and confidence under
per-class thresholds.

Oracle, on the CPU: the passing set comes from the bytes the existing ops.predict_u8(..., "class_prob") writes for the
same logits (class k passes where its byte is >= thr[k]); the label is the first maximum of the float32 logits over the
passing set (a bf16 widens exactly), the fallback where the set is empty; the confidence is the class_prob byte of the
chosen class, 0 where nothing passed.  Exact equality of both planes.  The TTA entry is held to the same rule on
ops.tta_probabilities with the bytes of ops.tta_predict_u8 'class_prob'.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
MAIN_CROP = (3, 5, 31, 45)  # y0, x0, h, w: a margin crop of 2 x 40 x 56


def rule(score, q, thr, fallback):
    """score: float32 [B, K, h, w] (the ordering), q: uint8 [B, K, h, w] (the class_prob bytes) -> label, confidence"""
    ok = q >= np.asarray(thr, dtype=np.uint8)[None, :, None, None]
    some = ok.any(1)
    best = np.where(ok, score, -np.inf).argmax(1)  # numpy's argmax is the first maximum
    label = np.where(some, best, fallback).astype(np.uint8)
    conf = np.where(some, np.take_along_axis(q, best[:, None], 1)[:, 0], 0).astype(np.uint8)
    return label, conf


def cropped(z, K, crop):
    y0, x0, h, w = crop
    return z[:, y0:y0 + h, x0:x0 + w, :K].float().cpu().numpy().transpose(0, 3, 1, 2)


def logits(shape, K, cp, dtype, scale, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W = shape
    return (scale * torch.randn(B, H, W, cp, generator=g)).to(dtype).cuda()


def run_both(z, K, thr, fallback, crop):
    """the two modes of the entry under test, against the oracle; -> (label, confidence, argmax of the plain entry)"""
    from flairhip import ops
    thr_dev = torch.tensor(thr, dtype=torch.uint8, device=z.device)
    q = ops.predict_u8(z, K, "class_prob", crop=crop).cpu().numpy()
    want_label, want_conf = rule(cropped(z, K, crop), q, thr, fallback)
    got0 = ops.predict_thresholded_u8(z, K, "argmax", thr_dev, fallback, crop=crop)
    got2 = ops.predict_thresholded_u8(z, K, "argmax_conf", thr_dev, fallback, crop=crop)
    B, _, h, w = q.shape
    assert got0.dtype == torch.uint8 and tuple(got0.shape) == (B, h, w)
    assert got2.dtype == torch.uint8 and tuple(got2.shape) == (B, 2, h, w)
    assert np.array_equal(got0.cpu().numpy(), want_label)
    assert np.array_equal(got2[:, 0].cpu().numpy(), want_label)
    assert np.array_equal(got2[:, 1].cpu().numpy(), want_conf)
    return want_label, want_conf, ops.predict_u8(z, K, "argmax", crop=crop).cpu().numpy()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("K,cp,shape,crop", [(19, 32, (2, 40, 56), MAIN_CROP), (19, 24, (1, 9, 300), (0, 0, 9, 300)),
                                             (2, 8, (1, 5, 7), (1, 1, 3, 5)), (1, 8, (1, 4, 4), (0, 0, 4, 4)),
                                             (32, 32, (3, 17, 33), (2, 0, 15, 33))])
def test_zero_thresholds_give_the_plain_outputs_byte_for_byte(cuda, K, cp, shape, crop, dtype):
    from flairhip import ops
    z = logits(shape, K, cp, dtype, 2.0, K + cp)
    zero = torch.zeros(K, dtype=torch.uint8, device=cuda)
    for fallback in (0, 255):  # unused
        assert torch.equal(ops.predict_thresholded_u8(z, K, "argmax", zero, fallback, crop=crop),
                           ops.predict_u8(z, K, "argmax", crop=crop))
        assert torch.equal(ops.predict_thresholded_u8(z, K, "argmax_conf", zero, fallback, crop=crop),
                           ops.predict_u8(z, K, "argmax_conf", crop=crop))


@pytest.mark.parametrize("fallback", [0, 18, 255])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_main_case_covers_kept_runner_up_and_fallback(cuda, dtype, fallback):
    from flairhip import ops
    K, cp = 19, 32
    # N(0, 2^2) logits; 160 on the even classes, 40 on the odd ones: a rejected even winner leaves the pixel to an odd
    # runner-up above 40 or, without one, to the fallback (tuned in numpy: about 56 % / 17 % / 27 %)
    thr = [160 if k % 2 == 0 else 40 for k in range(K)]
    z = logits((2, 40, 56), K, cp, dtype, 2.0, 3)
    label, conf, plain = run_both(z, K, thr, fallback, MAIN_CROP)
    q = ops.predict_u8(z, K, "class_prob", crop=MAIN_CROP).cpu().numpy()
    nothing = ~(q >= np.asarray(thr, dtype=np.uint8)[None, :, None, None]).any(1)
    kept, runner_up = ~nothing & (label == plain), ~nothing & (label != plain)
    shares = [float(m.mean()) for m in (kept, runner_up, nothing)]
    print(f"kept / runner-up / fallback: {shares[0]:.3f} / {shares[1]:.3f} / {shares[2]:.3f}")
    assert min(shares) >= 0.05, shares
    assert (label[nothing] == fallback).all() and (conf[nothing] == 0).all()
    assert (conf[~nothing] >= 40).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_two_classes_with_160_on_both(cuda, dtype):
    z = logits((1, 33, 70), 2, 8, dtype, 1.0, 8)
    label, conf, plain = run_both(z, 2, [160, 160], 18, (0, 0, 33, 70))
    fell = label == 18  # at most one class holds a score above 128: kept or fallback, never the runner-up
    assert 0.05 <= fell.mean() <= 0.95
    assert (label[~fell] == plain[~fell]).all() and (conf[~fell] >= 160).all() and (conf[fell] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_one_class(cuda, dtype):
    z = logits((1, 6, 11), 1, 8, dtype, 2.0, 4)
    label, conf, _ = run_both(z, 1, [255], 7, (1, 2, 4, 8))  # the only class always scores 255
    assert not label.any() and (conf == 255).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_exact_ties(cuda, dtype):
    from flairhip import ops
    K, cp = 19, 32
    z = logits((1, 8, 64), K, cp, dtype, 1.0, 6)
    z[..., 5] = 6.0
    z[..., 11] = 6.0  # two classes share the maximum of every pixel, and so the score (about 127)
    q = ops.predict_u8(z, K, "class_prob").cpu().numpy()
    assert (q[:, 5] == q[:, 11]).all() and (q[:, 5] > 100).all()
    thr = [0] * K
    label, conf, plain = run_both(z, K, thr, 18, (0, 0, 8, 64))
    assert (label == 5).all() and (plain == 5).all()  # both pass: the lowest index
    thr[5], thr[11] = 200, 100
    label, conf, _ = run_both(z, K, thr, 18, (0, 0, 8, 64))
    assert (label == 11).all() and (conf == q[:, 11]).all()  # the lower index does not pass: the other one
    thr[11] = 200
    thr[:5] = [1] * 5
    label, _, _ = run_both(z, K, thr, 18, (0, 0, 8, 64))
    assert not np.isin(label, (5, 11)).any()  # neither passes: the best of the rest, or the fallback


def test_refusals(cuda, lib):
    from flairhip import lib as L, ops
    K, cp = 19, 32
    z = torch.zeros((1, 8, 8, cp), dtype=torch.bfloat16, device=cuda)
    acc = ops.tta_buffer(1, K, 8, 8, cuda, cp=cp)
    thr = torch.zeros(K, dtype=torch.uint8, device=cuda)
    out = torch.full((1, 2, 8, 8), 77, dtype=torch.uint8, device=cuda)
    P = ctypes.c_void_p

    def call(dtype=L.BF16, mode=0, fallback=18, k=K, pitch=cp, y0=0, h=8, t=thr.data_ptr()):
        return lib.ffa_predict_thresholded_u8(dtype, mode, P(z.data_ptr()), P(t), fallback, P(out.data_ptr()), 1, 8, 8,
                                              k, pitch, y0, 0, h, 8, None)

    def call_tta(mode=0, fallback=18, k=K, pitch=cp, views=1, t=thr.data_ptr()):
        return lib.ffa_tta_predict_thresholded_u8(mode, P(acc.data_ptr()), P(t), fallback, P(out.data_ptr()), 1, k,
                                                  pitch, 8, 8, views, None)

    for bad in (dict(mode=1), dict(mode=3), dict(dtype=2), dict(fallback=256), dict(fallback=-1), dict(k=0), dict(k=33),
                dict(pitch=12), dict(y0=1), dict(h=0), dict(t=None)):
        assert call(**bad) == -1, bad
        assert lib.ffa_last_error().decode().startswith("predict_thresholded_u8:"), bad
    for bad in (dict(mode=1), dict(fallback=256), dict(k=33), dict(pitch=12), dict(views=0), dict(t=None)):
        assert call_tta(**bad) == -1, bad
        assert lib.ffa_last_error().decode().startswith("tta_predict_thresholded_u8:"), bad
    torch.cuda.synchronize()
    assert (out == 77).all()
    with pytest.raises(ValueError, match="class_prob"):
        ops.predict_thresholded_u8(z, K, "class_prob", thr, 18)
    with pytest.raises(ValueError, match="class_prob"):
        ops.tta_predict_thresholded_u8(acc, "class_prob", 1, thr, 18)
    with pytest.raises(ValueError, match="18 thresholds for 19 classes"):
        ops.predict_thresholded_u8(z, K, "argmax", thr[:18].contiguous(), 18)
    with pytest.raises(ValueError):
        ops.predict_thresholded_u8(z, K, "argmax", thr.cpu(), 18)
    with pytest.raises(ValueError):
        ops.predict_thresholded_u8(z, K, "argmax", thr, 256)


# ---- the TTA entry -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["argmax", "argmax_conf"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_one_identity_view_equals_the_logits_entry(cuda, dtype, mode):
    from flairhip import ops
    K, cp, crop = 19, 32, (4, 6, 30, 27)
    thr = torch.tensor([160 if k % 2 == 0 else 40 for k in range(K)], dtype=torch.uint8, device=cuda)
    z = logits((2, 40, 40), K, cp, dtype, 2.0, 12)
    acc = ops.tta_buffer(2, K, crop[2], crop[3], cuda, cp=cp)
    ops.tta_accumulate_(acc, z, K, 0, crop=crop, first=True)
    for fallback in (18, 255):
        got = ops.tta_predict_thresholded_u8(acc, mode, 1, thr, fallback)
        assert torch.equal(got, ops.predict_thresholded_u8(z, K, mode, thr, fallback, crop=crop))
    zero = torch.zeros(K, dtype=torch.uint8, device=cuda)
    assert torch.equal(ops.tta_predict_thresholded_u8(acc, mode, 1, zero, 3), ops.tta_predict_u8(acc, mode, 1))


@pytest.mark.parametrize("K,cp,thr_of", [(19, 32, lambda k: 120 if k % 2 == 0 else 30), (2, 8, lambda k: 160)])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_four_views_follow_the_rule_on_the_mean_probabilities(cuda, dtype, K, cp, thr_of):
    from flairhip import ops
    from flairhip.augment import tta_views
    crop = (2, 3, 29, 26)
    thr = [thr_of(k) for k in range(K)]
    thr_dev = torch.tensor(thr, dtype=torch.uint8, device=cuda)
    views = tta_views("flips")
    acc = ops.tta_buffer(2, K, crop[2], crop[3], cuda, cp=cp)
    for v, code in enumerate(views):
        ops.tta_accumulate_(acc, logits((2, 32, 32), K, cp, dtype, 2.0, 40 + v), K, code, crop=crop, first=v == 0)
    p = ops.tta_probabilities(acc, len(views)).cpu().numpy()
    q = ops.tta_predict_u8(acc, "class_prob", len(views)).cpu().numpy()
    want_label, want_conf = rule(p, q, thr, 18)
    nothing = want_label == 18 if K == 2 else ~(q >= np.asarray(thr, dtype=np.uint8)[None, :, None, None]).any(1)
    plain = ops.tta_predict_u8(acc, "argmax", len(views)).cpu().numpy()
    print(f"kept {(want_label == plain).mean():.3f}, fallback {nothing.mean():.3f}")
    assert nothing.mean() >= 0.05 and (want_label == plain).mean() >= 0.05
    got0 = ops.tta_predict_thresholded_u8(acc, "argmax", len(views), thr_dev, 18)
    got2 = ops.tta_predict_thresholded_u8(acc, "argmax_conf", len(views), thr_dev, 18)
    assert tuple(got0.shape) == (2, crop[2], crop[3]) and tuple(got2.shape) == (2, 2, crop[2], crop[3])
    assert np.array_equal(got0.cpu().numpy(), want_label)
    assert np.array_equal(got2[:, 0].cpu().numpy(), want_label)
    assert np.array_equal(got2[:, 1].cpu().numpy(), want_conf)
