"""ffa_calib_hist (csrc/calibration.hip) through ops.calib_hist: the per-class histograms of the score bytes, split by
whether the pixel's target is the class.

Oracle: the bytes ops.predict_u8(..., "class_prob") writes for the same logits, read to the host, and np.bincount per
class and side.  Integer counts of bytes an older kernel wrote: exact equality, nothing to tolerate.

Shapes: 1, 255, 256, 257 and 3 * 256 + 17 pixels (one lane, a ragged tile, a full tile, two tiles, four tiles) for every
K / pitch in (1, 8), (2, 8), (8, 8), (19, 24), (19, 32), (24, 24), (32, 32) in bf16 and f32 -- one per size of the
kernel's register arrays and per pitch; the pairs whose bins do not fit the block's LDS beside the staging tile (bf16:
32/32; f32: all from 19/24 on) walk the classes in two or three chunks.  300 001 pixels are above the grid cap of 1024
blocks x 256 threads, where blocks walk more than one tile.  About 6 % of the targets are >= K (255 and K itself).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NPIX = [1, 255, 256, 257, 3 * 256 + 17]
CLASSES = [(1, 8), (2, 8), (8, 8), (19, 24), (19, 32), (24, 24), (32, 32)]
DTYPES = [torch.bfloat16, torch.float32]
DEV = "cuda:0"


def targets(npix, K, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (npix,), generator=g).to(torch.uint8)
    r = torch.rand(npix, generator=g)
    t[r < 0.03] = 255
    t[(r >= 0.03) & (r < 0.06)] = K  # the first value that is no class
    return t


def oracle(z, t, K):
    """-> int64 [K, 2, 256] from the bytes of predict_u8 'class_prob' (z: [1, 1, npix, cp] on the GPU, t: uint8 [npix])"""
    from flairhip import ops
    q = ops.predict_u8(z, K, "class_prob").cpu().numpy().reshape(K, -1)
    t = t.cpu().numpy().reshape(-1)
    valid = t < K
    hist = np.zeros((K, 2, 256), dtype=np.int64)
    for k in range(K):
        for side in (0, 1):
            hist[k, side] = np.bincount(q[k][valid & ((t == k) == bool(side))], minlength=256)
    return hist


def check_sums(hist, t, K):
    t = t.cpu().numpy().reshape(-1)
    for k in range(K):
        assert hist[k, 1].sum() == (t == k).sum(), k
        assert hist[k].sum() == (t < K).sum(), k  # a target >= K appears on neither side


@functools.lru_cache(maxsize=None)
def case(npix, K, cp, dtype):
    """inputs on the GPU and the oracle's histograms, built once and shared: nobody writes to them"""
    g = torch.Generator().manual_seed(npix * 131 + K * 7 + cp + (dtype == torch.float32))
    z = (3.0 * torch.randn(npix, cp, generator=g)).to(dtype).reshape(1, 1, npix, cp).to(DEV)
    t = targets(npix, K, npix + K).reshape(1, 1, npix).to(DEV)
    return z, t, oracle(z, t, K)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("K,cp", CLASSES)
@pytest.mark.parametrize("npix", NPIX)
def test_histograms_equal_the_bincount_of_the_class_prob_bytes(cuda, npix, K, cp, dtype):
    from flairhip import ops
    z, t, want = case(npix, K, cp, dtype)
    hist = ops.calib_hist(z, t, K)
    assert hist.dtype == torch.int64 and tuple(hist.shape) == (K, 2, 256) and hist.device == z.device
    got = hist.cpu().numpy()
    assert np.array_equal(got, want)
    check_sums(got, t, K)
    if npix > 1 and K > 1:
        assert (t >= K).any() and ((got > 0).sum(-1) > 2).any()  # ignored targets are there; so are scores in 1..254


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_blocks_that_walk_several_tiles(cuda, dtype):
    from flairhip import ops
    npix, K, cp = 300_001, 19, 32  # 1172 tiles for 1024 blocks
    z, t, want = case(npix, K, cp, dtype)
    got = ops.calib_hist(z, t, K).cpu().numpy()
    assert np.array_equal(got, want)
    check_sums(got, t, K)


def test_a_block_that_walks_more_than_255_tiles(cuda):
    """A lane keeps its counts of the bins 0 and 255 in 8-bit fields that are emptied every 255 tiles: 1024 blocks x 256
    threads x 255 tiles + 257 pixels give the first blocks a 256th tile.  Saturated logits at the smallest pitch, so
    that every count goes through those fields; the oracle is a bincount on the device, of the same class_prob bytes."""
    from flairhip import ops
    K, cp, npix = 2, 8, 1024 * 256 * 255 + 257
    g = torch.Generator(device=cuda).manual_seed(3)
    winner = torch.randint(0, K, (npix,), device=cuda, generator=g)
    z = torch.full((1, 1, npix, cp), -40.0, dtype=torch.bfloat16, device=cuda)
    z[0, 0, torch.arange(npix, device=cuda), winner] = 40.0
    del winner
    t = torch.randint(0, K + 1, (1, 1, npix), device=cuda, generator=g).to(torch.uint8)  # a third of them no class
    q = ops.predict_u8(z, K, "class_prob").reshape(K, npix)
    tt = t.reshape(-1)
    want = torch.stack([torch.bincount((tt[tt < K] == k).long() * 256 + q[k][tt < K].long(), minlength=512)
                        for k in range(K)]).reshape(K, 2, 256)
    got = ops.calib_hist(z, t, K)
    assert torch.equal(got, want)
    assert int(got[0].sum()) == int((tt < K).sum()) and not bool(got[:, :, 1:255].any())


def hot_logits(kind, npix, K, cp, dtype):
    g = torch.Generator().manual_seed(5 + npix + K)
    winner = torch.randint(0, K, (npix,), generator=g)
    sat = torch.full((npix, cp), -40.0)
    sat[torch.arange(npix), winner] = 40.0
    if kind == "saturated":  # every score is 0 or 255: the ballots count them all
        z = sat
    elif kind == "constant":  # every class of every pixel has the same score
        z = torch.full((npix, cp), 1.25)
    else:  # lanes 0..31 of every wave saturated, lanes 32..63 broad: hot and mid bins in one wave
        z = torch.where((torch.arange(npix) % 64 < 32)[:, None], sat, 2.0 * torch.randn(npix, cp, generator=g))
    return z.to(dtype).reshape(1, 1, npix, cp).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("K,cp", [(2, 8), (19, 32), (32, 32)])
@pytest.mark.parametrize("kind", ["saturated", "constant", "mixed"])
def test_hot_bins(cuda, kind, K, cp, dtype):
    from flairhip import ops
    npix = 3 * 256 + 17
    z = hot_logits(kind, npix, K, cp, dtype)
    t = targets(npix, K, 99).reshape(1, 1, npix).to(DEV)
    want = oracle(z, t, K)
    got = ops.calib_hist(z, t, K).cpu().numpy()
    assert np.array_equal(got, want)
    check_sums(got, t, K)
    occupied = np.nonzero(got.sum((0, 1)))[0].tolist()
    if kind == "saturated":
        assert occupied == [0, 255]
    elif kind == "constant":
        assert occupied == [int(np.rint(np.float32(1.0) / np.float32(K) * np.float32(255.0)))]
    else:
        assert occupied[0] == 0 and occupied[-1] == 255 and len(occupied) > 2


def test_two_calls_accumulate_and_equal_calls_give_equal_bytes(cuda):
    from flairhip import ops
    K, cp = 19, 32
    za, ta, wa = case(257, K, cp, torch.bfloat16)
    zb, tb, wb = case(3 * 256 + 17, K, cp, torch.bfloat16)
    hist = ops.calib_hist(za, ta, K)
    assert ops.calib_hist(zb, tb, K, hist=hist) is hist
    assert np.array_equal(hist.cpu().numpy(), wa + wb)
    again = ops.calib_hist(zb, tb, K, hist=ops.calib_hist(za, ta, K))
    assert torch.equal(hist, again)
    before = torch.arange(K * 512, dtype=torch.int64, device=cuda).reshape(K, 2, 256) * (1 << 33)  # beyond 32 bits
    acc = before.clone()
    ops.calib_hist(zb, tb, K, hist=acc)
    assert np.array_equal((acc - before).cpu().numpy(), wb)


def test_no_pixels_leave_the_histograms_untouched(cuda, lib):
    from flairhip import lib as L, ops
    K, cp = 19, 32
    before = torch.arange(K * 512, dtype=torch.int64, device=cuda).reshape(K, 2, 256)
    hist = before.clone()
    z = torch.empty((1, 1, 0, cp), dtype=torch.bfloat16, device=cuda)
    t = torch.empty((1, 1, 0), dtype=torch.uint8, device=cuda)
    assert ops.calib_hist(z, t, K, hist=hist) is hist
    assert lib.ffa_calib_hist(L.BF16, None, None, 0, K, cp, hist.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(hist, before)
    fresh = ops.calib_hist(z, t, K)
    assert tuple(fresh.shape) == (K, 2, 256) and not bool(fresh.any())


def test_refusals(cuda, lib):
    from flairhip import lib as L, ops
    K, cp, npix = 19, 32, 64
    z = torch.zeros((1, 1, npix + 1, cp), dtype=torch.bfloat16, device=cuda)
    t = torch.zeros((1, 1, npix), dtype=torch.uint8, device=cuda)
    hist = torch.zeros((K, 2, 256), dtype=torch.int64, device=cuda)
    P = ctypes.c_void_p

    def call(dtype=L.BF16, logits=z.data_ptr(), tgt=t.data_ptr(), n=npix, k=K, pitch=cp, out=hist.data_ptr()):
        return lib.ffa_calib_hist(dtype, P(logits), P(tgt), n, k, pitch, P(out), None)

    for bad in (dict(dtype=2), dict(k=0), dict(k=33), dict(pitch=12), dict(k=19, pitch=16), dict(pitch=40), dict(n=-1),
                dict(n=(1 << 31) + 1), dict(logits=None), dict(tgt=None), dict(out=None),
                dict(logits=z.data_ptr() + 2)):  # the last: not 16-byte aligned
        assert call(**bad) == -1, bad
        assert lib.ffa_last_error().decode().startswith("calib_hist:"), bad
    torch.cuda.synchronize()
    assert not bool(hist.any())
    # the Python binding refuses what it can see itself
    with pytest.raises(ValueError):
        ops.calib_hist(z[:, :, :npix], t.to(torch.int32), K)
    with pytest.raises(ValueError):
        ops.calib_hist(z, t, K)  # one pixel more than targets
    with pytest.raises(ValueError):
        ops.calib_hist(z[:, :, :npix].contiguous(), t, K, hist=hist[:, :, :128])
    with pytest.raises(ValueError):
        ops.calib_hist(z[:, :, :npix].contiguous(), t, K, hist=hist.to(torch.int32))
