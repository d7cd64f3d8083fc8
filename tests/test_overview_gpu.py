"""ops.overview_pyramid (csrc/overview.hip) against the numpy oracle of the definition in include/flairhip.h: every
shape at which the kernel takes another path, data built for the rules' corner cases.  All comparisons are exact."""
import numpy as np
import pytest
import torch

from flairhip import ops
from overview_oracle import n_levels, next_level, pyramid

pytestmark = pytest.mark.gpu

METHODS = ["nearest", "mode", "average"]

# (bands, H, W, block): single pixels and lines; ragged multi-band; exactly one 64 x 256 tile, one pixel more and one
# less; a level-1 width that is no multiple of 16 (rows of the destination start on any byte: the unaligned store and,
# from level 1 on, load paths); more than four levels (a second launch on level 4); several tiles both ways
SHAPES = [(1, 1, 1, 1), (1, 1, 7, 1), (1, 7, 1, 1), (1, 2, 2, 1), (3, 37, 53, 4), (1, 64, 256, 8), (1, 65, 257, 8),
          (1, 63, 255, 8), (2, 100, 270, 16), (1, 130, 520, 8), (2, 131, 777, 1)]


def _run(base, block, method, ignore=None):
    got = ops.overview_pyramid(torch.from_numpy(base).cuda(), block=block, method=method, ignore=ignore)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in got]


def _compare(base, block, method, ignore=None):
    _, H, W = base.shape
    L = n_levels(H, W, block)
    want = pyramid(base, L, method, ignore)
    got = _run(base, block, method, ignore)
    assert len(got) == L == ops.overview_levels(H, W, block)
    for l, (g, w) in enumerate(zip(got, want), 1):
        assert g.shape == w.shape == (base.shape[0], -(-H // 2 ** l), -(-W // 2 ** l))
        assert np.array_equal(g, w), f"{method}: level {l} of {base.shape} differs at {np.argwhere(g != w)[:5].tolist()}"
    return got


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_classes_match_the_oracle(cuda, shape, method):
    bands, H, W, block = shape
    base = np.random.default_rng(H * 1000 + W).integers(0, 4, (bands, H, W), dtype=np.uint8)  # 4 classes: many ties
    got = _compare(base, block, method)
    if shape == (1, 130, 520, 8):
        assert len(got) == 7  # more than one launch
    if method == "nearest":
        for l, g in enumerate(got, 1):
            assert np.array_equal(g, base[..., ::2 ** l, ::2 ** l])


@pytest.mark.parametrize("method", METHODS)
def test_full_byte_range(cuda, method):
    base = np.random.default_rng(11).integers(0, 256, (2, 100, 270), dtype=np.uint8)
    _compare(base, 16, method)


def test_mode_ties_take_the_smaller_value(cuda):
    # every 2 x 2 block is a 2-2 tie, in all three arrangements (rows, columns, diagonals), with the smaller value in
    # either position
    H, W = 66, 260
    g = np.random.default_rng(2)
    a = g.integers(0, 200, (H // 2, W // 2))
    b = a + g.integers(1, 50, (H // 2, W // 2))
    kind = g.integers(0, 6, (H // 2, W // 2))
    lo_first = kind % 2 == 0
    p, q = np.where(lo_first, a, b), np.where(lo_first, b, a)
    base = np.zeros((1, H, W), np.uint8)
    arr = kind // 2  # 0: rows p p / q q, 1: columns p q / p q, 2: diagonals p q / q p
    base[0, 0::2, 0::2] = p
    base[0, 0::2, 1::2] = np.where(arr == 0, p, q)
    base[0, 1::2, 0::2] = np.where(arr == 1, p, q)
    base[0, 1::2, 1::2] = np.where(arr == 2, p, q)
    got = _compare(base, 64, "mode")
    assert np.array_equal(got[0][0], a.astype(np.uint8))


def test_mode_ignore(cuda):
    # blocks that are all ignore, part ignore, a tie after ignoring, and ignore as the would-be winner
    blocks = np.array([[255, 255, 255, 255], [255, 7, 255, 255], [255, 255, 9, 3], [255, 255, 255, 4],
                       [5, 255, 2, 255], [255, 3, 3, 8], [1, 1, 255, 255], [255, 6, 6, 6], [4, 2, 2, 4]], np.uint8)
    want1 = np.array([255, 7, 3, 4, 2, 3, 1, 6, 2], np.uint8)
    base = np.zeros((1, 2, 2 * len(blocks)), np.uint8)
    for k, b in enumerate(blocks):
        base[0, :, 2 * k:2 * k + 2] = b.reshape(2, 2)
    got = _compare(base, 1, "mode", ignore=255)
    assert np.array_equal(got[0][0, 0], want1)
    without = _compare(base, 1, "mode")  # every value votes: 255 wins where it is the most frequent
    assert without[0][0, 0].tolist() == [255, 255, 255, 255, 255, 3, 1, 6, 2]
    # a zone-clipped class raster: 255 outside a disc, ragged sizes, several tiles
    g = np.random.default_rng(4)
    cls = g.integers(0, 4, (1, 150, 530), dtype=np.uint8)
    yy, xx = np.mgrid[:150, :530]
    cls[0, (yy - 70) ** 2 + (xx - 260) ** 2 > 60 ** 2] = 255
    _compare(cls, 8, "mode", ignore=255)


def test_average_rounds_half_up(cuda):
    # n = 4: sums 0 .. 1020 with every remainder mod 4; extremes stay exact
    rows = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1], [255, 255, 255, 255], [255, 255, 255, 254],
                     [255, 255, 254, 254], [255, 254, 254, 254], [0, 255, 0, 255], [0, 0, 0, 255], [255, 255, 255, 0]])
    want = [0, 0, 1, 1, 255, 255, 255, 254, 128, 64, 191]
    base = np.zeros((1, 2, 2 * len(rows)), np.uint8)
    for k, b in enumerate(rows):
        base[0, :, 2 * k:2 * k + 2] = b.reshape(2, 2)
    got = _compare(base, 1, "average")
    assert got[0][0, 0].tolist() == want
    # n = 2 (last column / last row of an odd raster) and n = 1 (its corner)
    base = np.array([[[0, 1, 254], [1, 1, 255], [7, 8, 255]]], np.uint8)
    got = _compare(base, 1, "average")
    assert got[0][0].tolist() == [[1, 255], [8, 255]]  # (0+1+1+1+2)/4 = 1; (254+255+1)/2 = 255; (7+8+1)/2 = 8; 255
    base = np.random.default_rng(6).integers(0, 2, (1, 131, 515), dtype=np.uint8) * 255
    _compare(base, 4, "average")


def test_levels_are_views_of_one_allocation_and_repeat_exactly(cuda):
    base = torch.from_numpy(np.random.default_rng(8).integers(0, 19, (3, 100, 270), dtype=np.uint8)).cuda()
    a = ops.overview_pyramid(base, block=16, method="mode")
    b = ops.overview_pyramid(base, block=16, method="mode")
    assert len(a) == 5
    store = a[0].untyped_storage().data_ptr()
    pos = a[0].data_ptr()
    for lv in a:
        assert lv.untyped_storage().data_ptr() == store and lv.data_ptr() == pos and lv.is_contiguous()
        pos += lv.numel()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert ops.overview_pyramid(base, block=512) == []


def test_levels_past_the_single_pixel_repeat_it(cuda, lib):
    # the C entry point takes any level count up to 30: past the 1 x 1 level every level repeats it
    small = np.random.default_rng(8).integers(0, 19, (1, 5, 3), dtype=np.uint8)
    base = torch.from_numpy(small).cuda()
    n = lib.ffa_overview_pyramid_bytes(1, 5, 3, 5)
    assert n == 3 * 2 + 2 * 1 + 1 + 1 + 1
    pyr = torch.zeros(n, dtype=torch.uint8, device=cuda)
    assert lib.ffa_overview_pyramid_u8(base.data_ptr(), pyr.data_ptr(), 1, 5, 3, 5, 2, -1, None) == 0
    torch.cuda.synchronize()
    want = np.concatenate([lv.reshape(-1) for lv in pyramid(small, 5, "average")])
    assert np.array_equal(pyr.cpu().numpy(), want) and want[-1] == want[-2] == want[-3]


def test_cascade_is_not_a_resampling_of_the_base(cuda):
    # mode of modes: level 2 comes from level 1 (the definition), which differs from the mode of the 4 x 4 base block
    base = np.array([[[1, 1, 2, 2], [1, 3, 2, 4], [5, 5, 6, 6], [5, 7, 6, 8]]], np.uint8)
    lv1 = next_level(base, "mode")
    assert lv1[0].tolist() == [[1, 2], [5, 6]]
    got = _compare(base, 1, "mode")
    assert got[1][0].tolist() == [[1]]


def test_bad_arguments(cuda, lib):
    base = torch.zeros((1, 8, 8), dtype=torch.uint8, device=cuda)
    out = torch.zeros(64, dtype=torch.uint8, device=cuda)
    bp, op = base.data_ptr(), out.data_ptr()
    ERR_ARG = -1
    assert lib.ffa_overview_levels(0, 8, 4) == ERR_ARG and lib.ffa_overview_levels(8, 8, 0) == ERR_ARG
    assert lib.ffa_overview_levels(8, 8, 8) == 0 and lib.ffa_overview_levels(9, 8, 8) == 1
    assert lib.ffa_overview_levels(5000, 5000, 512) == 4 and lib.ffa_overview_levels(20000, 20000, 512) == 6
    assert lib.ffa_overview_pyramid_bytes(1, 8, 8, 2) == 16 + 4 and lib.ffa_overview_pyramid_bytes(3, 37, 53, 0) == 0
    assert lib.ffa_overview_pyramid_bytes(3, 37, 53, 2) == 3 * (19 * 27 + 10 * 14)
    assert lib.ffa_overview_pyramid_bytes(0, 8, 8, 1) == ERR_ARG
    assert lib.ffa_overview_pyramid_bytes(1, 1 << 16, 1 << 15, 1) == ERR_ARG  # bands * H * W = 2^31
    assert lib.ffa_overview_pyramid_bytes(1, 8, 8, 31) == ERR_ARG
    for args in [(0, 8, 8, 1, 0, -1), (1, 0, 8, 1, 0, -1), (1, 8, 0, 1, 0, -1), (1, 8, 8, -1, 0, -1),
                 (1, 8, 8, 31, 0, -1), (1, 8, 8, 1, 3, -1), (1, 8, 8, 1, -1, -1), (1, 8, 8, 1, 1, 256),
                 (1, 8, 8, 1, 1, -2), (1, 8, 8, 1, 2, 0), (1, 1 << 16, 1 << 15, 1, 0, -1)]:
        assert lib.ffa_overview_pyramid_u8(bp, op, *args, None) == ERR_ARG, args
    assert lib.ffa_overview_pyramid_u8(None, op, 1, 8, 8, 1, 0, -1, None) == ERR_ARG
    assert lib.ffa_overview_pyramid_u8(bp, None, 1, 8, 8, 1, 0, -1, None) == ERR_ARG
    assert lib.ffa_overview_pyramid_u8(bp, None, 1, 8, 8, 0, 0, -1, None) == 0  # no level: nothing to write
    assert b"overview" in lib.ffa_last_error()
    with pytest.raises(ValueError, match="uint8"):
        ops.overview_pyramid(base.float())
    with pytest.raises(ValueError, match="CUDA"):
        ops.overview_pyramid(base.cpu())
    with pytest.raises(ValueError, match=r"\[bands, H, W\]"):
        ops.overview_pyramid(base[0])
    with pytest.raises(ValueError, match="contiguous"):
        ops.overview_pyramid(base.expand(2, 8, 8).transpose(1, 2))
    with pytest.raises(ValueError, match="method"):
        ops.overview_pyramid(base, method="cubic")
    with pytest.raises(ValueError, match="ignore"):
        ops.overview_pyramid(base, method="mode", ignore=256)
    with pytest.raises(ValueError, match="ignore"):
        ops.overview_pyramid(base, method="average", ignore=0)
    with pytest.raises(ValueError, match="block"):
        ops.overview_pyramid(base, block=0)
    torch.cuda.synchronize()
