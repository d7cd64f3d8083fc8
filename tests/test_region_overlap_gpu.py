"""Region overlaps on the device (csrc/region_overlap.hip, ops.region_overlaps) against their definition restated in
numpy (tests/objects_oracle.py).  Every comparison is exact integer equality: both region tables, the pair list after
the sort of the ops level, the pair bound Q against the oracle's head count, and n_pairs <= Q."""
import numpy as np
import pytest
import torch

import objects_oracle as oracle

pytestmark = pytest.mark.gpu


# ---- inputs -------------------------------------------------------------------------------------------------------

def blobs(H, W, seed, classes=3, cell=(4, 5), salt=0.05):
    """coarse random cells of `classes` values with salt noise: regions of every size, many of one pixel"""
    g = np.random.default_rng(seed)
    ch, cw = cell
    coarse = g.integers(0, classes, ((H + ch - 1) // ch, (W + cw - 1) // cw))
    out = np.repeat(np.repeat(coarse, ch, 0), cw, 1)[:H, :W].astype(np.uint8)
    m = g.random((H, W)) < salt
    out[m] = g.integers(0, classes, int(m.sum()))
    return out


_oracle_cache = {}


def want(a, b, bga=None, bgb=None, mpa=1, mpb=1):
    key = (a.tobytes(), b.tobytes(), a.shape, bga, bgb, mpa, mpb)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.full(a, b, bga, bgb, mpa, mpb)
    return _oracle_cache[key]


def product(cuda, a, b, bga=None, bgb=None, mpa=1, mpb=1):
    from flairhip import ops
    return ops.region_overlaps(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), bga, bgb, mpa, mpb)


def table_of(first, cls, pixels):
    assert first.dtype == torch.int32 and cls.dtype == torch.int32 and pixels.dtype == torch.int64
    return list(zip(first.cpu().tolist(), cls.cpu().tolist(), pixels.cpu().tolist()))


def pairs_of(ov):
    assert ov.pair_a.dtype == torch.int32 and ov.pair_b.dtype == torch.int32 and ov.pair_pixels.dtype == torch.int64
    return list(zip(ov.pair_a.cpu().tolist(), ov.pair_b.cpu().tolist(), ov.pair_pixels.cpu().tolist()))


def check(cuda, a, b, **kw):
    ta, tb, pairs, Q = want(a, b, **kw)
    ov = product(cuda, a, b, **kw)
    assert table_of(ov.a_first, ov.a_class, ov.a_pixels) == ta
    assert table_of(ov.b_first, ov.b_class, ov.b_pixels) == tb
    assert pairs_of(ov) == pairs
    assert ov.pair_bound == Q and len(pairs) <= Q
    return ov


# ---- the smallest shapes at which each part can go wrong -----------------------------------------------------------

def test_single_pixel(cuda):
    one = np.array([[3]], np.uint8)
    ov = check(cuda, one, one)
    assert pairs_of(ov) == [(0, 0, 1)]
    assert pairs_of(check(cuda, one, one, bga=3)) == []


@pytest.mark.parametrize("shape", [(1, 70), (70, 1)])
def test_run_across_the_lane_63_64_boundary(cuda, shape):
    a = np.ones(70, np.uint8)
    b = np.array([0] * 60 + [1] * 10, np.uint8)  # the second run covers lanes 60 .. 63 of wave 0 and 0 .. 5 of wave 1
    ov = check(cuda, a.reshape(shape), b.reshape(shape))
    assert pairs_of(ov) == [(0, 0, 60), (0, 1, 10)]


def test_ragged_tiles_and_one_seam_each_way(cuda):
    check(cuda, blobs(33, 65, 1), blobs(33, 65, 2))


def test_4096_distinct_pairs(cuda):
    """every pixel of a is a region of its own, b has 64 vertical stripes: probing, collisions and the compaction"""
    a = (np.add.outer(np.arange(64), np.arange(64)) % 2).astype(np.uint8)
    b = np.broadcast_to((np.arange(64) % 2).astype(np.uint8), (64, 64)).copy()
    ov = check(cuda, a, b)
    assert len(ov.pair_a) == 4096 == ov.pair_bound and int(ov.pair_pixels.sum()) == 4096


def test_a_pair_at_the_end_of_one_row_and_the_start_of_the_next(cuda):
    """the flat run that joins the end of row 1 to the start of row 2 must count both"""
    a = np.ones((3, 70), np.uint8)
    b = np.zeros((3, 70), np.uint8)
    b[0, :] = 1
    b[:, :5] = 1
    b[:, 65:] = 1
    ov = check(cuda, a, b, bgb=0)
    assert pairs_of(ov) == [(0, 0, 70 + 2 * 10)]


def test_one_region_over_four_tiles_against_small_regions(cuda):
    a = np.zeros((48, 48), np.uint8)
    a[28:36, 4:44] = 1   # a cross through the tile corner at (32, 32)
    a[4:44, 28:36] = 1
    yy, xx = np.mgrid[0:48, 0:48]
    b = (((yy // 3) + (xx // 3)) % 2 + 1).astype(np.uint8)  # 3 x 3 squares, each its own region
    ov = check(cuda, a, b, bga=0)
    assert len(ov.a_first) == 1 and len(ov.pair_a) > 50  # the arms cross dozens of the squares


BLOB_A, BLOB_B = blobs(97, 130, 3), blobs(97, 130, 4)


@pytest.mark.parametrize("bg", [None, 0])
@pytest.mark.parametrize("mpa,mpb", [(1, 1), (5, 1), (1, 5), (5, 5)])
def test_random_blobs(cuda, bg, mpa, mpb):
    check(cuda, BLOB_A, BLOB_B, bga=bg, bgb=bg, mpa=mpa, mpb=mpb)


def test_different_backgrounds_per_side(cuda):
    check(cuda, BLOB_A, BLOB_B, bga=1, bgb=None, mpa=2, mpb=3)


@pytest.mark.parametrize("side", ["a", "b"])
def test_one_raster_all_background(cuda, side):
    x, z = blobs(33, 65, 5), np.zeros((33, 65), np.uint8)
    a, b = (z, x) if side == "a" else (x, z)
    ov = check(cuda, a, b, bga=0, bgb=0)
    assert ov.pair_bound == 0 and len(ov.pair_a) == 0
    assert len(ov.a_first if side == "a" else ov.b_first) == 0 and len(ov.b_first if side == "a" else ov.a_first) > 0


def test_regions_only_in_the_last_rows(cuda):
    """300 x 300 is 22 scan blocks: the index of a late region is wrong without the block sums"""
    a, b = np.zeros((300, 300), np.uint8), np.zeros((300, 300), np.uint8)
    a[297:], b[296:] = blobs(3, 300, 6, cell=(1, 3)) + 1, blobs(4, 300, 7, cell=(2, 2)) + 1
    ov = check(cuda, a, b, bga=0, bgb=0)
    assert int(ov.a_first.min()) >= 297 * 300


def test_512_against_the_oracle(cuda):
    check(cuda, blobs(512, 512, 8, cell=(9, 11), salt=0.02), blobs(512, 512, 9, cell=(7, 13), salt=0.02), bga=0, bgb=0,
          mpa=3, mpb=2)


# ---- properties ------------------------------------------------------------------------------------------------------

def test_swapping_the_rasters_transposes_the_list(cuda):
    ab = product(cuda, BLOB_A, BLOB_B, bga=0, bgb=None, mpa=2, mpb=1)
    ba = product(cuda, BLOB_B, BLOB_A, bga=None, bgb=0, mpa=1, mpb=2)
    assert table_of(ab.a_first, ab.a_class, ab.a_pixels) == table_of(ba.b_first, ba.b_class, ba.b_pixels)
    assert table_of(ab.b_first, ab.b_class, ab.b_pixels) == table_of(ba.a_first, ba.a_class, ba.a_pixels)
    assert sorted((y, x, n) for x, y, n in pairs_of(ab)) == pairs_of(ba)


def test_pair_pixels_sum_to_what_both_keep(cuda):
    ov = product(cuda, BLOB_A, BLOB_B, bga=0, bgb=0, mpa=5, mpb=5)
    per_a = torch.zeros_like(ov.a_pixels).index_add_(0, ov.pair_a.long(), ov.pair_pixels)
    per_b = torch.zeros_like(ov.b_pixels).index_add_(0, ov.pair_b.long(), ov.pair_pixels)
    assert bool((per_a <= ov.a_pixels).all()) and bool((per_b <= ov.b_pixels).all())
    ia, _ = oracle.regions(BLOB_A, 0, 5)
    ib, _ = oracle.regions(BLOB_B, 0, 5)
    assert int(ov.pair_pixels.sum()) == int(((ia >= 0) & (ib >= 0)).sum())


def test_two_runs_give_equal_bytes(cuda):
    x, y = product(cuda, BLOB_A, BLOB_B), product(cuda, BLOB_A, BLOB_B)
    for name in ("a_first", "a_class", "a_pixels", "b_first", "b_class", "b_pixels", "pair_a", "pair_b", "pair_pixels"):
        assert torch.equal(getattr(x, name), getattr(y, name)), name


@pytest.mark.parametrize("bg,mp", [(None, 1), (0, 4)])
def test_class_sorted_table_is_the_polygon_order(cuda, bg, mp):
    from flairhip import ops
    ov = product(cuda, BLOB_A, BLOB_B, bga=bg, bgb=bg, mpa=mp, mpb=mp)
    for cls, rc, rp in ((BLOB_A, ov.a_class, ov.a_pixels), (BLOB_B, ov.b_class, ov.b_pixels)):
        poly_class, poly_pixels = ops.polygonize(torch.from_numpy(cls).to(cuda), bg, mp)[:2]
        order = torch.sort(rc, stable=True).indices
        assert torch.equal(rc[order], poly_class) and torch.equal(rp[order], poly_pixels)


def test_batch_equals_the_per_image_calls(cuda):
    from flairhip import ops
    a = np.stack([blobs(33, 65, 10 + i) for i in range(3)])  # blobs touch every border
    b = np.stack([blobs(33, 65, 20 + i) for i in range(3)])
    got = ops.region_overlaps_batch(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), 0, None, 2, 1)
    assert len(got) == 3
    for i, ov in enumerate(got):
        ta, tb, pairs, Q = want(a[i], b[i], bga=0, bgb=None, mpa=2, mpb=1)
        assert table_of(ov.a_first, ov.a_class, ov.a_pixels) == ta
        assert table_of(ov.b_first, ov.b_class, ov.b_pixels) == tb
        assert pairs_of(ov) == pairs and ov.pair_bound == Q


def test_argument_errors(cuda):
    from flairhip import ops
    a = torch.zeros((4, 5), dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        ops.region_overlaps(a, torch.zeros((5, 4), dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        ops.region_overlaps(a, a.cpu())
    with pytest.raises(ValueError):
        ops.region_overlaps(a, a.int())
    with pytest.raises(ValueError):
        ops.region_overlaps(a, a, background_a=256)
