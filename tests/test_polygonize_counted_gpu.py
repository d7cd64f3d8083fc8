"""The count-sized polygoniser (ops.polygonize_counted: ffa_polygonize_count / _trace / _counted_emit /
_counted_zonal_sum_u8) against the bound-sized one (ops.polygonize), which tests/test_polygonize_gpu.py holds to the
scipy label oracle.  Normative: wherever both accept the input, all six output tensors are byte-identical.  Beyond
the old limit 4 * H * W < 2^31 the oracle is ops.polygonize on a small crop, shifted to where the crop was stamped.
"""

import numpy as np
import pytest
import torch

from test_polygonize_gpu import _eq_frames, spiral

pytestmark = pytest.mark.gpu

NAMES = ("poly_class", "poly_pixels", "poly_ring_offsets", "ring_vertex_offsets", "vertices", "sums")


def both(cls, background=None, min_pixels=1, values=None):
    from flairhip import ops
    c = torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).cuda()
    kw = {} if values is None else {"values": torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint8)).cuda()}
    old = [t.cpu().numpy() for t in ops.polygonize(c, background, min_pixels, **kw)]
    new = [t.cpu().numpy() for t in ops.polygonize_counted(c, background, min_pixels, **kw)]
    return old, new


def assert_same_bytes(old, new):
    assert len(old) == len(new)
    for name, a, b in zip(NAMES, old, new):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), name


def check_identity(cls, background=None, min_pixels=1, seed=0):
    """with values and without; the first five tensors must not depend on values either"""
    values = np.random.default_rng(seed).integers(0, 256, cls.shape).astype(np.uint8)
    old, new = both(cls, background, min_pixels)
    assert_same_bytes(old, new)
    old_v, new_v = both(cls, background, min_pixels, values)
    assert len(new_v) == 6
    assert_same_bytes(old_v, new_v)
    assert_same_bytes(old, new_v[:5])
    return new_v


def random_map(K, shape, seed):
    g = np.random.default_rng(seed)
    blocky = np.repeat(np.repeat(g.integers(0, K, (shape[0] // 4 + 1, shape[1] // 4 + 1)), 4, 0), 4, 1)
    cls = blocky[:shape[0], :shape[1]]
    return np.where(g.random(shape) < 0.1, g.integers(0, K, shape), cls).astype(np.uint8)


# the shapes cross the labeller's 32-pixel tile seams and the 64-lane boundaries; (700, 900) spans many blocks
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 130), (700, 900)])
@pytest.mark.parametrize("min_pixels", [1, 3, 50])
@pytest.mark.parametrize("bg", [None, 0])
@pytest.mark.parametrize("K", [2, 4])
def test_random_maps_byte_identical(cuda, K, bg, min_pixels, shape):
    check_identity(random_map(K, shape, K * 1000 + shape[0] * 7 + shape[1] + min_pixels), bg, min_pixels)


def test_checkerboard_counted_size_equals_the_bound(cuda):
    cls = (np.indices((64, 64)).sum(0) % 2).astype(np.uint8)
    out = check_identity(cls)
    assert len(out[0]) == 64 * 64 and len(out[4]) == 4 * 64 * 64  # E = 4 N: every edge slot of the bound is used


def test_all_background_launches_no_trace(cuda, monkeypatch):
    from flairhip import lib as L
    handle = L.load()
    old, _ = both(np.full((40, 50), 7, np.uint8), background=7)

    def no_trace(*a):
        raise AssertionError("ffa_polygonize_trace_bytes called although E = P = 0")

    monkeypatch.setattr(handle, "ffa_polygonize_trace_bytes", no_trace)
    values = np.full((40, 50), 9, np.uint8)
    _, new = both(np.full((40, 50), 7, np.uint8), background=7)
    assert_same_bytes(old, new)
    old_v, new_v = both(np.full((40, 50), 7, np.uint8), 7, 1, values)
    assert_same_bytes(old_v, new_v)
    assert len(new_v[0]) == 0 and list(new_v[2]) == [0] and list(new_v[3]) == [0] and new_v[4].shape == (0, 2)
    # every component below min_pixels: edges and polygons are counted on kept components only
    _, dropped = both(np.full((3, 3), 1, np.uint8), None, 10)
    assert len(dropped[0]) == 0 and list(dropped[2]) == [0]


def test_one_class_over_the_whole_raster(cuda):
    out = check_identity(np.full((123, 457), 4, np.uint8))
    assert len(out[0]) == 1 and len(out[4]) == 4


def test_pinch_inlet(cuda):
    cls = np.zeros((5, 5), np.uint8)
    cls[1:4, 1:4] = 1
    cls[2, 2] = 0
    cls[3, 3] = 0
    out = check_identity(cls, background=0)
    assert len(out[0]) == 1 and out[2][1] == 2


def test_concentric_squares_three_deep(cuda):
    cls = np.zeros((20, 20), np.uint8)
    cls[2:18, 2:18] = 1
    cls[5:15, 5:15] = 2
    cls[8:12, 8:12] = 3
    out = check_identity(cls)
    assert list(np.diff(out[2])) == [2, 2, 2, 1]


def test_long_spiral_ring(cuda):
    out = check_identity(spiral(400), background=1)
    assert len(out[0]) == 1 and out[3][1] - out[3][0] > 100_000  # one cycle far longer than E / rings on average


def test_deterministic_bytes(cuda):
    from flairhip import ops
    g = np.random.default_rng(9)
    cls = torch.from_numpy(g.integers(0, 4, (700, 900)).astype(np.uint8)).cuda()
    val = torch.from_numpy(g.integers(0, 256, (700, 900)).astype(np.uint8)).cuda()
    a = [t.cpu().numpy() for t in ops.polygonize_counted(cls, 3, 1, val)]
    b = [t.cpu().numpy() for t in ops.polygonize_counted(cls, 3, 1, val)]
    assert_same_bytes(a, b)


# ---- beyond 4 * H * W < 2^31 -------------------------------------------------------------------------------------------

BIG_H, BIG_W = 16385, 32768  # 2^29 + 2^15 pixels: pixel 2^29 is (row 16384, col 0), from there edge ids pass 2^31


def polygon_list(out, dy=0, dx=0):
    """[(class, pixels, sum, [ring as [(col, row), ...], ...])] in output order"""
    pc, pp, pro, rvo, verts, sums = out
    verts = verts.astype(np.int64) + np.array([dx, dy])
    return [(int(pc[q]), int(pp[q]), int(sums[q]),
             [[tuple(v) for v in verts[rvo[j]:rvo[j + 1]].tolist()] for j in range(pro[q], pro[q + 1])])
            for q in range(len(pc))]


def first_pixel(poly, W):
    """row-major index of the exterior's topmost-leftmost vertex = the component's first pixel"""
    y, x = min((y, x) for x, y in poly[3][0])
    return y * W + x


def test_beyond_the_old_limit(cuda):
    from flairhip import ops
    g = np.random.default_rng(41)
    crop = np.zeros((42, 62), np.uint8)
    crop[1:41, 1:61] = g.integers(1, 4, (40, 60))
    cval = g.integers(0, 256, crop.shape).astype(np.uint8)
    crop_dev, cval_dev = torch.from_numpy(crop).cuda(), torch.from_numpy(cval).cuda()
    small = [t.cpu().numpy() for t in ops.polygonize(crop_dev, 0, 1, cval_dev)]
    assert len(small[0]) > 100
    # (row, col) of the crop's corner.  The raster's outside is no component either, so a border row or column that
    # falls outside changes nothing: the second and third patches have pixels IN row 16384 (pixel index >= 2^29, edge
    # id >= 2^31), the third also in the last column.
    stamps = [(0, 0), (BIG_H - 41, 1000), (BIG_H - 41, BIG_W - 61)]
    cls = torch.zeros((BIG_H, BIG_W), dtype=torch.uint8, device=cuda)
    val = torch.zeros((BIG_H, BIG_W), dtype=torch.uint8, device=cuda)
    for r0, c0 in stamps:
        h, w = min(42, BIG_H - r0), min(62, BIG_W - c0)
        cls[r0:r0 + h, c0:c0 + w] = crop_dev[:h, :w]
        val[r0:r0 + h, c0:c0 + w] = cval_dev[:h, :w]
    with pytest.raises(ValueError):
        ops.polygonize(cls, 0)
    got = polygon_list([t.cpu().numpy() for t in ops.polygonize_counted(cls, 0, 1, val)])
    expected = [p for r0, c0 in stamps for p in polygon_list(small, r0, c0)]
    expected.sort(key=lambda p: (p[0], first_pixel(p, BIG_W)))
    assert max(first_pixel(p, BIG_W) for p in expected) >= 1 << 29
    assert len(got) == len(expected) == 3 * len(small[0])
    assert got == expected


def test_edge_count_beyond_the_limit_is_refused(cuda):
    from flairhip import lib as L, ops
    rows = (torch.arange(BIG_H, device=cuda) & 1).to(torch.uint8)
    cols = (torch.arange(BIG_W, device=cuda) & 1).to(torch.uint8)
    cls = rows[:, None] ^ cols[None, :]  # (row + col) & 1: every pixel its own component, E = 4 N > 2^31
    E = 4 * BIG_H * BIG_W
    assert E > 1 << 31
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match=str(E)):
        ops.polygonize_counted(cls)
    # the trace workspace for E edges would be about 90 GB; only the pixel workspace (and nothing E-sized) was taken
    assert torch.cuda.max_memory_allocated() - before <= L.load().ffa_polygonize_count_bytes(BIG_H, BIG_W) + (64 << 20)


def test_raster_to_polygons_workspace_counted_equals_the_default(cuda):
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    g = np.random.default_rng(17)
    cls = np.repeat(np.repeat(g.integers(0, 6, (60, 82)), 5, 0), 5, 1).astype(np.uint8)
    cls[cls == 5] = 18
    conf = g.integers(0, 256, cls.shape).astype(np.uint8)
    ras = ArrayRaster(cls, 651992.36, 6860417.84, 0.2)
    cras = ArrayRaster(conf, 651992.36, 6860417.84, 0.2)
    assert cls.shape == (300, 410)
    dflt = raster_to_polygons(ras, confidence=cras)
    counted = raster_to_polygons(ras, confidence=cras, workspace="counted")
    assert len(dflt) > 0 and _eq_frames(dflt, counted)
    assert list(dflt["pixels"]) == list(counted["pixels"])
    assert np.array_equal(np.asarray(dflt["confidence"]), np.asarray(counted["confidence"]))
    assert _eq_frames(dflt, raster_to_polygons(ras, confidence=cras, workspace="bound"))
    with pytest.raises(ValueError):
        raster_to_polygons(ras, workspace="tiled")
