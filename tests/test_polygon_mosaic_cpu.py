"""Host side of the full-size polygoniser: the mosaic grid arithmetic and the validation of rasters_to_polygons (both
run before anything touches a device), and the workspace size functions of the count-sized path, which are host
arithmetic."""

import numpy as np
import pytest

RES, LEFT, TOP = 0.2, 651992.36, 6860417.84


def bounds(r0, c0, h, w, res=RES):
    return (LEFT + c0 * res, TOP - (r0 + h) * res, LEFT + (c0 + w) * res, TOP - r0 * res)


WINS = [(0, 0, 41, 67), (0, 67, 41, 63), (41, 0, 55, 67), (41, 67, 55, 63)]


def test_mosaic_grid_aligned_and_shuffled():
    from flair_zonal_detection.inference import mosaic_grid
    H, W, left, top, wins = mosaic_grid([bounds(*w) for w in WINS], (RES, RES))
    assert (H, W, left, top) == (96, 130, LEFT, TOP) and wins == WINS
    order = [3, 0, 2, 1]
    H, W, left, top, wins = mosaic_grid([bounds(*WINS[i]) for i in order], (RES, RES))
    # the origin is the leftmost source's left and the topmost source's top themselves, bit for bit
    assert (H, W, left, top) == (96, 130, LEFT, TOP) and wins == [WINS[i] for i in order]
    # a gap: the union's bounding box, the windows inside it
    H, W, left, top, wins = mosaic_grid([bounds(*WINS[3]), bounds(*WINS[0])], (RES, RES))
    assert (H, W, left, top) == (96, 130, LEFT, TOP) and wins == [WINS[3], WINS[0]]
    # one source, non-square pixels
    assert mosaic_grid([(10.0, 0.0, 20.0, 6.0)], (0.5, 2.0)) == (3, 20, 10.0, 6.0, [(0, 0, 3, 20)])


def test_mosaic_grid_refuses_what_is_no_common_grid():
    from flair_zonal_detection.inference import mosaic_grid
    a = bounds(*WINS[0])
    with pytest.raises(ValueError, match="tile_b"):  # half a pixel to the right
        mosaic_grid([a, tuple(v + d for v, d in zip(bounds(*WINS[1]), (0.1, 0, 0.1, 0)))], (RES, RES),
                    names=["tile_a", "tile_b"])
    with pytest.raises(ValueError, match="tile_b"):  # half a pixel down
        mosaic_grid([a, tuple(v + d for v, d in zip(bounds(*WINS[2]), (0, 0.1, 0, 0.1)))], (RES, RES),
                    names=["tile_a", "tile_b"])
    with pytest.raises(ValueError, match="share pixels"):  # one column of overlap
        mosaic_grid([a, bounds(0, 66, 41, 64)], (RES, RES))
    with pytest.raises(ValueError, match="share pixels"):
        mosaic_grid([bounds(*w) for w in WINS] + [bounds(50, 70, 2, 2)], (RES, RES))
    mosaic_grid([a, bounds(0, 67 + 1e-7, 41, 63)], (RES, RES))  # within 1e-6 of a pixel
    with pytest.raises(ValueError, match="2\\^30"):
        mosaic_grid([(0.0, 0.0, 32768.0, 16384.0), (0.0, 16384.0, 32768.0, 32768.0)], (1.0, 1.0))
    with pytest.raises(ValueError):
        mosaic_grid([], (RES, RES))


def rasters(**kw):
    from flair_zonal_detection.raster import ArrayRaster
    res = kw.pop("res", RES)
    return [ArrayRaster(np.full((h, w), 3, np.uint8), LEFT + c0 * RES, TOP - r0 * RES, res, **kw) for r0, c0, h, w in WINS]


def test_rasters_to_polygons_validates_before_any_device_work():
    from flair_zonal_detection.inference import rasters_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    good = rasters()
    with pytest.raises(ValueError, match="source 1.*resolution"):
        rasters_to_polygons([good[0], rasters(res=0.25)[1]] + good[2:])
    with pytest.raises(ValueError, match="source 2.*CRS"):
        rasters_to_polygons(good[:2] + [rasters(crs="EPSG:32631")[2]] + good[3:])
    with pytest.raises(ValueError, match="source 1"):  # half-pixel offset
        rasters_to_polygons([good[0], ArrayRaster(np.zeros((41, 63), np.uint8), LEFT + 67.5 * RES, TOP, RES)])
    with pytest.raises(ValueError, match="share pixels"):
        rasters_to_polygons([good[0], ArrayRaster(np.zeros((41, 63), np.uint8), LEFT + 66 * RES, TOP, RES)])
    with pytest.raises(ValueError, match="ignore_background"):  # a gap cannot be filled when every value is a class
        rasters_to_polygons(good[:3], ignore_background=False)
    with pytest.raises(ValueError, match="source 0.*one-band"):
        rasters_to_polygons([ArrayRaster(np.zeros((3, 41, 67), np.uint8), LEFT, TOP, RES)])
    with pytest.raises(ValueError, match="confidence"):
        rasters_to_polygons(good, confidence=good[:2])
    with pytest.raises(ValueError):
        rasters_to_polygons([])


# ---- workspace sizes of the count-sized path (include/flairhip.h) -----------------------------------------------------

PIXEL_CONSTANT = 2 << 20   # ffa_polygonize_count_bytes(H, W) <= 16 H W + 2 MiB
TRACE_CONSTANT = 64 << 10  # ffa_polygonize_trace_bytes(E, P) <= 48 E + 64 P + 64 KiB


def test_count_bytes_is_sixteen_bytes_per_pixel(lib):
    for H, W in [(1, 1), (33, 65), (5000, 5000), (16385, 32768), (25000, 25000), (32767, 32768)]:
        n = lib.ffa_polygonize_count_bytes(H, W)
        assert 16 * H * W <= n <= 16 * H * W + PIXEL_CONSTANT, (H, W, n)
    assert lib.ffa_polygonize_count_bytes(32768, 32768) < 0  # H * W = 2^30
    assert b"2^30" in lib.ffa_last_error()
    assert lib.ffa_polygonize_count_bytes(0, 5) < 0
    # the bound-sized workspace keeps its bytes and its limit
    assert lib.ffa_polygonize_workspace_bytes(16384, 32768) < 0
    n = lib.ffa_polygonize_workspace_bytes(5000, 5000)
    assert 184 * 5000 * 5000 <= n <= 185 * 5000 * 5000


def test_trace_bytes_depends_on_the_counts_alone(lib):
    for E, P in [(4, 1), (4096, 1024), (1_000_003, 17), (130_000_000, 5_000_000), ((1 << 31) - 2, 1 << 29)]:
        n = lib.ffa_polygonize_trace_bytes(E, P)
        assert 28 * E <= n <= 48 * E + 64 * P + TRACE_CONSTANT, (E, P, n)
    # monotone in both, and no raster size enters the signature at all
    assert lib.ffa_polygonize_trace_bytes(1000, 10) <= lib.ffa_polygonize_trace_bytes(2000, 10)
    assert lib.ffa_polygonize_trace_bytes(1000, 10) <= lib.ffa_polygonize_trace_bytes(1000, 5000)
    assert lib.ffa_polygonize_trace_bytes(0, 0) <= TRACE_CONSTANT
    assert lib.ffa_polygonize_trace_bytes((1 << 31) - 1, 1) < 0
    assert str((1 << 31) - 1).encode() in lib.ffa_last_error()
    assert lib.ffa_polygonize_trace_bytes(-1, 0) < 0


def test_workspace_bytes_are_pinned(lib):
    """The exact answers of the four size functions: integrators allocate by them, and a workspace that shrinks under
    a caller's buffer is not caught by the bounds above.  Numbers from the library built at e65cbdf."""
    rasters = [(1, 1), (1, 70), (33, 65), (700, 900), (5000, 5000), (23170, 23170)]
    assert [lib.ffa_polygonize_workspace_bytes(H, W) for H, W in rasters] == [
        7936, 19712, 400384, 116084480, 4606381056, 98917070336]
    assert [lib.ffa_sieve_workspace_bytes(H, W) for H, W in rasters] == [
        1024, 2048, 37120, 10710272, 425000192, 9126432256]
    assert [lib.ffa_polygonize_count_bytes(H, W) for H, W in rasters + [(25000, 25000), (32768, 32767)]] == [
        1536, 2560, 35328, 10081280, 400025856, 8590108160, 10000611840, 17180395008]
    counts = [(0, 0), (4, 1), (4096, 1024), (1_000_003, 17), (130_000_000, 5_000_000), ((1 << 31) - 2, 1 << 29)]
    assert [lib.ffa_polygonize_trace_bytes(E, P) for E, P in counts] == [
        6656, 6656, 178688, 42069248, 5468258304, 90330663168]


def test_a_full_dalle_fits_sixteen_gib(lib):
    """25 000 x 25 000 pixels at the 0.2 boundary edges per pixel of real land-cover maps"""
    total = lib.ffa_polygonize_count_bytes(25000, 25000) + lib.ffa_polygonize_trace_bytes(130_000_000, 5_000_000)
    assert total < 16 << 30, total
