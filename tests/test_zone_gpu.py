"""Geozone clipping on the GPU (csrc/zone_mask.hip through ops.rasterize_zone / zone_clip_ / zone_window_counts,
raster_to_polygons(zone=, classes=), run_inference with skip_tiles_outside_zone, the --zone / --classes options).

The oracle is ``oracle_mask`` below: the definition of include/flairhip.h restated in numpy, operation for operation
(float64, every operation rounded separately).  It agrees with matplotlib.path.Path.contains_points on the pixel
centres for the star and the random polygons (0 mismatching pixels), so every comparison with the kernel is ``==`` on
every pixel.
"""
import copy
import json
import logging
import os
import re
import sqlite3

import numpy as np
import pytest
import torch

from helpers import MOD, ROOT, TASK, oracle_to_product_keys

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
H0, W0 = 97, 131  # W is no multiple of 32: 5 words per row, the last one partial


def oracle_mask(rings, H, W):
    tog = np.zeros((H, W + 1), dtype=bool)
    rows = np.arange(H)
    yc = rows + 0.5
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        for (x0, y0), (x1, y1) in zip(ring, np.roll(ring, -1, axis=0)):
            if y0 == y1:
                continue
            cross = (y0 <= yc) != (y1 <= yc)
            xc = x0 + ((yc[cross] - y0) * (x1 - x0)) / (y1 - y0)
            c0 = np.clip(np.floor(xc - 0.5) + 1, 0, W).astype(np.int64)
            np.logical_xor.at(tog, (rows[cross], c0), True)  # a toggle at column W falls off the mask
    return np.logical_xor.accumulate(tog[:, :W], axis=1).astype(np.uint8)


def star(cx, cy, radii, points, phase=0.0):
    """2 * points vertices, radii alternating from radii[0], vertex k at the angle phase + k pi / points from +y"""
    k = np.arange(2 * points)
    ang = phase + np.pi * k / points
    rad = np.where(k % 2 == 0, radii[0], radii[1])
    return np.stack([cx + rad * np.sin(ang), cy + rad * np.cos(ang)], axis=1)


STAR = star(63.3, 47.7, (22.0, 70.0), 7, 0.1)   # sticks out of the 97 x 131 raster on all four sides
STAR_HOLE = star(60.2, 50.1, (12.0, 5.0), 5)
CENTRE_BOX = np.array([[10.5, 20.5], [30.5, 20.5], [30.5, 40.5], [10.5, 40.5]])


def random_polygons():
    g = np.random.default_rng(0)
    out = []
    for _ in range(20):
        n = int(g.integers(3, 40))
        cx, cy = g.uniform(20, 110), g.uniform(20, 80)
        ang = np.sort(g.uniform(0, 2 * np.pi, n))
        rad = g.uniform(5, 80, n)
        out.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))
    return out


def flat(rings):
    rings = [np.asarray(r, dtype=np.float64) for r in rings]
    return np.concatenate(rings), np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)


def gpu_mask(rings, H, W, **kw):
    from flairhip import ops
    xy, offsets = flat(rings)
    out = ops.rasterize_zone(xy, offsets, H, W, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def matplotlib_mask(ring, H, W):
    from matplotlib.path import Path
    yy, xx = np.mgrid[0:H, 0:W]
    pts = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], axis=1)
    return Path(np.vstack([ring, ring[:1]])).contains_points(pts).reshape(H, W)


@pytest.fixture(scope="module")
def star_mask():
    m = oracle_mask([STAR, STAR_HOLE], H0, W0)
    m.setflags(write=False)
    return m


# ---- 1. mask against the oracle, exact ---------------------------------------------------------------------------------

def test_star_with_a_hole(cuda, star_mask):
    assert int(star_mask.sum()) == 4319 and star_mask.size == 12707
    assert star_mask[0].any() and star_mask[-1].any() and star_mask[:, 0].any() and star_mask[:, -1].any()
    got = gpu_mask([STAR, STAR_HOLE], H0, W0)
    assert got.dtype == np.uint8 and got.shape == (H0, W0)
    assert np.array_equal(got, star_mask)
    # orientation does not matter, closed rings (repeated first vertex) neither
    assert np.array_equal(gpu_mask([STAR[::-1], np.vstack([STAR_HOLE, STAR_HOLE[:1]])], H0, W0), star_mask)


def test_random_radial_polygons(cuda):
    for k, ring in enumerate(random_polygons()):
        want = oracle_mask([ring], H0, W0)
        assert np.array_equal(gpu_mask([ring], H0, W0), want), k


def test_matplotlib_agrees_where_it_is_installed(cuda):
    pytest.importorskip("matplotlib")
    star_only = gpu_mask([STAR], H0, W0)
    assert int((star_only.astype(bool) != matplotlib_mask(STAR, H0, W0)).sum()) == 0
    for k, ring in enumerate(random_polygons()):
        got = gpu_mask([ring], H0, W0).astype(bool)
        assert int((got != matplotlib_mask(ring, H0, W0)).sum()) == 0, k


def test_box_with_corners_on_pixel_centres(cuda):
    got = gpu_mask([CENTRE_BOX], H0, W0)
    want = np.zeros((H0, W0), np.uint8)
    want[20:40, 11:31] = 1
    assert int(got.sum()) == 400 and np.array_equal(got, want)
    assert np.array_equal(oracle_mask([CENTRE_BOX], H0, W0), want)


def test_horizontal_edges_and_repeated_vertices(cuda):
    ring = np.array([[5.0, 5.0], [5.0, 5.0], [60.0, 5.0], [60.0, 5.0], [60.0, 30.5], [90.25, 30.5], [90.25, 30.5],
                     [90.25, 70.0], [40.0, 70.0], [40.0, 50.5], [5.0, 50.5], [5.0, 5.0], [5.0, 5.0]])
    want = oracle_mask([ring], H0, W0)
    assert want.any()
    assert np.array_equal(gpu_mask([ring], H0, W0), want)


def test_ring_outside_the_raster(cuda):
    for ring in (CENTRE_BOX + [500.0, 0.0], CENTRE_BOX - [0.0, 300.0], CENTRE_BOX + [-200.0, 400.0]):
        assert not oracle_mask([ring], H0, W0).any()
        assert not gpu_mask([ring], H0, W0).any()
    from flairhip import ops
    assert not ops.rasterize_zone(np.zeros((0, 2)), [0], H0, W0).any()  # no ring at all


# ---- 2. wide and tiny rasters ------------------------------------------------------------------------------------------

def test_wide_rows_carry_between_waves(cuda):
    H, W = 3, 2113  # 67 words per row: more than the 64 one wave scans at a time
    tri = np.array([[-3.0, -1.0], [2125.0, -1.0], [2110.7, 4.0]])
    want = oracle_mask([tri], H, W)
    assert want[:, :64 * 32].any() and want[:, 64 * 32:].any()
    assert np.array_equal(gpu_mask([tri], H, W), want)
    # a toggle in the last bit of word 63 and one far right: the inside run crosses the wave boundary
    slab = np.array([[2047.2, -1.0], [2100.4, -1.0], [2100.4, 5.0], [2047.2, 5.0]])
    assert np.array_equal(gpu_mask([slab, tri], H, W), oracle_mask([slab, tri], H, W))


@pytest.mark.parametrize("H,W", [(1, 1), (1, 33), (64, 1)])
def test_degenerate_shapes(cuda, H, W):
    big = np.array([[-1.0, -1.0], [W + 1.0, -1.0], [W + 1.0, H + 1.0], [-1.0, H + 1.0]])
    assert gpu_mask([big], H, W).all()
    part = np.array([[0.2, 0.1], [W * 0.7 + 0.4, 0.1], [W * 0.7 + 0.4, H * 0.6 + 0.45], [0.2, H * 0.6 + 0.45]])
    assert np.array_equal(gpu_mask([part], H, W), oracle_mask([part], H, W))
    assert np.array_equal(gpu_mask([big, part], H, W), oracle_mask([big, part], H, W))


# ---- 3. accumulate -----------------------------------------------------------------------------------------------------

def test_accumulate_is_the_union_and_one_call_the_xor(cuda):
    from flairhip import ops
    a = np.array([[10.2, 10.7], [70.9, 10.7], [70.9, 60.1], [10.2, 60.1]])
    b = np.array([[40.4, 30.3], [120.6, 30.3], [120.6, 90.8], [40.4, 90.8]])
    ma, mb = oracle_mask([a], H0, W0), oracle_mask([b], H0, W0)
    assert (ma & mb).any()
    m = ops.rasterize_zone(*flat([a]), H0, W0)
    m2 = ops.rasterize_zone(*flat([b]), H0, W0, out=m, accumulate=True)
    assert m2 is m
    assert np.array_equal(m.cpu().numpy(), ma | mb)
    both = gpu_mask([a, b], H0, W0)
    assert np.array_equal(both, ma ^ mb) and np.array_equal(both, oracle_mask([a, b], H0, W0))
    # a mask view that is not 16-byte aligned takes the same values
    buf = torch.zeros(H0 * W0 + 16, dtype=torch.uint8, device=cuda)
    view = buf[3:3 + H0 * W0].view(H0, W0)
    ops.rasterize_zone(*flat([a]), H0, W0, out=view)
    ops.rasterize_zone(*flat([b]), H0, W0, out=view, accumulate=True)
    assert np.array_equal(view.cpu().numpy(), ma | mb)
    assert not buf[:3].any() and not buf[3 + H0 * W0:].any()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------

def test_equal_bytes_whatever_the_workspace_held(cuda, star_mask):
    from flairhip import ops
    xy, offsets = flat([STAR, STAR_HOLE])
    outs = []
    for garbage in (0xFF, 0x5A):
        ops.workspace(1, cuda, ops.ZONE_WORKSPACE_SLOT).fill_(garbage)
        out = torch.full((H0, W0), 7, dtype=torch.uint8, device=cuda)
        ops.rasterize_zone(xy, offsets, H0, W0, out=out)
        outs.append(out.cpu().numpy().tobytes())
    assert outs[0] == outs[1] == star_mask.tobytes()


# ---- 5. clip -----------------------------------------------------------------------------------------------------------

def test_clip_equals_numpy_where(cuda, star_mask):
    from flairhip import ops
    g = np.random.default_rng(5)
    cls = g.integers(0, 9, (H0, W0)).astype(np.uint8)
    cls[g.random((H0, W0)) < 0.01] = 255
    mask = torch.from_numpy(star_mask.copy()).to(cuda)
    keep = np.isin(cls, [3, 6])

    def run(m, k, fill):
        t = torch.from_numpy(cls).to(cuda)
        assert ops.zone_clip_(t, m, keep_classes=k, fill=fill) is t
        return t.cpu().numpy()

    assert np.array_equal(run(mask, [3, 6], 18), np.where((star_mask == 1) & keep, cls, 18))
    assert np.array_equal(run(mask, None, 200), np.where(star_mask == 1, cls, 200))
    assert np.array_equal(run(None, [3, 6], 0), np.where(keep, cls, 0))
    assert np.array_equal(run(None, None, 9), cls)
    assert np.array_equal(run(mask, [], 4), np.full_like(cls, 4))
    # misaligned views of both operands
    cbuf = torch.zeros(H0 * W0 + 32, dtype=torch.uint8, device=cuda)
    cview = cbuf[5:5 + H0 * W0].view(H0, W0)
    cview.copy_(torch.from_numpy(cls))
    mbuf = torch.zeros(H0 * W0 + 32, dtype=torch.uint8, device=cuda)
    mview = mbuf[2:2 + H0 * W0].view(H0, W0)
    mview.copy_(mask)
    ops.zone_clip_(cview, mview, keep_classes=[3, 6], fill=18)
    assert np.array_equal(cview.cpu().numpy(), np.where((star_mask == 1) & keep, cls, 18))
    assert not cbuf[:5].any() and not cbuf[5 + H0 * W0:].any()
    with pytest.raises(ValueError):
        ops.zone_clip_(torch.from_numpy(cls).to(cuda), None, fill=256)
    with pytest.raises(ValueError):
        ops.zone_clip_(torch.from_numpy(cls).to(cuda), None, keep_classes=[300])


# ---- 6. window counts --------------------------------------------------------------------------------------------------

def test_window_counts_are_exact(cuda, star_mask):
    from flairhip import ops
    g = np.random.default_rng(6)
    r = np.sort(g.integers(-20, H0 + 20, (50, 2)), axis=1)
    c = np.sort(g.integers(-20, W0 + 20, (50, 2)), axis=1)
    win = np.stack([r[:, 0], c[:, 0], r[:, 1], c[:, 1]], axis=1)
    win[0] = (0, 0, H0, W0)           # everything
    win[1] = (-5, -7, H0 + 9, W0 + 3)  # everything, past every border
    win[2] = (40, 60, 40, 90)         # no rows
    win[3] = (50, 70, 30, 90)         # inverted
    win[4] = (H0 + 2, 0, H0 + 9, W0)  # wholly outside
    want = [int(star_mask[max(r0, 0):max(r1, 0), max(c0, 0):max(c1, 0)].sum()) for r0, c0, r1, c1 in win]
    assert want[0] == want[1] == 4319 and want[2] == want[3] == want[4] == 0 and sum(w > 0 for w in want) > 20
    got = ops.zone_window_counts(torch.from_numpy(star_mask.copy()).to(cuda), win)
    assert got.dtype == torch.int64 and got.cpu().tolist() == want
    assert ops.zone_window_counts(torch.from_numpy(star_mask.copy()).to(cuda), np.zeros((0, 4), np.int32)).numel() == 0


# ---- 7. raster_to_polygons with a zone ---------------------------------------------------------------------------------

RH, RW, RES, LEFT, TOP = 96, 128, 0.2, 651992.4, 6860417.8


def class_raster():
    g = np.random.default_rng(7)
    seeds = g.integers(0, 8, (RH // 8 + 1, RW // 8 + 1))
    cls = np.repeat(np.repeat(seeds, 8, 0), 8, 1)[:RH, :RW]
    return np.where(g.random((RH, RW)) < 0.05, g.integers(0, 8, (RH, RW)), cls).astype(np.uint8)


def zone_pixels():
    return [star(60.3, 45.7, (20.0, 66.0), 7, 0.1), star(58.2, 47.1, (11.0, 5.0), 5)]


def to_map(ring):
    return np.stack([LEFT + ring[:, 0] * RES, TOP - ring[:, 1] * RES], axis=1)


def zone_geojson():
    return {"type": "Feature", "properties": {}, "geometry": {
        "type": "Polygon", "coordinates": [np.vstack([to_map(r), to_map(r)[:1]]).tolist() for r in zone_pixels()]}}


def map_zone_mask():
    """the oracle on the pixel coordinates zone.zone_mask derives from the map coordinates (same two numpy lines)"""
    rings = []
    for r in zone_pixels():
        m = to_map(r)
        rings.append(np.stack([(m[:, 0] - LEFT) / RES, (TOP - m[:, 1]) / RES], axis=1))
    return oracle_mask(rings, RH, RW)


def frames_equal(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for col in a.columns:
        if col == "geometry":
            for ga, gb in zip(a[col], b[col]):
                ra, rb = [ga.exterior] + list(ga.interiors), [gb.exterior] + list(gb.interiors)
                assert len(ra) == len(rb) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ra, rb))
        else:
            assert a[col].to_numpy().tobytes() == b[col].to_numpy().tobytes(), col
    return True


@pytest.mark.parametrize("classes", [None, [2, 5, 6]], ids=["all-classes", "three-classes"])
def test_raster_to_polygons_with_a_zone_equals_the_premasked_raster(cuda, classes):
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls = class_raster()
    conf = np.random.default_rng(8).integers(0, 256, (RH, RW)).astype(np.uint8)
    mask = map_zone_mask()
    assert 0.2 < mask.mean() < 0.7
    inside = (mask == 1) if classes is None else (mask == 1) & np.isin(cls, classes)
    pre = np.where(inside, cls, 7).astype(np.uint8)
    ras = ArrayRaster(cls[None], LEFT, TOP, RES)
    ras_pre = ArrayRaster(pre[None], LEFT, TOP, RES)
    cras = ArrayRaster(conf[None], LEFT, TOP, RES)
    kw = dict(background_value=7, min_area=0.0, simplification=0.0)
    got = raster_to_polygons(ras, zone=zone_geojson(), classes=classes, confidence=cras, **kw)
    want = raster_to_polygons(ras_pre, confidence=cras, **kw)
    assert len(want) > 10 and frames_equal(got, want)
    assert list(got.columns) == ["class_id", "confidence", "pixels", "geometry"]
    assert int(got["pixels"].sum()) == int((inside & (cls != 7)).sum())
    if classes is not None:
        assert set(got["class_id"]) <= set(classes)
    # without the confidence columns, and with the defaults (min_area, simplification) as well
    assert frames_equal(raster_to_polygons(ras, zone=zone_geojson(), classes=classes, background_value=7),
                        raster_to_polygons(ras_pre, background_value=7))
    # the input raster is not modified
    assert np.array_equal(ras.data[0], cls)


def test_raster_to_polygons_without_zone_and_classes_is_unchanged(cuda):
    from flair_zonal_detection.inference import min_pixels_for_area, raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    from flairhip import ops
    cls = class_raster()
    ras = ArrayRaster(cls[None], LEFT, TOP, RES)
    got = raster_to_polygons(ras, background_value=7, zone=None, classes=None)
    # today's output: ops.polygonize of the raster itself, (class, first pixel) order, map coordinates, simplified
    want_classes = ops.polygonize(torch.from_numpy(cls).to(cuda), 7, min_pixels_for_area(1.0, RES * RES))[0].cpu().numpy()
    assert got["class_id"].tolist() == want_classes.tolist() and len(got) > 5
    assert frames_equal(got, raster_to_polygons(ras, background_value=7))
    # a zone that covers everything and every class changes nothing either
    everything = (LEFT - 10.0, TOP - RH * RES - 10.0, LEFT + RW * RES + 10.0, TOP + 10.0)
    assert frames_equal(got, raster_to_polygons(ras, background_value=7, zone=everything, classes=range(256)))


def test_no_background_uses_255_and_refuses_rasters_that_hold_it(cuda):
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls = class_raster()
    mask = map_zone_mask()
    ras = ArrayRaster(cls[None], LEFT, TOP, RES)
    kw = dict(ignore_background=False, min_area=0.0, simplification=0.0)
    got = raster_to_polygons(ras, zone=zone_geojson(), **kw)
    want = raster_to_polygons(ArrayRaster(np.where(mask == 1, cls, 255).astype(np.uint8)[None], LEFT, TOP, RES),
                              background_value=255, min_area=0.0, simplification=0.0)
    assert frames_equal(got, want) and set(got["class_id"]) == set(np.unique(cls[mask == 1]).tolist())
    bad = cls.copy()
    bad[3, 4] = 255
    bras = ArrayRaster(bad[None], LEFT, TOP, RES)
    with pytest.raises(ValueError, match="255"):
        raster_to_polygons(bras, zone=zone_geojson(), **kw)
    with pytest.raises(ValueError, match="255"):
        raster_to_polygons(bras, classes=[3, 255], **kw)
    assert len(raster_to_polygons(bras, classes=[3, 6], **kw))  # 255 is not a kept class: fine


# ---- 8. / 9. tile skipping end to end, CLI -----------------------------------------------------------------------------

ZH, ZW = 200, 260


def l_zone(ras):
    """an L along the left and bottom sides of the raster, about a third of it, reaching past its borders"""
    b = ras.bounds
    x0, x1, x2 = b.left - 3.0, b.left + 50.3 * 0.2, b.right + 3.0
    y0, y1, y2 = b.bottom - 3.0, b.bottom + 40.6 * 0.2, b.top + 3.0
    ring = [[x0, y0], [x2, y0], [x2, y1], [x1, y1], [x1, y2], [x0, y2], [x0, y0]]
    return {"type": "Polygon", "coordinates": [ring]}


@pytest.fixture(scope="module")
def zonal(tmp_path_factory):
    """the smallest multi-tile configuration of tests/test_zonal_gpu.py: 200 x 260 pixels of 0.2 m, 128-pixel tiles
    with a 16-pixel margin, bf16, hip_graph as it defaults"""
    import yaml
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    tmp = tmp_path_factory.mktemp("zone")
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(1, 255, (3, ZH, ZW)).astype(np.uint8), 651992.4, 6860417.8, 0.2)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": 0.2, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    oracle = UnetResNet34(3, 19)
    sd = fill_state_dict(oracle.state_dict(), seed=5)
    sd["segmentation_head.0.bias"] = sd["segmentation_head.0.bias"] + torch.linspace(0, 3, 19)  # class 0 = never written
    oracle.load_state_dict(sd)
    cfg["model_weights"] = str(tmp / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    return cfg, ras, l_zone(ras), tmp


def raster_zone_mask(ras, zone):
    b = ras.bounds
    ring = np.asarray(zone["coordinates"][0], dtype=np.float64)
    pix = np.stack([(ring[:, 0] - float(b.left)) / 0.2, (float(b.top) - ring[:, 1]) / 0.2], axis=1)
    return oracle_mask([pix], ZH, ZW)


def test_tiles_outside_the_zone_are_skipped_and_the_zone_is_unchanged(cuda, zonal, caplog):
    from flair_zonal_detection.inference import prep_config, raster_to_polygons, run_inference
    from flair_zonal_detection.slicing import generate_patches_from_reference
    cfg, ras, zone, _ = zonal
    mask = raster_zone_mask(ras, zone)
    assert 0.25 < mask.mean() < 0.45

    # expected: the kept bounds of every tile as a pixel rectangle, snapped outward, one pixel larger on every side
    tiles = generate_patches_from_reference(prep_config(copy.deepcopy(cfg)), ras, zone)
    b = ras.bounds
    sums = []
    for t in tiles.itertuples():
        r0 = max(int(np.floor((b.top - t.top) / 0.2)) - 1, 0)
        r1 = min(int(np.ceil((b.top - t.bottom) / 0.2)) + 1, ZH)
        c0 = max(int(np.floor((t.left - b.left) / 0.2)) - 1, 0)
        c1 = min(int(np.ceil((t.right - b.left) / 0.2)) + 1, ZW)
        sums.append(int(mask[r0:r1, c0:c1].sum()))
    n, k = len(sums), sum(s == 0 for s in sums)
    # 3 x 3 tiles: origins -16, 80 and a last one clamped to the raster's end (row 89, column 148) on a 96-pixel stride
    assert n == 9 and 0 < k < n

    skip_cfg = copy.deepcopy(cfg)
    skip_cfg["skip_tiles_outside_zone"] = True
    with caplog.at_level(logging.INFO, logger="flair_zonal_detection.inference"):
        skipped = run_inference(skip_cfg, geozone=zone)
    logged = [re.search(r"(\d+) of (\d+) tiles outside the zone skipped", r.getMessage()) for r in caplog.records]
    logged = [m for m in logged if m]
    assert len(logged) == 1 and (int(logged[0].group(1)), int(logged[0].group(2))) == (k, n)

    off_cfg = copy.deepcopy(cfg)
    off_cfg["skip_tiles_outside_zone"] = False
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="flair_zonal_detection.inference"):
        full = run_inference(off_cfg, geozone=zone)
        plain = run_inference(copy.deepcopy(cfg), geozone=zone)  # the key absent
    assert not any("tiles outside the zone" in r.getMessage() for r in caplog.records)
    a, f = skipped[TASK].data, full[TASK].data
    assert f.all() and not a.all()                     # the skipped tiles left never-written zeros behind
    assert a[0][mask == 1].all()
    assert np.array_equal(a[0][mask == 1], f[0][mask == 1])
    assert plain[TASK].data.tobytes() == f.tobytes()
    assert frames_equal(raster_to_polygons(skipped, zone=zone), raster_to_polygons(full, zone=zone))


def test_cli_zone_and_classes(cuda, zonal, tmp_path):
    import yaml
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.inference import raster_to_polygons, run_inference
    from flair_zonal_detection.main import main
    cfg, ras, zone, _ = zonal
    src = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src, ras, 3) as w:
        w.data[...] = ras.data
    zpath = str(tmp_path / "zone.geojson")
    with open(zpath, "w") as f:
        json.dump({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {}, "geometry": zone}]}, f)
    fcfg = copy.deepcopy(cfg)
    fcfg["modalities"][MOD]["input_img_path"] = src
    fcfg["output_path"] = str(tmp_path / "out")
    fcfg["skip_tiles_outside_zone"] = True
    ypath = str(tmp_path / "zonal.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(fcfg, f)
    # the classes the in-memory run finds most often inside the zone
    mem = run_inference(copy.deepcopy(cfg), geozone=zone)
    mask = raster_zone_mask(ras, zone)
    top = np.argsort(np.bincount(mem[TASK].data[0][mask == 1], minlength=19))[-3:].tolist()
    want = raster_to_polygons(mem, zone=zone, classes=top)
    assert len(want) > 0
    gpkg = str(tmp_path / "polygons.gpkg")
    main(["--config", ypath, "--zone", zpath, "--polygons", gpkg, "--classes", ",".join(str(c) for c in top)])
    con = sqlite3.connect(gpkg)
    try:
        table = con.execute("SELECT table_name FROM gpkg_contents").fetchone()[0]
        rows = con.execute(f'SELECT class_id FROM "{table}"').fetchall()
    finally:
        con.close()
    assert len(rows) == len(want) and sorted(r[0] for r in rows) == sorted(want["class_id"].tolist())
