"""Zonal statistics on the GPU (csrc/zone_stats.hip through ops.zone_class_stats, zonal_stats.zonal_class_stats, the
--zone-stats option).

The oracle is tests/zone_stats_oracle.py: the inside mask of include/flairhip.h restated in numpy (``oracle_mask`` as
tests/test_zone_gpu.py writes it), applied zone by zone, then np.bincount with the values >= K folded into column K, and
the same with the confidence bytes as int64 weights.  Every result is an integer and every comparison is ``==``; the
only ratios are the confidence columns of the host table, float64 quotients of exact integers compared with ``==`` to
the same numpy expression.
"""
import copy
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

from helpers import MOD, ROOT, TASK, oracle_to_product_keys
from zone_stats_oracle import (CENTRE_BOX, H0, STAR, STAR_HOLE, W0, base_rasters, oracle_mask, oracle_masks,
                               oracle_stats, parcel_grid, random_polygons, window_rule)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
K0 = 19


def gpu_stats(cls, zones, K, conf=None, **kw):
    """(counts, conf_sums) of ops.zone_class_stats as numpy arrays"""
    from flairhip import ops
    dev = torch.device("cuda")
    counts, sums = ops.zone_class_stats(torch.tensor(cls, device=dev), zones, K,
                                        conf=None if conf is None else torch.tensor(conf, device=dev), **kw)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(zones), K + 1) and counts.is_cuda
    if conf is None:
        assert sums is None
        return counts.cpu().numpy(), None
    assert sums.dtype == torch.int64 and sums.shape == counts.shape
    return counts.cpu().numpy(), sums.cpu().numpy()


def check(cls, conf, zones, K, **kw):
    """the GPU table of the zones equals the oracle's; returns (counts, sums, masks)"""
    masks = oracle_masks(zones, *cls.shape)
    want_c, want_s = oracle_stats(cls, conf, masks, K)
    got_c, got_s = gpu_stats(cls, zones, K, conf, **kw)
    assert np.array_equal(got_c, want_c)
    if conf is not None:
        assert np.array_equal(got_s, want_s)
    return got_c, got_s, masks


@pytest.fixture(scope="module")
def base():
    cls, conf = base_rasters()
    assert cls.shape == (H0, W0) and (cls == 255).sum() > 100 and cls[cls != 255].max() == 18
    cls.setflags(write=False)
    conf.setflags(write=False)
    return cls, conf


@pytest.fixture(scope="module")
def parcels(base):
    """the 24 x 24 parcel grid, its oracle masks and oracle table (computed once, read-only)"""
    cls, conf = base
    zones = parcel_grid()
    masks = oracle_masks(zones, H0, W0)
    counts, sums = oracle_stats(cls, conf, masks, K0)
    for a in (masks, counts, sums):
        a.setflags(write=False)
    return zones, masks, counts, sums


def mixed_zones():
    outside = CENTRE_BOX + [500.0, 0.0]
    larger = np.array([[-9.0, -7.0], [W0 + 8.0, -7.0], [W0 + 8.0, H0 + 6.0], [-9.0, H0 + 6.0]])
    return [[STAR, STAR_HOLE], [CENTRE_BOX], [outside], [larger], []] + [[p] for p in random_polygons()]


# ---- 1. mixed zones ----------------------------------------------------------------------------------------------------

def test_mixed_zones(cuda, base):
    from flairhip import ops
    cls, conf = base
    zones = mixed_zones()
    assert len(zones) == 25
    counts, sums, masks = check(cls, conf, zones, K0)
    assert counts[0].sum() == 4319 and counts[1].sum() == 400 and counts[2].sum() == 0  # star with hole, box, outside
    assert counts[3].sum() == H0 * W0 and counts[4].sum() == 0 and counts[:, K0].sum() > 0
    assert masks.sum(axis=0).max() > 5  # the zones overlap: a pixel counts in every zone that holds it
    # the member pixels of every zone are the mask of the existing kernel for that zone's rings in one call
    for z, rings in enumerate(zones):
        xy = np.concatenate(rings) if rings else np.zeros((0, 2))
        offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
        assert int(ops.rasterize_zone(xy, offsets, H0, W0).sum()) == int(counts[z].sum()), z
    # orientation and closedness do not matter
    flipped = [[np.vstack([r[::-1], r[::-1][:1]]) for r in rings] for rings in zones]
    assert np.array_equal(gpu_stats(cls, flipped, K0)[0], counts)


# ---- 2. parcel grid ----------------------------------------------------------------------------------------------------

def test_parcel_grid(cuda, base, parcels):
    cls, conf = base
    zones, masks, want_c, want_s = parcels
    # preconditions on the input: the masks tile the raster, 67 of the 576 parcels are empty, the windows lose nothing
    assert len(zones) == 576 and np.all(masks.sum(axis=0) == 1)
    assert int((masks.reshape(576, -1).sum(axis=1) == 0).sum()) == 67
    for rings, m in zip(zones, masks):
        r0, c0, r1, c1 = window_rule(rings, H0, W0)
        inside = np.zeros_like(m)
        inside[r0:r1, c0:c1] = True
        assert not (m & ~inside).any()
    got_c, got_s = gpu_stats(cls, zones, K0, conf)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_s, want_s)
    folded = np.minimum(cls.astype(np.int64), K0)
    assert np.array_equal(got_c.sum(axis=0), np.bincount(folded.ravel(), minlength=K0 + 1))
    assert np.array_equal(got_s.sum(axis=0), np.bincount(folded.ravel(), weights=conf.ravel().astype(np.int64),
                                                         minlength=K0 + 1).astype(np.int64))


# ---- 3. wide rows ------------------------------------------------------------------------------------------------------

def test_wide_rows_carry_and_a_one_word_window(cuda):
    from flairhip import ops
    H, W = 3, 4136  # 130 words per row, the last one partial: more than the 64 a wave scans at a time, twice over
    cls, conf = base_rasters(H, W, seed=12)
    xs = np.linspace(-3.0, W + 2.0, 41)
    top = np.stack([xs, np.where(np.arange(41) % 2 == 0, -1.0, 2.2)], axis=1)  # a zigzag through rows 0 and 1
    zigzag = np.vstack([top, [[W + 2.0, 4.0], [-3.0, 4.0]]])
    small = np.array([[2050.3, 0.2], [2069.6, 0.2], [2069.6, 2.7], [2050.3, 2.7]])
    assert window_rule([zigzag], H, W) == (0, 0, 3, W)
    assert window_rule([small], H, W) == (0, 2048, 3, 2071)  # one word per row
    m = oracle_mask([zigzag], H, W)
    assert m[:, :2048].any() and m[:, 2048:4096].any() and m[:, 4096:].any() and not m.all()
    check(cls, conf, [[zigzag]], K0)
    check(cls, conf, [[small]], K0)
    check(cls, conf, [[zigzag], [small], [zigzag, small]], K0)
    # an inside run that crosses both 64-word boundaries of the scan
    slab = np.array([[2047.2, -1.0], [4100.4, -1.0], [4100.4, 5.0], [2047.2, 5.0]])
    counts, _, _ = check(cls, conf, [[slab], [slab, zigzag]], K0)
    assert counts[0].sum() == 3 * (4100 - 2047)
    assert ops.ZONE_STATS_NARROW_WORDS < 64


# ---- 4. chunk boundary -------------------------------------------------------------------------------------------------

def test_a_zone_of_several_chunks(cuda):
    from flairhip import ops
    cap = ops.ZONE_STATS_CHUNK_WORDS
    side = 400
    if cap > 5000:  # size the raster from the constant: more than cap words in one window, at most 2 Mpx
        side = min(int(np.ceil(np.sqrt(32.0 * (cap + 1)))) + 32, 1414)
    cls, conf = base_rasters(side, side, seed=13)
    big = np.array([[7.3, 5.1], [side - 9.4, 11.6], [side - 3.2, side - 6.7], [side / 2.0, side - 60.2], [3.9, side - 8.8]])
    small = np.array([[40.2, 50.7], [71.9, 52.3], [60.4, 90.1]])
    win = ops.zone_stats_windows(*ops.zone_stats_flatten([[big], [small]]), side, side)
    words = ops.zone_stats_plane_words(win)[2]
    chunks = ops.zone_stats_plan(win)[3]
    assert words[0] > cap and words[0] % cap != 0 and 0 < words[1] < cap
    assert (chunks[:, 0] == 0).sum() == -(-words[0] // cap) >= 2 and (chunks[:, 0] == 1).sum() == 1
    counts, _, _ = check(cls, conf, [[big], [small]], K0)
    assert counts[0].sum() > 32 * cap // 2 and counts[1].sum() > 0


# ---- 5. degenerate shapes ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [1, 256])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 33), (64, 1)])
def test_degenerate_shapes(cuda, H, W, K):
    g = np.random.default_rng(H * 100 + W)
    cls = g.integers(0, 256, (H, W)).astype(np.uint8)
    conf = g.integers(0, 256, (H, W)).astype(np.uint8)
    big = np.array([[-1.0, -1.0], [W + 1.0, -1.0], [W + 1.0, H + 1.0], [-1.0, H + 1.0]])
    part = np.array([[0.2, 0.1], [W * 0.7 + 0.4, 0.1], [W * 0.7 + 0.4, H * 0.6 + 0.45], [0.2, H * 0.6 + 0.45]])
    counts, sums, _ = check(cls, conf, [[big], [part], [big, part], []], K)
    assert counts[0].sum() == H * W and sums[0].sum() == conf.astype(np.int64).sum()
    if K == 1:
        assert counts[0, 1] == (cls >= 1).sum()
    else:
        assert counts[:, 256].sum() == 0 and np.array_equal(counts[0, :256], np.bincount(cls.ravel(), minlength=256))
    # without a confidence raster the sums are None, and the counts the same
    got, none = gpu_stats(cls, [[big], [part], [big, part], []], K)
    assert none is None and np.array_equal(got, counts)


def test_no_zone_gives_empty_tables(cuda, base):
    from flairhip import ops
    cls, conf = base
    counts, sums = ops.zone_class_stats(torch.tensor(cls).cuda(), [], K0, conf=torch.tensor(conf).cuda())
    assert tuple(counts.shape) == (0, K0 + 1) and tuple(sums.shape) == (0, K0 + 1)
    assert counts.dtype == torch.int64 and sums.dtype == torch.int64 and counts.is_cuda
    counts, sums = ops.zone_class_stats(torch.tensor(cls).cuda(), [], K0)
    assert tuple(counts.shape) == (0, K0 + 1) and sums is None
    # zones without any vertex: zero rows, one launch-free answer each
    got, _ = gpu_stats(cls, [[], []], K0, conf)
    assert got.shape == (2, K0 + 1) and not got.any()


# ---- 6. batching -------------------------------------------------------------------------------------------------------

def test_batches_give_the_bytes_of_the_single_call(cuda, base, parcels):
    from flairhip import ops
    cls, conf = base
    zones, _, want_c, want_s = parcels
    win = ops.zone_stats_windows(*ops.zone_stats_flatten(zones), H0, W0)
    words = ops.zone_stats_plane_words(win)[2]
    budget = 4 * int(words.sum()) // 3
    assert len(ops.zone_stats_batches(words, budget)) >= 3
    one_c, one_s = gpu_stats(cls, zones, K0, conf)
    got_c, got_s = gpu_stats(cls, zones, K0, conf, max_workspace_bytes=budget)
    assert got_c.tobytes() == one_c.tobytes() == want_c.tobytes()
    assert got_s.tobytes() == one_s.tobytes() == want_s.tobytes()
    tight = 4 * int(words.max())  # every batch as small as the largest zone allows
    assert len(ops.zone_stats_batches(words, tight)) > 20
    assert gpu_stats(cls, zones, K0, conf, max_workspace_bytes=tight)[0].tobytes() == want_c.tobytes()
    z = int(np.flatnonzero(words == words.max())[0])
    with pytest.raises(ValueError, match=f"zone {z} "):
        gpu_stats(cls, zones, K0, conf, max_workspace_bytes=tight - 1)


# ---- 7. garbage workspace, repeated calls ------------------------------------------------------------------------------

def test_equal_bytes_whatever_the_workspace_held(cuda, base):
    from flairhip import ops
    cls, conf = base
    zones = mixed_zones() + parcel_grid()[200:260]
    masks = oracle_masks(zones, H0, W0)
    want_c, want_s = oracle_stats(cls, conf, masks, K0)
    outs = []
    for garbage in (0xFF, None, 0x5A):  # None: a second call straight after the first
        if garbage is not None:
            ops.workspace(1, cuda, "zone_stats").fill_(garbage)
        c, s = gpu_stats(cls, zones, K0, conf)
        outs.append(c.tobytes() + s.tobytes())
    assert ops.ZONE_STATS_WORKSPACE_SLOT == "zone_stats"
    assert outs[0] == outs[1] == outs[2] == want_c.tobytes() + want_s.tobytes()


# ---- 8. argument errors ------------------------------------------------------------------------------------------------

def test_argument_errors(cuda, base):
    from flairhip import ops
    cls, conf = base
    zones = [[CENTRE_BOX]]
    d_cls, d_conf = torch.tensor(cls).cuda(), torch.tensor(conf).cuda()
    with pytest.raises(ValueError, match="uint8"):
        ops.zone_class_stats(d_cls.to(torch.int32), zones, K0)
    with pytest.raises(ValueError, match="CUDA"):
        ops.zone_class_stats(torch.tensor(cls), zones, K0)
    with pytest.raises(ValueError, match="conf"):
        ops.zone_class_stats(d_cls, zones, K0, conf=d_conf[:, :-1].contiguous())
    with pytest.raises(ValueError, match="conf"):
        ops.zone_class_stats(d_cls, zones, K0, conf=torch.tensor(conf))
    bad = CENTRE_BOX.copy()
    bad[2, 0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        ops.zone_class_stats(d_cls, [[CENTRE_BOX], [bad]], K0)
    bad[2, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ops.zone_class_stats(d_cls, [[bad]], K0)
    for K in (0, 257, -3):
        with pytest.raises(ValueError, match="n_classes"):
            ops.zone_class_stats(d_cls, zones, K)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        ops.zone_class_stats(d_cls, [[np.zeros((4, 3))]], K0)


# ---- 9. host level -----------------------------------------------------------------------------------------------------

RES, LEFT, TOP = 0.2, 651992.4, 6860417.8


def to_map(ring):
    return np.stack([LEFT + ring[:, 0] * RES, TOP - ring[:, 1] * RES], axis=1)


def to_pix(coords):
    """the pixel coordinates zonal_class_stats derives from map coordinates (the same two numpy lines)"""
    m = np.asarray(coords, dtype=np.float64)
    return np.stack([(m[:, 0] - LEFT) / RES, (TOP - m[:, 1]) / RES], axis=1)


def closed_map(ring):
    m = to_map(ring)
    return np.vstack([m, m[:1]]).tolist()


def layer():
    """three zones in map coordinates with an ``id`` property: a star with a hole, a MultiPolygon of two boxes, a
    triangle off the raster"""
    feats = [
        {"type": "Feature", "properties": {"id": "star", "n": 1},
         "geometry": {"type": "Polygon", "coordinates": [closed_map(STAR), closed_map(STAR_HOLE)]}},
        {"type": "Feature", "properties": {"id": "boxes", "n": 2},
         "geometry": {"type": "MultiPolygon", "coordinates": [[closed_map(CENTRE_BOX + [0.2, 0.3])],
                                                              [closed_map(CENTRE_BOX * [2.0, 1.0] + [41.3, 33.4])]]}},
        {"type": "Feature", "properties": {"id": "nowhere", "n": 3},
         "geometry": {"type": "Polygon", "coordinates": [closed_map(CENTRE_BOX + [300.0, 200.0])]}},
    ]
    return {"type": "FeatureCollection", "features": feats}


def layer_pixel_zones(coll):
    zones = []
    for f in coll["features"]:
        g = f["geometry"]
        polys = [g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]
        zones.append([to_pix(ring) for poly in polys for ring in poly])
    return zones


def expected_table(ids, counts, sums, area):
    """every column as the numpy expression of its definition, from the oracle's integers"""
    K = counts.shape[1] - 1
    pixels = counts.sum(axis=1)
    t = {"zone": np.asarray(ids), "pixels": pixels, "area": pixels * area}
    for k in range(K):
        t[f"pixels_{k}"] = counts[:, k]
        t[f"area_{k}"] = counts[:, k] * area
    t["other"] = counts[:, K]
    t["majority"] = np.array([int(np.argmax(row[:K])) if row[:K].sum() else -1 for row in counts])
    if sums is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            t["confidence"] = np.where(pixels > 0, sums.sum(axis=1) / (255.0 * pixels), np.nan)
            for k in range(K):
                t[f"confidence_{k}"] = np.where(counts[:, k] > 0, sums[:, k] / (255.0 * counts[:, k]), np.nan)
    return t


def tables_equal(a, b):
    assert list(a) == list(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape, name
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y), name
    return True


def test_zonal_class_stats_table_csv_and_zone_crs(cuda, base, tmp_path):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.raster import ArrayRaster
    from flair_zonal_detection.zonal_stats import write_zone_stats_csv, zonal_class_stats
    from flair_zonal_detection.zone import reproject_zone
    cls, conf = base
    paths = {}
    for name, data in (("classes", cls), ("confidence", conf)):
        paths[name] = str(tmp_path / f"{name}.tif")
        with GeoTiffWriter.like(paths[name], ArrayRaster(data[None], LEFT, TOP, RES), 1) as w:
            w.data[...] = data[None]
    coll = layer()
    zpath = str(tmp_path / "zones.geojson")
    with open(zpath, "w") as f:
        json.dump(coll, f)
    zones = layer_pixel_zones(coll)
    masks = oracle_masks(zones, H0, W0)
    counts, sums = oracle_stats(cls, conf, masks, K0)
    assert counts[0].sum() > 3000 and counts[1].sum() == 400 + 800 and counts[2].sum() == 0

    table = zonal_class_stats(paths["classes"], zpath, id_field="id", confidence=paths["confidence"])
    want = expected_table(["star", "boxes", "nowhere"], counts, sums, abs(RES * RES))
    assert tables_equal(table, want)
    assert table["majority"][2] == -1 and np.isnan(table["confidence"][2]) and table["other"].sum() > 0
    assert table.n_classes == K0 and table.crs == "EPSG:2154"
    # the index names the zones without an id_field; no confidence, no confidence columns; another K, other columns
    plain = zonal_class_stats(paths["classes"], coll, n_classes=5)
    c5, _ = oracle_stats(cls, None, masks, 5)
    assert tables_equal(plain, expected_table(np.arange(3), c5, None, abs(RES * RES)))
    with pytest.raises(ValueError, match="owner"):
        zonal_class_stats(paths["classes"], coll, id_field="owner")
    # the outputs-dict form of raster_to_polygons, confidence=True
    outs = {TASK: paths["classes"], TASK + "_confidence": paths["confidence"]}
    assert tables_equal(zonal_class_stats(outs, coll, id_field="id", confidence=True), want)

    # the CSV round-trips
    with open(write_zone_stats_csv(table, str(tmp_path / "t.csv")), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(want) and len(rows) == 4
    for c, name in enumerate(rows[0]):
        col = [r[c] for r in rows[1:]]
        if name == "zone":
            assert col == ["star", "boxes", "nowhere"]
        elif want[name].dtype.kind == "i":
            assert [int(v) for v in col] == want[name].tolist()
        else:
            assert np.array_equal(np.array([float(v) for v in col]), want[name], equal_nan=True), name

    # a layer in another CRS: zone_crs reprojects it like reproject_zone on the host does
    def moved(src, dst, feats):
        return {"type": "FeatureCollection", "features": [
            {"type": "Feature", "properties": f["properties"], "geometry": reproject_zone(f, src, dst)} for f in feats]}

    lonlat = moved("EPSG:2154", "EPSG:4326", coll["features"])
    assert abs(lonlat["features"][0]["geometry"]["coordinates"][0][0][0][1]) < 90.0
    back = moved("EPSG:4326", "EPSG:2154", lonlat["features"])
    a = zonal_class_stats(paths["classes"], lonlat, id_field="id", confidence=paths["confidence"], zone_crs="EPSG:4326")
    b = zonal_class_stats(paths["classes"], back, id_field="id", confidence=paths["confidence"])
    assert tables_equal(a, b) and a["pixels"][0] > 3000 and a["pixels"][1] > 1000
    # naming the raster's own CRS changes nothing
    assert tables_equal(zonal_class_stats(paths["classes"], coll, id_field="id", confidence=paths["confidence"],
                                          zone_crs="EPSG:2154"), want)


# ---- 10. CLI end to end ------------------------------------------------------------------------------------------------

ZH, ZW = 200, 260


@pytest.fixture(scope="module")
def zonal(tmp_path_factory):
    """the smallest multi-tile configuration of tests/test_zonal_gpu.py: 200 x 260 pixels of 0.2 m, 128-pixel tiles
    with a 16-pixel margin, bf16, hip_graph as it defaults (a fixture of this module's own)"""
    import yaml
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    tmp = tmp_path_factory.mktemp("zone_stats")
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(1, 255, (3, ZH, ZW)).astype(np.uint8), LEFT, TOP, RES)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": 0.2, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    oracle = UnetResNet34(3, 19)
    sd = fill_state_dict(oracle.state_dict(), seed=5)
    sd["segmentation_head.0.bias"] = sd["segmentation_head.0.bias"] + torch.linspace(0, 3, 19)
    oracle.load_state_dict(sd)
    cfg["model_weights"] = str(tmp / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    return cfg, ras


def test_cli_zone_stats(cuda, zonal, tmp_path):
    import yaml
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.main import main
    from flair_zonal_detection.raster import open_raster
    cfg, ras = zonal
    src = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src, ras, 3) as w:
        w.data[...] = ras.data
    rings = {"l": np.array([[-9.0, -4.0], [ZW + 6.0, -4.0], [ZW + 6.0, 41.3], [50.6, 41.3], [50.6, ZH + 5.0], [-9.0, ZH + 5.0]]),
             "tri": np.array([[100.2, 60.4], [230.8, 75.1], [140.5, 180.9]]),
             "off": CENTRE_BOX + [400.0, 0.0]}
    coll = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"id": k}, "geometry": {"type": "Polygon", "coordinates": [closed_map(r)]}}
        for k, r in rings.items()]}
    zpath = str(tmp_path / "parcels.geojson")
    with open(zpath, "w") as f:
        json.dump(coll, f)

    def run(out_dir, extra_cfg, argv):
        fcfg = copy.deepcopy(cfg)
        fcfg["modalities"][MOD]["input_img_path"] = src
        fcfg["output_path"] = str(tmp_path / out_dir)
        fcfg.update(extra_cfg)
        ypath = str(tmp_path / f"{out_dir}.yaml")
        with open(ypath, "w") as f:
            yaml.safe_dump(fcfg, f)
        main(["--config", ypath] + argv)
        return sorted(glob.glob(os.path.join(fcfg["output_path"], "**", "*"), recursive=True))

    files = run("with", {"write_confidence": True}, ["--zone-stats", zpath, "--zone-stats-id", "id"])
    tables = [p for p in files if p.endswith("_zone_stats.csv")]
    assert len(tables) == 1
    tif = tables[0][:-len("_zone_stats.csv")] + ".tif"
    conf_tif, = [p for p in files if p.endswith(".tif") and "confidence" in os.path.basename(p)]
    assert tif in files and tif != conf_tif
    written, wconf = open_raster(tif).read(1), open_raster(conf_tif).read(1)
    assert written.shape == (ZH, ZW) and written.dtype == np.uint8
    masks = oracle_masks(layer_pixel_zones(coll), ZH, ZW)
    counts, sums = oracle_stats(written, wconf, masks, 19)
    assert counts[0].sum() > 10000 and counts[1].sum() > 5000 and counts[2].sum() == 0
    want = expected_table(list(rings), counts, sums, abs(RES * RES))
    with open(tables[0], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(want) and [r[0] for r in rows[1:]] == ["l", "tri", "off"]
    for c, name in enumerate(rows[0][1:], start=1):
        col = [r[c] for r in rows[1:]]
        if want[name].dtype.kind == "i":
            assert [int(v) for v in col] == want[name].tolist(), name
        else:
            assert np.array_equal(np.array([float(v) for v in col]), want[name], equal_nan=True), name

    # without the flag (and without the config key) no table appears
    files = run("without", {}, [])
    assert any(p.endswith(".tif") for p in files) and not [p for p in files if "zone_stats" in os.path.basename(p)]
