"""Land-cover change at the host level (flair_zonal_detection/change.py, the config key change_from): two small
GeoTIFFs on one grid written with the project's own writer, the tables against tests/change_oracle.py, the change
polygons of a hand-made pair, and the run_inference path."""
import copy
import csv
import glob
import json
import os

import numpy as np
import pytest
import torch

from change_oracle import oracle_change
from helpers import MOD, ROOT, TASK, oracle_to_product_keys
from zone_stats_oracle import CENTRE_BOX, H0, STAR, STAR_HOLE, W0, base_rasters, oracle_masks

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")
K0 = 19
RES, LEFT, TOP = 0.2, 651992.4, 6860417.8


def to_map(ring):
    return np.stack([LEFT + ring[:, 0] * RES, TOP - ring[:, 1] * RES], axis=1)


def to_pix(coords):
    """the pixel coordinates the host derives from map coordinates (the same two numpy lines)"""
    m = np.asarray(coords, dtype=np.float64)
    return np.stack([(m[:, 0] - LEFT) / RES, (TOP - m[:, 1]) / RES], axis=1)


def closed_map(ring):
    m = to_map(ring)
    return np.vstack([m, m[:1]]).tolist()


def write_tif(path, data, left=LEFT, top=TOP):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.raster import ArrayRaster
    with GeoTiffWriter.like(str(path), ArrayRaster(data[None], left, top, RES), 1) as w:
        w.data[...] = data[None]
    return str(path)


def tables_equal(a, b):
    assert list(a) == list(b)
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.shape == y.shape, name
        assert np.array_equal(x, y, equal_nan=True) if x.dtype.kind == "f" else np.array_equal(x, y), name
    return True


def read_csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def csv_equals(path, columns):
    """a CSV file holds ``columns`` ({name: array}): the names in order, ints exactly, floats as the same float64"""
    head, rows = read_csv(path)
    assert head == list(columns) and len(rows) == len(next(iter(columns.values())))
    for c, name in enumerate(head):
        col, want = [r[c] for r in rows], np.asarray(columns[name])
        if want.dtype.kind == "i":
            assert [int(v) for v in col] == want.tolist(), name
        elif want.dtype.kind == "f":
            assert np.array_equal(np.array([float(v) for v in col]), want, equal_nan=True), name
        else:
            assert col == [str(v) for v in want], name
    return True


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("change_pair")
    before, _ = base_rasters(seed=11)
    after, conf = base_rasters(seed=12)
    paths = {n: write_tif(tmp / f"{n}.tif", d) for n, d in (("before", before), ("after", after), ("conf", conf))}
    return before, after, conf, paths


def layer():
    feats = [
        {"type": "Feature", "properties": {"id": "star"},
         "geometry": {"type": "Polygon", "coordinates": [closed_map(STAR), closed_map(STAR_HOLE)]}},
        {"type": "Feature", "properties": {"id": "boxes"},
         "geometry": {"type": "MultiPolygon", "coordinates": [[closed_map(CENTRE_BOX + [0.2, 0.3])],
                                                              [closed_map(CENTRE_BOX * [2.0, 1.0] + [41.3, 33.4])]]}},
        {"type": "Feature", "properties": {"id": "nowhere"},
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


def test_zonal_change_stats_tables_and_csv(cuda, pair, tmp_path):
    from flair_zonal_detection.change import (change_table, write_change_csv, write_transitions_csv,
                                              zonal_change_stats)
    before, after, conf, paths = pair
    coll = layer()
    zpath = str(tmp_path / "parcels.geojson")
    with open(zpath, "w") as f:
        json.dump(coll, f)
    masks = oracle_masks(layer_pixel_zones(coll), H0, W0)
    counts, sums = oracle_change(before, after, conf, masks, K0)
    assert counts[0].sum() > 3000 and counts[1].sum() == 400 + 800 and counts[2].sum() == 0
    table = zonal_change_stats(paths["before"], paths["after"], zpath, id_field="id", confidence=paths["conf"])
    want = change_table(["star", "boxes", "nowhere"], counts, sums, RES * RES)
    assert tables_equal(table, want) and tables_equal(table.transitions, want.transitions)
    assert table.n_classes == K0 and table.crs == "EPSG:2154"
    assert table["changed"][0] > 3000 and np.isnan(table["changed_fraction"][2]) and np.isnan(table["confidence_changed"][2])
    assert (table.transitions["from"] == -1).any() and (table.transitions["to"] == -1).any()
    # no zones: the whole raster is one zone; no confidence: no confidence columns; another K
    whole = zonal_change_stats(paths["before"], paths["after"], n_classes=5)
    c5, _ = oracle_change(before, after, None, np.ones((1, H0, W0), bool), 5)
    assert tables_equal(whole, change_table([0], c5, None, RES * RES)) and whole["pixels"][0] == H0 * W0
    assert "confidence_changed" not in whole and "confidence" not in whole.transitions
    # the outputs-dict form with confidence=True
    outs = {TASK: paths["after"], TASK + "_confidence": paths["conf"]}
    assert tables_equal(zonal_change_stats(paths["before"], outs, coll, id_field="id", confidence=True), want)
    # both CSV forms round-trip
    assert csv_equals(write_change_csv(table, str(tmp_path / "wide.csv")), want)
    assert csv_equals(write_transitions_csv(table, str(tmp_path / "long.csv")), want.transitions)
    assert len(read_csv(str(tmp_path / "wide.csv"))[1]) == 3
    assert len(read_csv(str(tmp_path / "long.csv"))[1]) == np.count_nonzero(counts)


def test_a_before_raster_on_another_grid_is_refused(cuda, pair, tmp_path):
    from flair_zonal_detection.change import change_polygons, zonal_change_stats
    before, after, conf, paths = pair
    shifted = write_tif(tmp_path / "shifted.tif", before, left=LEFT + RES)
    with pytest.raises(ValueError, match="zonal_change_stats: the before raster's bounds"):
        zonal_change_stats(shifted, paths["after"])
    with pytest.raises(ValueError, match="change_polygons: the before raster's bounds"):
        change_polygons(shifted, paths["after"])
    smaller = write_tif(tmp_path / "smaller.tif", before[:-1])
    with pytest.raises(ValueError, match="before raster is"):
        zonal_change_stats(smaller, paths["after"])
    with pytest.raises(ValueError, match="n_classes"):
        zonal_change_stats(paths["before"], paths["after"], n_classes=33)


def test_change_polygons_of_a_hand_made_pair(cuda, tmp_path):
    from flair_zonal_detection.change import change_polygons
    before = np.full((60, 80), 3, np.uint8)
    before[:, 40:] = 9
    after = before.copy()
    after[5:15, 10:20] = 0     # a 10 x 10 block becomes class 0 (from 3)
    after[30:34, 50:54] = 6    # a 4 x 4 block becomes class 6 (from 9)
    after[34:37, 54:57] = 6    # and a 3 x 3 block diagonally adjacent to it: 4-connectivity keeps them apart
    conf = np.full((60, 80), 51, np.uint8)
    pb, pa, pc = (write_tif(tmp_path / f"{n}.tif", d) for n, d in (("b", before), ("a", after), ("c", conf)))
    frame = change_polygons(pb, pa, min_area=0.0, simplification=0.0, confidence=pc)
    assert list(frame.columns)[:3] == ["transition", "from_class", "to_class"] and "class_id" not in frame.columns
    assert len(frame) == 3 and frame.crs == "EPSG:2154"
    assert frame["transition"].tolist() == ["*:0", "*:6", "*:6"]
    assert frame["from_class"].tolist() == [-1, -1, -1] and frame["to_class"].tolist() == [0, 6, 6]
    assert frame["pixels"].tolist() == [100, 16, 9]
    assert [g.area for g in frame["geometry"]] == pytest.approx([100 * RES * RES, 16 * RES * RES, 9 * RES * RES], rel=1e-9)
    assert frame["confidence"].tolist() == [51 / 255.0] * 3
    x0, y0, x1, y1 = frame["geometry"].iloc[0].bounds
    assert (x0, y1) == pytest.approx((LEFT + 10 * RES, TOP - 5 * RES), abs=1e-6)
    # a listed transition keeps only its regions; explicit pairs carry both classes
    only = change_polygons(pb, pa, transitions=["*:0"], min_area=0.0, simplification=0.0)
    assert len(only) == 1 and only["to_class"].tolist() == [0] and only["geometry"].iloc[0].area == pytest.approx(4.0, rel=1e-9)
    exact = change_polygons(pb, pa, transitions=["3:6", "9:6"], min_area=0.0, simplification=0.0)
    assert exact["transition"].tolist() == ["9:6", "9:6"] and exact["from_class"].tolist() == [9, 9]
    # min_area is the polygoniser's: 0.5 m2 = 12.5 pixels drops the 3 x 3 block
    assert len(change_polygons(pb, pa, min_area=0.5, simplification=0.0)) == 2
    # an unchanged pair: an empty frame with the same columns
    none = change_polygons(pa, pa, min_area=0.0)
    assert len(none) == 0 and list(none.columns)[:3] == ["transition", "from_class", "to_class"]


# ---- the run_inference path -------------------------------------------------------------------------------------------

ZH, ZW = 200, 260


@pytest.fixture(scope="module")
def zonal(tmp_path_factory):
    """the smallest multi-tile configuration of tests/test_zonal_gpu.py, as tests/test_zone_stats_gpu.py builds it:
    200 x 260 pixels of 0.2 m, 128-pixel tiles with a 16-pixel margin, bf16"""
    import yaml
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    tmp = tmp_path_factory.mktemp("change_run")
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


def test_run_inference_with_change_from(cuda, zonal, tmp_path):
    import yaml
    import sqlite3
    from flair_zonal_detection.change import change_polygons, change_table
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.inference import run_inference
    from flair_zonal_detection.main import main
    from flair_zonal_detection.raster import open_raster
    cfg, ras = zonal
    src = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src, ras, 3) as w:
        w.data[...] = ras.data
    earlier = np.random.default_rng(8).integers(0, 19, (ZH, ZW)).astype(np.uint8)
    earlier[:20, :30] = 255
    before = write_tif(tmp_path / "earlier.tif", earlier)
    rings = {"l": np.array([[-9.0, -4.0], [ZW + 6.0, -4.0], [ZW + 6.0, 41.3], [50.6, 41.3], [50.6, ZH + 5.0], [-9.0, ZH + 5.0]]),
             "tri": np.array([[100.2, 60.4], [230.8, 75.1], [140.5, 180.9]]),
             "off": CENTRE_BOX + [400.0, 0.0]}
    coll = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {"id": k}, "geometry": {"type": "Polygon", "coordinates": [closed_map(r)]}}
        for k, r in rings.items()]}
    zpath = str(tmp_path / "parcels.geojson")
    with open(zpath, "w") as f:
        json.dump(coll, f)

    def run(out_dir, extra_cfg, argv=None):
        fcfg = copy.deepcopy(cfg)
        fcfg["modalities"][MOD]["input_img_path"] = src
        fcfg["output_path"] = str(tmp_path / out_dir)
        fcfg.update(extra_cfg)
        ypath = str(tmp_path / f"{out_dir}.yaml")
        with open(ypath, "w") as f:
            yaml.safe_dump(fcfg, f)
        if argv is None:
            run_inference(ypath)
        else:
            main(["--config", ypath] + argv)
        return sorted(glob.glob(os.path.join(fcfg["output_path"], "**", "*"), recursive=True))

    files = run("with", {"write_confidence": True, "change_from": {TASK: before}, "zone_stats": zpath, "zone_stats_id": "id"})
    wide = [p for p in files if p.endswith("_zone_change.csv")]
    long = [p for p in files if p.endswith("_zone_transitions.csv")]
    assert len(wide) == 1 and len(long) == 1
    tif = wide[0][:-len("_zone_change.csv")] + ".tif"
    conf_tif, = [p for p in files if p.endswith(".tif") and "confidence" in os.path.basename(p)]
    assert tif in files and tif != conf_tif and long[0] == tif[:-len(".tif")] + "_zone_transitions.csv"
    written, wconf = open_raster(tif).read(1), open_raster(conf_tif).read(1)
    assert written.shape == (ZH, ZW) and written.dtype == np.uint8
    masks = oracle_masks(layer_pixel_zones(coll), ZH, ZW)
    counts, sums = oracle_change(earlier, written, wconf, masks, 19)
    assert counts[0].sum() > 10000 and counts[1].sum() > 5000 and counts[2].sum() == 0 and counts[0, 19].sum() > 0
    want = change_table(list(rings), counts, sums, RES * RES)
    assert csv_equals(wide[0], want) and csv_equals(long[0], want.transitions)

    # the command line: the same tables from --change-from, and the changed regions as a GeoPackage
    gpkg = str(tmp_path / "changed.gpkg")
    top = int(np.bincount(written.ravel(), minlength=19)[:19].argmax())  # the run's most frequent class: regions of it exist
    files = run("cli", {"write_confidence": True, "zone_stats": zpath, "zone_stats_id": "id"},
                ["--change-from", before, "--change-polygons", gpkg, "--change-transitions", f"*:{top},*:*"])
    cli_wide, = [p for p in files if p.endswith("_zone_change.csv")]
    assert read_csv(cli_wide) == read_csv(wide[0])
    frame = change_polygons(before, tif, transitions=[f"*:{top}", "*:*"], confidence=conf_tif)
    con = sqlite3.connect(gpkg)
    rows = con.execute('SELECT class_id, from_class, to_class, pixels, confidence FROM "changed" ORDER BY fid').fetchall()
    con.close()
    assert len(rows) == len(frame) > 0 and rows[0][0] == 0 and {r[0] for r in rows} <= {0, 1}
    assert [r[0] for r in rows] == [0 if t == f"*:{top}" else 1 for t in frame["transition"]]
    assert [r[1:4] for r in rows] == list(zip(frame["from_class"], frame["to_class"], frame["pixels"]))
    assert [r[4] for r in rows] == frame["confidence"].tolist()
    assert {(r[1], r[2]) for r in rows} <= {(-1, top), (-1, -1)}

    # without the key nothing is written
    files = run("without", {})
    assert any(p.endswith(".tif") for p in files) and not [p for p in files if "zone_" in os.path.basename(p)]
