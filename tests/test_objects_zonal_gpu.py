"""Where users meet object matching: raster_to_polygons(compare=...), compare.compare_objects and the test stage's
object_metrics.json, each against the numpy oracle (tests/objects_oracle.py) on rasters written with the project's
GeoTIFF writer."""
import csv
import json
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import objects_oracle as oracle

pytestmark = pytest.mark.gpu

H, W, RES, LEFT, TOP, CRS = 96, 128, 0.2, 650000.0, 6860000.0, "EPSG:2154"
OPTIONS = dict(background_value=0, min_area=0.12, simplification=0.0)  # 0.12 / 0.04: three pixels or more
MINP = 3


def blobs(h, w, seed, classes=4, cell=(5, 6), salt=0.03):
    g = np.random.default_rng(seed)
    ch, cw = cell
    coarse = g.integers(0, classes, ((h + ch - 1) // ch, (w + cw - 1) // cw))
    out = np.repeat(np.repeat(coarse, ch, 0), cw, 1)[:h, :w].astype(np.uint8)
    m = g.random((h, w)) < salt
    out[m] = g.integers(0, classes, int(m.sum()))
    return out


def write_raster(path, data, dtype=np.uint8, col0=0):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    h, w = data.shape
    out = GeoTiffWriter(str(path), w, h, 1, LEFT + col0 * RES, TOP, RES, crs=CRS, dtype=dtype)
    out.data[0] = data
    out.close()
    return str(path)


@pytest.fixture(scope="module")
def rasters(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    root = tmp_path_factory.mktemp("objects")
    pred = blobs(H, W, 1)
    ref = np.roll(pred, (1, 2), (0, 1))
    ref[40:60, 30:80] = blobs(20, 50, 2)
    ia, ta = oracle.regions(pred, 0, MINP)
    ib, tb = oracle.regions(ref, 0, MINP)
    return SimpleNamespace(root=root, pred=pred, ref=ref, pred_path=write_raster(root / "pred.tif", pred),
                           ref_path=write_raster(root / "ref.tif", ref), ia=ia, ib=ib, ta=ta, tb=tb,
                           pairs=oracle.overlaps(ia, ib))


def want_columns(ta, tb, pairs, thr, classes):
    a_match, _, a_cov, b_match, _, _, accepted = oracle.match(ta, tb, pairs, thr, classes)
    oa, ob = oracle.class_order(ta), oracle.class_order(tb)
    rank_b = {i: r for r, i in enumerate(ob)}
    rank_a = {i: r for r, i in enumerate(oa)}
    pred = {"match_iou": [accepted.get((i, a_match[i]), 0.0) for i in oa],
            "matched": [int(a_match[i] >= 0) for i in oa],
            "ref_id": [rank_b[a_match[i]] if a_match[i] >= 0 else -1 for i in oa],
            "ref_fraction": [a_cov[i] for i in oa]}
    ref = {"match_iou": [accepted.get((b_match[i], i), 0.0) for i in ob],
           "pred_id": [rank_a[b_match[i]] if b_match[i] >= 0 else -1 for i in ob]}
    return pred, ref, (a_match, b_match, accepted)


@pytest.mark.parametrize("thr,classes", [(0.5, "same"), (0.3, "any")])
def test_the_four_columns_against_the_oracle(cuda, rasters, thr, classes):
    from flair_zonal_detection.inference import raster_to_polygons
    frame = raster_to_polygons(rasters.pred_path, compare=rasters.ref_path, compare_iou=thr, compare_classes=classes,
                               **OPTIONS)
    want, _, _ = want_columns(rasters.ta, rasters.tb, rasters.pairs, thr, classes)
    assert list(frame.columns) == ["class_id", "match_iou", "matched", "ref_id", "ref_fraction", "geometry"]
    assert frame["class_id"].tolist() == [rasters.ta[i][1] for i in oracle.class_order(rasters.ta)]
    for name, dtype in (("match_iou", np.float64), ("matched", np.int64), ("ref_id", np.int64),
                        ("ref_fraction", np.float64)):
        assert frame[name].dtype == dtype, name
        assert frame[name].tolist() == want[name], name
    assert 0 < sum(want["matched"]) < len(want["matched"])


def test_compare_none_changes_nothing_and_the_other_columns_do_not_depend_on_compare(cuda, rasters):
    from flair_zonal_detection.inference import raster_to_polygons
    conf = write_raster(rasters.root / "conf.tif", (blobs(H, W, 9, classes=200) + 50).astype(np.uint8))
    plain = raster_to_polygons(rasters.pred_path, confidence=conf, **OPTIONS)
    none = raster_to_polygons(rasters.pred_path, confidence=conf, compare=None, **OPTIONS)
    with_ref = raster_to_polygons(rasters.pred_path, confidence=conf, compare=rasters.ref_path, **OPTIONS)
    assert list(plain.columns) == list(none.columns) == ["class_id", "confidence", "pixels", "geometry"]
    assert list(with_ref.columns) == ["class_id", "confidence", "pixels", "match_iou", "matched", "ref_id",
                                      "ref_fraction", "geometry"]
    for other in (none, with_ref):
        for name in ("class_id", "confidence", "pixels"):
            assert plain[name].to_numpy().tobytes() == other[name].to_numpy().tobytes(), name
        assert [g.wkb for g in plain["geometry"]] == [g.wkb for g in other["geometry"]]


def test_a_mosaic_takes_a_reference_over_its_whole_grid(cuda, rasters):
    from flair_zonal_detection.inference import raster_to_polygons, rasters_to_polygons
    parts = [write_raster(rasters.root / "left.tif", rasters.pred[:, :67].copy()),
             write_raster(rasters.root / "right.tif", rasters.pred[:, 67:].copy(), col0=67)]
    got = rasters_to_polygons(parts[::-1], compare=rasters.ref_path, **OPTIONS)
    want = raster_to_polygons(rasters.pred_path, compare=rasters.ref_path, **OPTIONS)
    assert list(got.columns) == list(want.columns) and len(got) == len(want) > 0
    for name in ("class_id", "match_iou", "matched", "ref_id", "ref_fraction"):
        assert got[name].to_numpy().tobytes() == want[name].to_numpy().tobytes(), name
    with pytest.raises(ValueError, match="compare raster is"):
        rasters_to_polygons(parts[:1], compare=rasters.ref_path, **OPTIONS)


def test_a_reference_of_another_grid_raises(cuda, rasters):
    from flair_zonal_detection.inference import raster_to_polygons
    small = write_raster(rasters.root / "small.tif", rasters.ref[:, :120].copy())
    with pytest.raises(ValueError, match="compare raster is"):
        raster_to_polygons(rasters.pred_path, compare=small, **OPTIONS)
    wide = write_raster(rasters.root / "wide.tif", rasters.ref.astype(np.uint16), dtype=np.uint16)
    with pytest.raises(ValueError, match="uint8 compare raster expected"):
        raster_to_polygons(rasters.pred_path, compare=wide, **OPTIONS)
    with pytest.raises(ValueError, match="compare_classes"):
        raster_to_polygons(rasters.pred_path, compare=rasters.ref_path, compare_classes="both", **OPTIONS)


def test_a_geometry_gives_the_share_of_the_zone_mask(cuda, rasters):
    from flair_zonal_detection.inference import raster_to_polygons
    r0, r1, c0, c1 = 10, 70, 20, 90  # a box on pixel borders: the centres of rows 10 .. 69, columns 20 .. 89 are inside
    box = (LEFT + c0 * RES, TOP - r1 * RES, LEFT + c1 * RES, TOP - r0 * RES)
    frame = raster_to_polygons(rasters.pred_path, compare=box, compare_iou=0.5, compare_classes="same", **OPTIONS)
    inside = np.zeros((H, W), bool)
    inside[r0:r1, c0:c1] = True
    want = []
    for i in oracle.class_order(rasters.ta):
        region = rasters.ia == i
        want.append(int((region & inside).sum()) / int(region.sum()))
    assert frame["ref_fraction"].tolist() == want
    assert 0.0 in want and 1.0 in want and any(0.0 < v < 1.0 for v in want)
    assert set(frame["ref_id"].tolist()) <= {-1, 0}  # the box is one region; classes were not asked to agree


def test_compare_objects_statuses_agree_with_the_summary(cuda, rasters):
    from flair_zonal_detection.compare import compare_objects
    pred, ref, summary = compare_objects(rasters.pred_path, rasters.ref_path, compare_iou=0.5, **OPTIONS)
    want_pred, want_ref, (a_match, b_match, accepted) = want_columns(rasters.ta, rasters.tb, rasters.pairs, 0.5, "same")
    assert pred["status"].tolist() == ["matched" if m else "new" for m in want_pred["matched"]]
    assert ref["pred_id"].tolist() == want_ref["pred_id"] and ref["match_iou"].tolist() == want_ref["match_iou"]
    assert ref["status"].tolist() == ["matched" if i >= 0 else "missing" for i in want_ref["pred_id"]]
    assert ref["class_id"].tolist() == [rasters.tb[i][1] for i in oracle.class_order(rasters.tb)]
    micro = summary["micro"]
    assert micro["tp"] == (pred["status"] == "matched").sum() == (ref["status"] == "matched").sum() == len(accepted)
    assert micro["fp"] == (pred["status"] == "new").sum() and micro["fn"] == (ref["status"] == "missing").sum()
    counts, sums = oracle.counts(rasters.ta, rasters.tb, a_match, b_match, accepted, 4)
    for k in range(4):
        got = summary["classes"][str(k)]
        assert [got["tp"], got["fp"], got["fn"]] == counts[k]
    assert summary["iou_threshold"] == 0.5 and summary["compare_classes"] == "same"
    # every matched pair points at each other
    for q, r in enumerate(pred["ref_id"].tolist()):
        assert r < 0 or ref["pred_id"].tolist()[r] == q


def test_the_geopackage_takes_the_four_columns(cuda, rasters, tmp_path):
    import sqlite3
    from flair_zonal_detection.inference import raster_to_polygons
    frame = raster_to_polygons(rasters.pred_path, compare=rasters.ref_path, **OPTIONS)
    path = str(tmp_path / "objects.gpkg")
    frame.to_file(path, driver="GPKG")
    with sqlite3.connect(path) as db:
        table = db.execute("SELECT table_name FROM gpkg_contents").fetchone()[0]
        types = {row[1]: row[2] for row in db.execute(f'PRAGMA table_info("{table}")')}
        rows = db.execute(f'SELECT match_iou, matched, ref_id, ref_fraction FROM "{table}" ORDER BY rowid').fetchall()
    assert types["match_iou"] == "REAL" and types["ref_fraction"] == "REAL"
    assert types["matched"] == "INTEGER" and types["ref_id"] == "INTEGER"
    assert [list(r) for r in rows] == [list(r) for r in zip(frame["match_iou"].tolist(), frame["matched"].tolist(),
                                                            frame["ref_id"].tolist(), frame["ref_fraction"].tolist())]


# ---- the command line -----------------------------------------------------------------------------------------------

def test_cli_compare(cuda, tmp_path):
    """the smallest multi-tile configuration of tests/test_zone_gpu.py through main(): the GeoPackage carries the four
    columns and <polygons stem>_objects.json the summary, both equal to the direct call on the written raster"""
    import sqlite3
    import yaml
    from helpers import MOD, ROOT, oracle_to_product_keys
    from helpers import TASK as ZTASK
    from flair_zonal_detection.compare import summary_of
    from flair_zonal_detection.geotiff import GeoTiffRaster, GeoTiffWriter
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.main import main
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    zh, zw, left, top = 200, 260, 651992.4, 6860417.8
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(1, 255, (3, zh, zw)).astype(np.uint8), left, top, 0.2)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp_path), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": 0.2, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}, "compare_iou": 0.25})
    cfg["modalities"][MOD].update({"channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": ZTASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    net = UnetResNet34(3, 19)
    net.load_state_dict(fill_state_dict(net.state_dict(), seed=5))
    cfg["model_weights"] = str(tmp_path / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(net.state_dict()).items()}},
               cfg["model_weights"])
    src = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src, ras, 3) as w:
        w.data[...] = ras.data
    cfg["modalities"][MOD]["input_img_path"] = src
    ypath = str(tmp_path / "zonal.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(cfg, f)
    ref_path = str(tmp_path / "ref.tif")
    with GeoTiffWriter.like(ref_path, ras, 1) as w:
        w.data[0] = blobs(zh, zw, 12, classes=19, cell=(3, 3), salt=0.2)
    gpkg = str(tmp_path / "polygons.gpkg")
    main(["--config", ypath, "--polygons", gpkg, "--compare", ref_path, "--compare-classes", "any"])

    sink = {}
    with GeoTiffRaster(str(tmp_path / f"z_{ZTASK}_argmax_i.tif")) as r:
        want = raster_to_polygons(r, compare=ref_path, compare_iou=0.25, compare_classes="any", _compare_sink=sink)
    assert len(want) > 0
    with sqlite3.connect(gpkg) as db:
        table = db.execute("SELECT table_name FROM gpkg_contents").fetchone()[0]
        rows = db.execute(f'SELECT class_id, match_iou, matched, ref_id, ref_fraction FROM "{table}" ORDER BY fid').fetchall()
    assert [list(r) for r in rows] == [list(r) for r in zip(*(want[c].tolist() for c in (
        "class_id", "match_iou", "matched", "ref_id", "ref_fraction")))]
    with open(str(tmp_path / "polygons_objects.json")) as f:
        summary = json.load(f)
    assert {k: summary[k] for k in ("classes", "micro", "iou_threshold", "compare_classes")} == \
        json.loads(json.dumps(summary_of(sink, 0.25)))
    assert summary["iou_threshold"] == 0.25 and summary["compare_classes"] == "any" and summary["polygons"] == len(want)
    assert summary["micro"]["tp"] + summary["micro"]["fp"] == len(want)


# ---- the test stage ----------------------------------------------------------------------------------------------------

TASK, K, N, SIZE = "LABEL", 4, 4, 64
OBJECT_OPTIONS = {"iou_threshold": 0.5, "min_pixels": 2, "classes": None}


def stage_config(root, object_metrics):
    tasks = {"predict": False, "metrics_only": True, "write_files": False, "georeferencing_output": False}
    if object_metrics is not None:
        tasks["object_metrics"] = object_metrics
    return {"labels": [TASK], "labels_configs": {TASK: {"value_name": {0: "soil", 1: "roof", 2: "pool", 3: "road"}}},
            "modalities": {"inputs": {"AERIAL_RGBI": True}}, "tasks": tasks,
            "paths": {"out_model_name": "m", "test_csv": os.path.join(root, "test.csv")}}


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """four 64 x 64 label / prediction pairs on disk, values >= K among the labels, and the oracle's counts"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    root = str(tmp_path_factory.mktemp("stage"))
    pred_dir = os.path.join(root, "out", "predictions_m", TASK)
    os.makedirs(pred_dir)
    os.makedirs(os.path.join(root, "labels"))
    g = np.random.default_rng(5)
    labels, preds, paths = [], [], []
    counts, sums = np.zeros((K, 3), np.int64), np.zeros(K)
    for j in range(N):
        label = blobs(SIZE, SIZE, 30 + j, classes=K, cell=(6, 7))
        pred = np.roll(label, (1, 1), (0, 1))
        pred[20:40, 10:50] = blobs(20, 40, 40 + j, classes=K)
        label[g.random((SIZE, SIZE)) < 0.03] = 200  # ignored ground truth
        labels.append(label)
        preds.append(pred)
        paths.append(write_raster(os.path.join(root, "labels", f"L_{j}.tif"), label))
        write_raster(os.path.join(pred_dir, f"PRED_L_{j}.tif"), pred)
        tgt = np.where(label >= K, 255, label).astype(np.uint8)
        prd = np.where(label >= K, 255, pred).astype(np.uint8)
        ia, ta = oracle.regions(prd, 255, OBJECT_OPTIONS["min_pixels"])
        ib, tb = oracle.regions(tgt, 255, OBJECT_OPTIONS["min_pixels"])
        a_match, _, _, b_match, _, _, accepted = oracle.match(ta, tb, oracle.overlaps(ia, ib), 0.5, "same")
        c, s = oracle.counts(ta, tb, a_match, b_match, accepted, K)
        counts += np.array(c)
        sums += np.array(s)
    with open(os.path.join(root, "test.csv"), "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow([TASK])
        wr.writerows([p] for p in paths)
    return SimpleNamespace(root=root, labels=labels, preds=preds, paths=paths, counts=counts, sums=sums)


def run_metrics_only(stage, tmp_path, object_metrics):
    from flair_hub.writer.prediction_writer import PredictionWriter
    out = str(tmp_path / ("on" if object_metrics else "off"))
    shutil.copytree(os.path.join(stage.root, "out"), out)
    PredictionWriter(stage_config(stage.root, object_metrics), out).load_predictions_and_compute_metrics()
    return os.path.join(out, "metrics_m", TASK)


def check_object_metrics(path, stage):
    with open(path) as f:
        got = json.load(f)
    names = ["soil", "roof", "pool", "road"]
    assert list(got["classes"]) == names
    for k, name in enumerate(names):
        row = got["classes"][name]
        tp, fp, fn = (int(v) for v in stage.counts[k])
        assert [row["tp"], row["fp"], row["fn"]] == [tp, fp, fn], name
        assert row["precision"] == (tp / (tp + fp) if tp + fp else None)
        assert row["recall"] == (tp / (tp + fn) if tp + fn else None)
        assert row["f1"] == (2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn else None)
        assert row["mean_matched_iou"] == pytest.approx(stage.sums[k] / tp, rel=1e-14) if tp else \
            row["mean_matched_iou"] is None
    assert got["micro"]["tp"] == int(stage.counts[:, 0].sum()) > 0 and got["micro"]["fp"] == int(stage.counts[:, 1].sum())
    assert got["micro"]["fn"] == int(stage.counts[:, 2].sum())
    assert got["iou_threshold"] == 0.5 and got["min_pixels"] == 2
    return got


def test_metrics_only_writes_object_metrics_and_leaves_metrics_json_alone(cuda, stage, tmp_path):
    on = run_metrics_only(stage, tmp_path, OBJECT_OPTIONS)
    off = run_metrics_only(stage, tmp_path, None)
    check_object_metrics(os.path.join(on, "object_metrics.json"), stage)
    assert not os.path.exists(os.path.join(off, "object_metrics.json"))
    for name in ("metrics.json", "confmat_metrics_only.npy"):
        with open(os.path.join(on, name), "rb") as f, open(os.path.join(off, name), "rb") as g:
            assert f.read() == g.read(), name


def test_write_on_batch_end_agrees_with_metrics_only(cuda, stage, tmp_path):
    from flair_hub.writer.prediction_writer import PredictionWriter
    want = check_object_metrics(os.path.join(run_metrics_only(stage, tmp_path, OBJECT_OPTIONS), "object_metrics.json"),
                                stage)
    cfg = stage_config(stage.root, OBJECT_OPTIONS)
    cfg["tasks"].update(predict=True, metrics_only=False)
    onehot = torch.nn.functional.one_hot(torch.from_numpy(np.stack(stage.preds)).long(), K)  # [B, H, W, K]
    logits = (onehot.permute(0, 3, 1, 2).float() * 8.0).contiguous().to(cuda)
    module = SimpleNamespace(device=cuda, _last_logits={TASK: logits})
    out = str(tmp_path / "batch")
    writer = PredictionWriter(cfg, out)
    writer.write_on_batch_end(None, module, None, None, {f"ID_{TASK}": stage.paths}, 0, 0)
    writer.on_predict_epoch_end(None, module)
    with open(os.path.join(out, "metrics_m", TASK, "object_metrics.json")) as f:
        assert json.load(f) == want
    assert np.array_equal(writer.object_counts[TASK], stage.counts)
