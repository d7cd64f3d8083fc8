"""Host side of the per-polygon confidence (no GPU): extra attribute columns in the GeoPackage writer and in
PolygonFrame, config validation of write_confidence, argument validation of the fork-named helpers."""
import sqlite3

import numpy as np
import pytest


def polys():
    ext = np.array([(651992.4, 6860417.8), (651992.4, 6860417.0), (651993.0, 6860417.0), (651993.0, 6860417.8)])
    hole = np.array([(651992.6, 6860417.4), (651992.8, 6860417.4), (651992.8, 6860417.2), (651992.6, 6860417.2)])
    tri = np.array([(0.5, 0.5), (1.5, 0.5), (1.0, 1.5)])
    return [(3, [ext, hole]), (7, [tri])]


def test_gpkg_extra_columns_round_trip(tmp_path):
    from flair_zonal_detection.gpkg import parse_blob, write_polygons
    path = str(tmp_path / "c.gpkg")
    conf = np.array([0.1 + 0.2, 1.0 / 3.0])   # values with no short decimal form: REAL keeps the float64 bits
    pix = np.array([12, 2 ** 40], np.int64)
    write_polygons(path, polys(), crs="EPSG:2154", columns={"confidence": conf, "pixels": pix})
    con = sqlite3.connect(path)
    assert con.execute("PRAGMA integrity_check").fetchone()[0] == "ok"
    cols = [(r[1], r[2]) for r in con.execute('PRAGMA table_info("c")')]
    assert cols == [("fid", "INTEGER"), ("geom", "POLYGON"), ("class_id", "INTEGER"), ("confidence", "REAL"),
                    ("pixels", "INTEGER")]
    rows = con.execute('SELECT fid, geom, class_id, confidence, pixels FROM "c" ORDER BY fid').fetchall()
    con.close()
    assert [(r[0], r[2], r[3], r[4]) for r in rows] == [(1, 3, conf[0], 12), (2, 7, conf[1], 2 ** 40)]
    assert all(isinstance(r[3], float) and isinstance(r[4], int) for r in rows)
    assert np.array_equal(parse_blob(rows[1][1])[2][0][:-1], polys()[1][1][0])


def test_gpkg_without_columns_writes_the_same_bytes_as_before(tmp_path):
    from flair_zonal_detection.gpkg import write_polygons
    a, b = str(tmp_path / "t.gpkg"), str(tmp_path / "u" / "t.gpkg")
    (tmp_path / "u").mkdir()
    write_polygons(a, polys(), crs="EPSG:2154")
    write_polygons(b, polys(), crs="EPSG:2154", columns={})
    assert open(a, "rb").read() == open(b, "rb").read()
    con = sqlite3.connect(a)
    assert [(r[1], r[2]) for r in con.execute('PRAGMA table_info("t")')] == \
        [("fid", "INTEGER"), ("geom", "POLYGON"), ("class_id", "INTEGER")]
    con.close()


def test_gpkg_rejects_bad_columns(tmp_path):
    from flair_zonal_detection.gpkg import write_polygons
    path = str(tmp_path / "d.gpkg")
    with pytest.raises(ValueError):
        write_polygons(path, polys(), columns={"confidence": np.array([0.5])})          # one value, two polygons
    with pytest.raises(ValueError):
        write_polygons(path, polys(), columns={"confidence": np.array([0.5, 0.1, 0.2])})
    with pytest.raises(ValueError):
        write_polygons(path, polys(), columns={"name": np.array(["a", "b"])})           # neither float nor int
    with pytest.raises(ValueError):
        write_polygons(path, polys(), columns={"class_id": np.array([1, 2])})           # taken
    with pytest.raises(ValueError):
        write_polygons(path, polys(), columns={'x" INTEGER); --': np.array([1, 2])})    # not an identifier


def flat_polygons():
    from flair_zonal_detection.polygons import FlatPolygons
    src = polys()
    rings = [r for _, rs in src for r in rs]
    return FlatPolygons(np.array([3, 7], np.int32), np.array([0, 2, 3], np.int32),
                        np.cumsum([0] + [len(r) for r in rings]).astype(np.int32), np.concatenate(rings))


def test_polygon_frame_carries_extra_columns(tmp_path):
    from flair_zonal_detection.polygons import PolygonFrame
    flat = flat_polygons()
    plain = PolygonFrame.from_flat(flat, "EPSG:2154")
    assert list(plain.columns) == ["class_id", "geometry"]
    conf, pix = np.array([0.25, 0.75]), np.array([5, 9], np.int64)
    df = PolygonFrame.from_flat(flat, "EPSG:2154", columns={"confidence": conf, "pixels": pix})
    assert list(df.columns) == ["class_id", "confidence", "pixels", "geometry"] and df.crs == "EPSG:2154"
    assert df["confidence"].dtype == np.float64 and df["pixels"].dtype == np.int64
    sub = df[df["confidence"] > 0.5]                    # still a PolygonFrame with its crs and columns
    assert isinstance(sub, PolygonFrame) and sub.crs == "EPSG:2154" and list(sub["pixels"]) == [9]
    path = str(tmp_path / "f.gpkg")
    df.to_file(path, driver="GPKG")
    con = sqlite3.connect(path)
    assert con.execute('SELECT class_id, confidence, pixels FROM "f" ORDER BY fid').fetchall() == \
        [(3, 0.25, 5), (7, 0.75, 9)]
    con.close()
    sub_path = str(tmp_path / "s.gpkg")
    sub.to_file(sub_path, driver="GPKG")
    con = sqlite3.connect(sub_path)
    assert con.execute('SELECT fid, class_id, confidence, pixels FROM "s"').fetchall() == [(1, 7, 0.75, 9)]
    con.close()
    with pytest.raises(ValueError):
        PolygonFrame.from_flat(flat, None, columns={"confidence": np.array([0.5])})
    # a frame without the columns writes the table it always wrote
    plain_path = str(tmp_path / "p.gpkg")
    plain.to_file(plain_path, driver="GPKG")
    con = sqlite3.connect(plain_path)
    assert [r[1] for r in con.execute('PRAGMA table_info("p")')] == ["fid", "geom", "class_id"]
    con.close()


def test_write_confidence_config_validation(tmp_path):
    from flair_zonal_detection.config import REQUIRED_KEYS, validate_config, validate_write_confidence
    assert validate_write_confidence({}) is False
    assert validate_write_confidence({"write_confidence": False, "output_type": "class_prob"}) is False
    assert validate_write_confidence({"write_confidence": True}) is True                 # output_type defaults to argmax
    assert validate_write_confidence({"write_confidence": True, "output_type": "argmax"}) is True
    for bad in ("true", 1, 0, None, [True]):
        with pytest.raises(ValueError):
            validate_write_confidence({"write_confidence": bad})
    with pytest.raises(ValueError):
        validate_write_confidence({"write_confidence": True, "output_type": "class_prob"})
    # through validate_config, before it looks for the checkpoint
    weights = tmp_path / "w.ckpt"
    weights.write_bytes(b"")
    cfg = {k: None for k in REQUIRED_KEYS}
    cfg.update({"model_weights": str(weights), "output_path": str(tmp_path / "out")})
    validate_config(dict(cfg))
    validate_config(dict(cfg, write_confidence=True))
    with pytest.raises(ValueError):
        validate_config(dict(cfg, write_confidence=True, output_type="class_prob"))
    with pytest.raises(ValueError):
        validate_config(dict(cfg, write_confidence="yes", model_weights=str(tmp_path / "missing.ckpt")))


def test_polygon_source_ignores_confidence_entries():
    from flair_zonal_detection.inference import _polygon_source
    from flair_zonal_detection.raster import ArrayRaster
    a = ArrayRaster(np.zeros((1, 4, 4), np.uint8), 0.0, 4.0, 1.0)
    c = ArrayRaster(np.zeros((1, 4, 4), np.uint8), 0.0, 4.0, 1.0)
    assert _polygon_source({"task": a}) is a
    assert _polygon_source({"task_confidence": c, "task": a}) is a
    assert _polygon_source({"AERIAL_LABEL-COSIA": a, "AERIAL_LABEL-COSIA_confidence": c, "other": c}) is a
    with pytest.raises(KeyError):
        _polygon_source({"t1": a, "t2": a, "t1_confidence": c})


def test_logits_to_labels_and_confidence():
    import torch
    from flair_zonal_detection.inference import logits_to_labels_and_confidence
    g = np.random.default_rng(2)
    probs = g.random((5, 7, 9)).astype(np.float32)
    probs[:, 0, 0] = 0.5   # ties: first maximum
    labels, conf = logits_to_labels_and_confidence(probs)
    assert labels.dtype == np.uint8 and labels.shape == (7, 9) and np.array_equal(labels, probs.argmax(0))
    assert labels[0, 0] == 0 and conf.dtype == np.float32 and np.array_equal(conf, probs.max(0))
    lt, ct = logits_to_labels_and_confidence(torch.from_numpy(probs))
    assert np.array_equal(lt, labels) and np.array_equal(ct, conf)
    u8 = (probs * 255).astype(np.uint8)
    assert logits_to_labels_and_confidence(u8)[1].dtype == np.uint8
    with pytest.raises(ValueError):
        logits_to_labels_and_confidence(probs[0])
    with pytest.raises(ValueError):
        logits_to_labels_and_confidence(np.zeros((257, 2, 2), np.float32))


def test_vectorize_segmentation_parallel_argument_validation():
    import inspect
    from flair_zonal_detection.inference import quantize_confidence, vectorize_segmentation_parallel as vsp
    sig = inspect.signature(vsp)
    assert list(sig.parameters) == ["labels", "confidence", "transform", "n_jobs", "simplification_tolerance",
                                    "min_area", "crs"]
    assert [sig.parameters[k].default for k in ("n_jobs", "simplification_tolerance", "min_area", "crs")] == \
        [4, 1.0, 4.0, "EPSG:5490"]
    labels = np.zeros((4, 6), np.uint8)
    conf = np.zeros((4, 6), np.uint8)
    t = (1.0, 0.0, 10.0, 0.0, -1.0, 20.0)
    with pytest.raises(ValueError):
        vsp(labels.astype(np.int32), conf, t)
    with pytest.raises(ValueError):
        vsp(labels[None], conf, t)
    with pytest.raises(ValueError):
        vsp(labels, conf[:, :-1], t)
    with pytest.raises(ValueError):
        vsp(labels, conf.astype(np.int16), t)
    with pytest.raises(ValueError):
        vsp(labels, np.full((4, 6), 1.5), t)
    with pytest.raises(ValueError):
        vsp(labels, np.full((4, 6), np.nan), t)
    with pytest.raises(ValueError):
        vsp(labels, conf, (1.0, 0.0, 10.0, 0.0, 1.0, 20.0))      # south-up
    with pytest.raises(ValueError):
        vsp(labels, conf, (1.0, 0.1, 10.0, 0.0, -1.0, 20.0))     # rotated
    with pytest.raises(ValueError):
        vsp(labels, conf, (1.0, 0.0, 10.0))
    with pytest.raises(ValueError):
        vsp(labels, conf, 3.0)
    q = quantize_confidence(np.array([0.0, 0.5, 1.0, 0.2, 2.5 / 255.0, 3.5 / 255.0]))
    assert q.dtype == np.uint8 and q.tolist() == [0, 128, 255, 51, 2, 4]   # rint: half to even
    u = np.arange(6, dtype=np.uint8)
    assert quantize_confidence(u) is u
