"""rasters_to_polygons: adjacent rasters polygonised as one.  The oracle is raster_to_polygons of the single raster
that holds the same pixels: class_id, pixels, confidence, every ring's coordinates and the order must be equal."""

import numpy as np
import pytest

from test_polygonize_gpu import _eq_frames

pytestmark = pytest.mark.gpu

RES, LEFT, TOP = 0.2, 651992.36, 6860417.84
H, W, ROW_CUT, COL_CUT = 96, 130, 41, 67
WINDOWS = [(0, 0, ROW_CUT, COL_CUT), (0, COL_CUT, ROW_CUT, W - COL_CUT), (ROW_CUT, 0, H - ROW_CUT, COL_CUT),
           (ROW_CUT, COL_CUT, H - ROW_CUT, W - COL_CUT)]
KW = dict(min_area=0.0, simplification=0.0)


def whole_map(seed=5):
    g = np.random.default_rng(seed)
    blocky = np.repeat(np.repeat(g.integers(0, 3, (H // 4 + 1, W // 4 + 1)), 4, 0), 4, 1)[:H, :W]
    cls = np.where(g.random((H, W)) < 0.1, g.integers(0, 3, (H, W)), blocky).astype(np.uint8)
    cls[cls == 0] = 18  # the default background
    return cls, g.integers(0, 256, (H, W)).astype(np.uint8)


def cut(plane, windows=WINDOWS):
    from flair_zonal_detection.raster import ArrayRaster
    return [ArrayRaster(np.ascontiguousarray(plane[r0:r0 + h, c0:c0 + w]), LEFT + c0 * RES, TOP - r0 * RES, RES)
            for r0, c0, h, w in windows]


def assert_equal_frames(a, b):
    assert len(a) == len(b) > 0
    assert list(a["class_id"]) == list(b["class_id"])
    assert list(a["pixels"]) == list(b["pixels"])
    assert np.array_equal(np.asarray(a["confidence"]), np.asarray(b["confidence"]))
    assert _eq_frames(a, b)
    assert a.crs == b.crs


def test_shuffled_parts_equal_the_whole_raster(cuda):
    from flair_zonal_detection.inference import raster_to_polygons, rasters_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls, conf = whole_map()
    whole = raster_to_polygons(ArrayRaster(cls, LEFT, TOP, RES), confidence=ArrayRaster(conf, LEFT, TOP, RES), **KW)
    parts, cparts = cut(cls), cut(conf)
    order = [2, 0, 3, 1]
    got = rasters_to_polygons([parts[i] for i in order], confidence=[cparts[i] for i in order], **KW)
    assert_equal_frames(got, whole)
    # the defaults (min_area, simplification) and the count-sized workspace go through the same tail
    dflt = raster_to_polygons(ArrayRaster(cls, LEFT, TOP, RES), confidence=ArrayRaster(conf, LEFT, TOP, RES))
    assert_equal_frames(rasters_to_polygons(parts[::-1], confidence=cparts[::-1], workspace="counted"), dflt)
    # without confidence: the same geometry, no extra columns
    plain = rasters_to_polygons(parts, **KW)
    assert _eq_frames(plain, whole) and list(plain["class_id"]) == list(whole["class_id"])


def test_parts_written_as_geotiffs(cuda, tmp_path):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.inference import raster_to_polygons, rasters_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls, conf = whole_map(6)
    paths, cpaths = [], []
    for kind, plane, out in (("cls", cls, paths), ("conf", conf, cpaths)):
        for i, ras in enumerate(cut(plane)):
            out.append(str(tmp_path / f"{kind}{i}.tif"))
            with GeoTiffWriter.like(out[-1], ras, 1) as w:
                w.data[...] = ras.data
    whole = raster_to_polygons(ArrayRaster(cls, LEFT, TOP, RES), confidence=ArrayRaster(conf, LEFT, TOP, RES), **KW)
    order = [3, 1, 0, 2]
    got = rasters_to_polygons([paths[i] for i in order], confidence=[cpaths[i] for i in order], **KW)
    assert_equal_frames(got, whole)
    # tools/polygonize_rasters.py is that call and to_file: the same rows as the whole raster's GeoPackage
    import importlib.util
    import os
    import sqlite3
    from helpers import ROOT
    spec = importlib.util.spec_from_file_location("polygonize_rasters", os.path.join(ROOT, "tools", "polygonize_rasters.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out, ref = str(tmp_path / "mosaic.gpkg"), str(tmp_path / "whole.gpkg")
    assert tool.main([out] + [paths[i] for i in order] + ["--confidence"] + [cpaths[i] for i in order]
                     + ["--min-area", "0", "--simplification", "0"]) == 0
    whole.to_file(ref, driver="GPKG")
    rows = [sqlite3.connect(p).execute(f'SELECT geom, class_id, confidence, pixels FROM "{t}" ORDER BY fid').fetchall()
            for p, t in ((out, "mosaic"), (ref, "whole"))]
    assert len(rows[0]) == len(whole) and rows[0] == rows[1]


def test_a_missing_part_is_background(cuda):
    from flair_zonal_detection.inference import raster_to_polygons, rasters_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls, conf = whole_map(7)
    holed = cls.copy()
    holed[:ROW_CUT, :COL_CUT] = 18  # the top-left part is left out: the origin comes from two other parts
    whole = raster_to_polygons(ArrayRaster(holed, LEFT, TOP, RES), confidence=ArrayRaster(conf, LEFT, TOP, RES), **KW)
    parts, cparts = cut(cls)[1:], cut(conf)[1:]
    assert_equal_frames(rasters_to_polygons(parts[::-1], confidence=cparts[::-1], **KW), whole)
    with pytest.raises(ValueError, match="ignore_background"):
        rasters_to_polygons(parts, ignore_background=False, **KW)


def test_an_object_across_the_cut_is_one_polygon(cuda):
    from flair_zonal_detection.inference import raster_to_polygons, rasters_to_polygons
    cls = np.full((H, W), 18, np.uint8)
    cls[10:21, 60:76] = 3        # 11 x 16 pixels, 7 columns left of the vertical cut and 9 right of it
    cls[14:17, 64:70] = 18       # with a hole that the cut crosses as well
    conf = np.full((H, W), 100, np.uint8)
    conf[:, COL_CUT:] = 200
    parts, cparts = cut(cls), cut(conf)
    got = rasters_to_polygons(parts, confidence=cparts, **KW)
    assert len(got) == 1 and list(got["class_id"]) == [3]
    n_left, n_right = 11 * 7 - 3 * 3, 11 * 9 - 3 * 3
    assert list(got["pixels"]) == [n_left + n_right]
    assert list(got["confidence"]) == [(100 * n_left + 200 * n_right) / (255.0 * (n_left + n_right))]
    geom = got["geometry"][0] if not hasattr(got["geometry"], "iloc") else got["geometry"].iloc[0]
    assert len(geom.interiors) == 1
    # what the driver's loop gives: each raster on its own cuts the object in two
    halves = [raster_to_polygons(p, confidence=c, **KW) for p, c in zip(parts[:2], cparts[:2])]
    assert [list(h["pixels"]) for h in halves] == [[n_left], [n_right]]
