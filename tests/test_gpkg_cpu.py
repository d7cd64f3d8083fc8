"""GeoPackage writer (flair_zonal_detection/gpkg.py, stdlib sqlite3, no GPU)."""
import sqlite3

import numpy as np
import pytest


def polys():
    ext = np.array([(651992.4, 6860417.8), (651992.4, 6860417.0), (651993.0, 6860417.0), (651993.0, 6860417.8)])
    hole = np.array([(651992.6, 6860417.4), (651992.8, 6860417.4), (651992.8, 6860417.2), (651992.6, 6860417.2)])
    tri = np.array([(0.5, 0.5), (1.5, 0.5), (1.0, 1.5)])
    return [(3, [ext, hole]), (7, [tri])]


def test_header_tables_and_integrity(tmp_path):
    from flair_zonal_detection.gpkg import APPLICATION_ID, write_polygons
    path = str(tmp_path / "a.gpkg")
    write_polygons(path, polys(), crs="EPSG:2154")
    con = sqlite3.connect(path)
    assert con.execute("PRAGMA application_id").fetchone()[0] == APPLICATION_ID == 0x47504B47
    assert con.execute("PRAGMA user_version").fetchone()[0] == 10200
    assert con.execute("PRAGMA integrity_check").fetchone()[0] == "ok"
    tables = {r[0] for r in con.execute("SELECT name FROM sqlite_master WHERE type = 'table'")}
    assert {"gpkg_spatial_ref_sys", "gpkg_contents", "gpkg_geometry_columns", "a"} <= tables
    srs = {r[1]: r for r in con.execute("SELECT * FROM gpkg_spatial_ref_sys")}
    assert set(srs) == {-1, 0, 4326, 2154}
    assert srs[2154][2:5] == ("EPSG", 2154, "undefined") and srs[4326][2] == "EPSG"
    contents = con.execute("SELECT table_name, data_type, identifier, min_x, min_y, max_x, max_y, srs_id "
                           "FROM gpkg_contents").fetchall()
    assert contents == [("a", "features", "a", 0.5, 0.5, 651993.0, 6860417.8, 2154)]
    assert con.execute("SELECT * FROM gpkg_geometry_columns").fetchall() == [("a", "geom", "POLYGON", 2154, 0, 0)]
    cols = [(r[1], r[2]) for r in con.execute('PRAGMA table_info("a")')]
    assert cols == [("fid", "INTEGER"), ("geom", "POLYGON"), ("class_id", "INTEGER")]
    con.close()


def test_blobs_parse_back(tmp_path):
    from flair_zonal_detection.gpkg import parse_blob, write_polygons
    path = str(tmp_path / "b.gpkg")
    src = polys()
    write_polygons(path, src, crs="EPSG:2154", layer="polygons")
    con = sqlite3.connect(path)
    rows = con.execute("SELECT fid, geom, class_id FROM polygons ORDER BY fid").fetchall()
    con.close()
    assert [r[0] for r in rows] == [1, 2] and [r[2] for r in rows] == [3, 7]
    for (fid, blob, cid), (c, rings) in zip(rows, src):
        assert blob[:2] == b"GP" and blob[2] == 0 and blob[3] == 0b011
        srs, env, got = parse_blob(blob)
        assert srs == 2154
        assert env == (rings[0][:, 0].min(), rings[0][:, 0].max(), rings[0][:, 1].min(), rings[0][:, 1].max())
        assert len(got) == len(rings)
        for g, r in zip(got, rings):
            assert np.array_equal(g[:-1], r) and np.array_equal(g[0], g[-1])  # closed on write, exact float64


def test_empty_result_is_a_valid_empty_layer(tmp_path):
    from flair_zonal_detection.gpkg import write_polygons
    path = str(tmp_path / "e.gpkg")
    write_polygons(path, [], crs="EPSG:2154")
    con = sqlite3.connect(path)
    assert con.execute("PRAGMA integrity_check").fetchone()[0] == "ok"
    assert con.execute('SELECT COUNT(*) FROM "e"').fetchone()[0] == 0
    assert con.execute("SELECT table_name, srs_id FROM gpkg_contents").fetchall() == [("e", 2154)]
    con.close()


def test_deterministic_bytes_and_no_crs(tmp_path):
    from flair_zonal_detection.gpkg import write_polygons
    a, b = str(tmp_path / "x.gpkg"), str(tmp_path / "y.gpkg")
    write_polygons(a, polys(), crs=None, layer="l")
    write_polygons(b, polys(), crs=None, layer="l")
    assert open(a, "rb").read() == open(b, "rb").read()
    con = sqlite3.connect(a)
    assert con.execute("SELECT srs_id FROM gpkg_geometry_columns").fetchone()[0] == -1
    con.close()


def test_polygon_frame_to_file_roundtrip(tmp_path):
    from flair_zonal_detection.gpkg import parse_blob
    from flair_zonal_detection.polygons import FlatPolygons, PolygonFrame
    ext = np.array([(0, 0), (3, 0), (3, 3), (0, 3)], float)
    hole = np.array([(1, 1), (1, 2), (2, 2), (2, 1)], float)
    flat = FlatPolygons(np.array([4], np.int32), np.array([0, 2], np.int32), np.array([0, 4, 8], np.int32),
                        np.concatenate([ext, hole]))
    df = PolygonFrame.from_flat(flat, "EPSG:2154")
    assert len(df) == 1 and df.crs == "EPSG:2154" and df["geometry"][0].area == 8.0
    assert len(df["geometry"][0].interiors) == 1
    path = str(tmp_path / "f.gpkg")
    df.to_file(path, driver="GPKG")
    con = sqlite3.connect(path)
    (blob,) = con.execute('SELECT geom FROM "f"').fetchone()
    con.close()
    assert parse_blob(blob)[2][0][:-1].tolist() == ext.tolist()
    assert df["geometry"][0].wkb == blob[40:]
    with pytest.raises(ValueError):
        df.to_file(str(tmp_path / "f.shp"), driver="ESRI Shapefile")


def test_gdal_reads_the_file(tmp_path):
    reader = None
    for name in ("pyogrio", "fiona", "osgeo.ogr"):
        try:
            reader = __import__(name, fromlist=["_"])
            break
        except ImportError:
            continue
    if reader is None:
        pytest.skip("no GDAL-based reader (pyogrio, fiona, osgeo) is installed")
    from flair_zonal_detection.gpkg import write_polygons
    path = str(tmp_path / "g.gpkg")
    write_polygons(path, polys(), crs="EPSG:2154")
    if reader.__name__ == "pyogrio":
        info = reader.read_info(path)
        assert info["features"] == 2 and info["geometry_type"] == "Polygon"
    elif reader.__name__ == "fiona":
        with reader.open(path) as f:
            assert len(f) == 2
    else:
        ds = reader.Open(path)
        assert ds.GetLayer(0).GetFeatureCount() == 2
