"""Host side of the reprojection feature (no GPU): the CRS parameter table and parser (flair_zonal_detection/crs.py),
CRS detection of GeoJSON zones, the lon/lat warning, reproject_zone's ring bookkeeping (the kernel stubbed by a
recording fake) and the command-line options."""
import json
import logging

import numpy as np
import pytest


def test_parameter_table_spot_values():
    from flair_zonal_detection import crs
    for code in (4326, 4171, 4258):
        assert crs.parse(code).kind == crs.GEOGRAPHIC and crs.parse(code).is_geographic
    assert crs.parse(4326).inv_flattening == 298.257223563 and crs.parse(4258).inv_flattening == 298.257222101
    l93 = crs.parse(2154)
    assert l93.parameters() == (crs.LCC2SP, 6378137.0, 298.257222101, 3.0, 46.5, 49.0, 44.0, 1.0, 700000.0, 6600000.0)
    for zone in range(42, 51):
        cc = crs.parse(3900 + zone)
        assert (cc.kind, cc.inv_flattening, cc.lon0, cc.lat0) == (crs.LCC2SP, 298.257222101, 3.0, float(zone))
        assert sorted((cc.lat1, cc.lat2)) == [zone - 0.75, zone + 0.75]
        assert (cc.false_easting, cc.false_northing) == (1700000.0, (zone - 41) * 1e6 + 200000.0)
    assert crs.parse(3946).false_northing == 5200000.0


def test_utm_zones():
    from flair_zonal_detection import crs
    for zone in range(1, 61):
        n, s = crs.parse(32600 + zone), crs.parse(32700 + zone)
        for p, fn in ((n, 0.0), (s, 10000000.0)):
            assert (p.kind, p.inv_flattening, p.lon0, p.lat0, p.k0) == (crs.TMERC, 298.257223563, 6.0 * zone - 183.0, 0.0, 0.9996)
            assert (p.false_easting, p.false_northing) == (500000.0, fn)
    for zone in range(28, 39):
        p = crs.parse(25800 + zone)
        assert (p.inv_flattening, p.lon0, p.false_northing) == (298.257222101, 6.0 * zone - 183.0, 0.0)
    grs80 = {5490: (20, 0.0), 2972: (22, 0.0), 4467: (21, 0.0), 2975: (40, 1e7), 4471: (38, 1e7)}
    for code, (zone, fn) in grs80.items():
        p = crs.parse(code)
        assert (p.kind, p.inv_flattening, p.lon0, p.k0, p.false_easting, p.false_northing) == \
            (crs.TMERC, 298.257222101, 6.0 * zone - 183.0, 0.9996, 500000.0, fn)
    assert crs.parse(5490).lon0 == -63.0 and crs.parse(2975).lon0 == 57.0 and crs.parse(32631).lon0 == 3.0


def test_parse_forms_and_refusals():
    from flair_zonal_detection import crs

    class Rasterio:
        def __init__(self, code):
            self.code = code

        def to_epsg(self):
            return self.code

    want = crs.from_epsg(2154)
    assert crs.parse("EPSG:2154") == want and crs.parse("epsg:2154") == want and crs.parse(2154) == want
    assert crs.parse(np.int64(2154)) == want and crs.parse(Rasterio(2154)) == want and crs.parse(want) is want
    assert str(want) == "EPSG:2154"
    for bad in (3857, "EPSG:27572", 32661, 25839, Rasterio(2056)):
        with pytest.raises(ValueError) as exc:
            crs.parse(bad)
        code = bad.code if isinstance(bad, Rasterio) else str(bad).replace("EPSG:", "")
        assert str(code) in str(exc.value) and "2154" in str(exc.value) and "UTM" in str(exc.value)
    for bad in (None, "Lambert-93", Rasterio(None), True, "+proj=lcc"):
        with pytest.raises(ValueError):
            crs.parse(bad)


def test_same():
    from flair_zonal_detection import crs
    assert crs.same("EPSG:2154", 2154) and crs.same(32631, "EPSG:32631")
    assert crs.same(4171, 4258)                 # equal parameter sets under two codes
    assert crs.same(4326, 4258)                 # geographic to geographic: the datum rule carries lon / lat across
    assert not crs.same(2154, 4326) and not crs.same(32631, 25831) and not crs.same(3946, 3947)
    assert not crs.same(32631, 32731)


STAR = [[2.0, 48.0], [2.001, 48.0], [2.001, 48.001], [2.0, 48.001]]


def geojson(member=None):
    g = {"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [STAR + STAR[:1]]}}]}
    if member is not None:
        g["crs"] = {"type": "name", "properties": {"name": member}}
    return g


def test_auto_detection_of_the_crs_member(tmp_path):
    from flair_zonal_detection.zone import detect_zone_crs
    assert detect_zone_crs(geojson()) == "EPSG:4326"
    assert detect_zone_crs(geojson("urn:ogc:def:crs:EPSG::2154")) == "EPSG:2154"
    assert detect_zone_crs(geojson("urn:ogc:def:crs:EPSG:9.8.1:32631")) == "EPSG:32631"
    assert detect_zone_crs(geojson("EPSG:5490")) == "EPSG:5490"
    assert detect_zone_crs(geojson("urn:ogc:def:crs:OGC:1.3:CRS84")) == "EPSG:4326"
    path = tmp_path / "zone.geojson"
    path.write_text(json.dumps(geojson("urn:ogc:def:crs:EPSG::2975")))
    assert detect_zone_crs(str(path)) == "EPSG:2975" and detect_zone_crs(path) == "EPSG:2975"
    for bad in (geojson("Lambert 93"), {**geojson(), "crs": {"type": "link"}}):
        with pytest.raises(ValueError):
            detect_zone_crs(bad)
    with pytest.raises(ValueError, match="auto"):
        detect_zone_crs((0.0, 0.0, 1.0, 1.0))  # bounds carry no CRS


class Recorder:
    """stands in for ops.reproject_points: records the calls, shifts x by 1000 and y by -1000"""

    def __init__(self):
        self.calls = []

    def __call__(self, xy, src, dst, out=None):
        assert isinstance(xy, np.ndarray) and xy.dtype == np.float64 and xy.ndim == 2 and xy.shape[1] == 2
        assert xy.flags["C_CONTIGUOUS"]
        self.calls.append((xy.copy(), str(src), str(dst)))
        return xy + [1000.0, -1000.0]


@pytest.fixture
def fake(monkeypatch):
    from flairhip import ops
    rec = Recorder()
    monkeypatch.setattr(ops, "reproject_points", rec)
    return rec


def test_reproject_zone_keeps_the_ring_structure(fake):
    from flair_zonal_detection.zone import reproject_zone, zone_rings
    outer = [[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0], [0.0, 0.0]]          # closed
    hole = [[2.0, 2.0], [4.0, 2.0], [4.0, 4.0]]                                        # open
    second = [[20.0, 0.0], [30.0, 0.0], [25.0, 8.0], [22.0, 9.0]]                      # open
    zone = {"type": "GeometryCollection", "geometries": [
        {"type": "Polygon", "coordinates": [outer, hole]}, {"type": "MultiPolygon", "coordinates": [[second]]}]}
    got = reproject_zone(zone, "EPSG:4326", 2154)
    assert len(fake.calls) == 1                                      # every ring in the one call
    xy, src, dst = fake.calls[0]
    assert (src, dst) == ("EPSG:4326", "2154") or (src, dst) == ("EPSG:4326", "EPSG:2154")
    assert xy.tolist() == outer + hole + second
    assert got["type"] == "MultiPolygon" and "crs" not in got
    before, after = zone_rings(zone), zone_rings(got)
    assert [len(p) for p in after] == [len(p) for p in before] == [2, 1]
    for pb, pa in zip(before, after):
        for rb, ra in zip(pb, pa):
            assert np.array_equal(ra, rb + [1000.0, -1000.0])        # order and vertex count kept
            assert np.array_equal(ra[0], ra[-1]) == np.array_equal(rb[0], rb[-1])  # closed stays closed, open open
    assert reproject_zone({"type": "FeatureCollection", "features": []}, 4326, 2154) == \
        {"type": "MultiPolygon", "coordinates": []} and len(fake.calls) == 1
    # a vertex without an image is an error, not a silent NaN in the mask
    fake_nan = lambda xy, s, d, out=None: np.full_like(xy, np.nan)  # noqa: E731
    from flairhip import ops
    ops.reproject_points, keep = fake_nan, ops.reproject_points
    try:
        with pytest.raises(ValueError, match="no image"):
            reproject_zone(zone, 4326, 2154)
    finally:
        ops.reproject_points = keep


def test_zone_in_raster_crs_launches_only_when_it_must(fake):
    from flair_zonal_detection.zone import zone_in_raster_crs
    zone = geojson()
    assert zone_in_raster_crs(zone, None, "EPSG:2154") is zone
    assert zone_in_raster_crs(zone, "EPSG:2154", 2154) is zone
    assert zone_in_raster_crs(geojson("urn:ogc:def:crs:EPSG::2154"), "auto", "EPSG:2154")["type"] == "FeatureCollection"
    assert zone_in_raster_crs(None, "EPSG:4326", "EPSG:2154") is None
    assert not fake.calls
    out = zone_in_raster_crs(zone, "auto", "EPSG:2154")
    assert out["type"] == "MultiPolygon" and len(fake.calls) == 1 and fake.calls[0][1:] == ("EPSG:4326", "EPSG:2154")
    for raster_crs in (None, "unknown"):
        with pytest.raises(ValueError, match="recognisable"):
            zone_in_raster_crs(zone, "EPSG:4326", raster_crs)
    with pytest.raises(ValueError, match="3857"):
        zone_in_raster_crs(zone, "EPSG:3857", "EPSG:2154")
    with pytest.raises(ValueError, match="27572"):
        zone_in_raster_crs(zone, "EPSG:4326", "EPSG:27572")


def test_lonlat_warning_fires_once_and_only_without_a_zone_crs(fake, monkeypatch, caplog):
    from flair_zonal_detection import zone as Z
    monkeypatch.setattr(Z, "_lonlat_warned", False)
    metres = (651992.4, 6860398.4, 652018.6, 6860417.8)

    def warnings():
        return [r for r in caplog.records if r.levelno == logging.WARNING and "lon/lat" in r.getMessage()]

    with caplog.at_level(logging.WARNING, logger="flair_zonal_detection.zone"):
        Z.zone_in_raster_crs(geojson(), "EPSG:4326", "EPSG:2154")     # a zone_crs: nothing to warn about
        Z.zone_in_raster_crs(geojson(), "auto", "EPSG:2154")
        Z.zone_in_raster_crs(metres, None, "EPSG:2154")               # metres on a projected raster
        Z.zone_in_raster_crs(geojson(), None, "EPSG:4326")            # degrees on a geographic raster
        Z.zone_in_raster_crs(geojson(), None, None)                   # no raster CRS to compare with
        assert not warnings()
        assert Z.zone_in_raster_crs(geojson(), None, "EPSG:2154")["type"] == "FeatureCollection"  # unchanged
        assert len(warnings()) == 1 and "zone_crs" in warnings()[0].getMessage()
        Z.zone_in_raster_crs(geojson(), None, "EPSG:2154")
        Z.zone_in_raster_crs((2.0, 48.0, 2.1, 48.1), None, "EPSG:32631")
        assert len(warnings()) == 1


def test_config_key():
    from flair_zonal_detection.config import validate_geozone_crs
    assert validate_geozone_crs({}) is None and validate_geozone_crs({"geozone_crs": None}) is None
    assert validate_geozone_crs({"geozone_crs": "auto"}) == "auto"
    assert validate_geozone_crs({"geozone_crs": "EPSG:4326"}) == "EPSG:4326"
    assert validate_geozone_crs({"geozone_crs": 32631}) == 32631
    for bad in ("EPSG:3857", 1.5, True, ["EPSG:4326"]):
        with pytest.raises(ValueError):
            validate_geozone_crs({"geozone_crs": bad})


def test_cli_options(capsys):
    from flair_zonal_detection.main import build_parser, main
    args = build_parser().parse_args(["--config", "c.yaml"])
    assert args.zone_crs is None and args.target_crs is None
    args = build_parser().parse_args(["--config", "c.yaml", "--zone", "z.geojson", "--zone-crs", "auto",
                                      "--polygons", "p.gpkg", "--target-crs", "EPSG:4326"])
    assert (args.zone, args.zone_crs, args.polygons, args.target_crs) == ("z.geojson", "auto", "p.gpkg", "EPSG:4326")
    for argv, word in ((["--zone-crs", "EPSG:4326"], "--zone"), (["--target-crs", "EPSG:4326"], "--polygons"),
                       (["--zone", "z.geojson", "--zone-crs", "EPSG:3857"], "3857"),
                       (["--polygons", "p.gpkg", "--target-crs", "auto"], "--target-crs")):
        with pytest.raises(SystemExit) as exc:
            main(["--config", "c.yaml"] + argv)   # refused while parsing: the config is never opened
        assert exc.value.code == 2 and word in capsys.readouterr().err


def test_polygon_frame_to_crs(fake):
    from flair_zonal_detection.polygons import FlatPolygons, PolygonFrame
    xy = np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [0.0, 3.0], [1.0, 1.0], [2.0, 1.0], [2.0, 2.0],
                   [10.0, 10.0], [12.0, 10.0], [12.0, 11.0]])
    flat = FlatPolygons(np.array([3, 5], np.int32), np.array([0, 2, 3], np.int32), np.array([0, 4, 7, 10], np.int32), xy)
    frame = PolygonFrame.from_flat(flat, "EPSG:2154", columns={"pixels": np.array([12, 1])})
    moved = frame.to_crs("EPSG:4326")
    assert len(fake.calls) == 1 and fake.calls[0][0].tolist() == xy.tolist()   # the flat store, once
    assert moved is not frame and frame.crs == "EPSG:2154" and moved.crs == "EPSG:4326"
    assert list(moved.columns) == list(frame.columns) and moved["pixels"].tolist() == [12, 1]
    assert np.array_equal(frame["geometry"][0].exterior[0], [0.0, 0.0])         # the old frame is untouched
    g = moved["geometry"][0]
    assert np.array_equal(g.exterior, np.array([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0], [0.0, 3.0], [0.0, 0.0]]) + [1000.0, -1000.0])
    assert len(g.interiors) == 1 and g.bounds == (1000.0, -1000.0, 1004.0, -997.0) and g.area == 12.0 - 0.5
    assert moved["geometry"][1].bounds == (1010.0, -990.0, 1012.0, -989.0)
    # a row subset still goes through the store once; the same CRS launches nothing
    fake.calls.clear()
    tail = frame[frame["class_id"] == 5].to_crs(4326)
    assert len(fake.calls) == 1 and len(tail) == 1 and tail["geometry"].iloc[0].bounds == (1010.0, -990.0, 1012.0, -989.0)
    fake.calls.clear()
    assert frame.to_crs(2154).crs == "EPSG:2154" and not fake.calls
    frame.crs = None
    with pytest.raises(ValueError):
        frame.to_crs(4326)
