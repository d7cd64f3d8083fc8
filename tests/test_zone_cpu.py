"""Geozone reading without shapely / geopandas (flair_zonal_detection/zone.py) and the skip_tiles_outside_zone key."""
import json

import numpy as np
import pytest

from helpers import ROOT  # noqa: F401  (puts the package on sys.path)

OUTER = [[0.0, 0.0], [10.0, 0.0], [10.0, 8.0], [0.0, 8.0], [0.0, 0.0]]
HOLE = [[2.0, 2.0], [4.0, 2.0], [4.0, 4.0], [2.0, 4.0], [2.0, 2.0]]
OTHER = [[20.0, -3.0], [25.0, -3.0], [22.0, 5.0]]
POLYGON = {"type": "Polygon", "coordinates": [OUTER, HOLE]}
MULTI = {"type": "MultiPolygon", "coordinates": [[OUTER, HOLE], [OTHER]]}


def shapes(polys):
    return [[r.tolist() for r in rings] for rings in polys]


def test_polygon_with_a_hole():
    from flair_zonal_detection.zone import zone_bounds, zone_rings
    polys = zone_rings(POLYGON)
    assert shapes(polys) == [[OUTER, HOLE]]
    assert all(r.dtype == np.float64 and r.shape[1] == 2 for r in polys[0])
    assert zone_bounds(POLYGON) == (0.0, 0.0, 10.0, 8.0)


def test_multipolygon_feature_and_collections():
    from flair_zonal_detection.zone import zone_bounds, zone_rings
    assert shapes(zone_rings(MULTI)) == [[OUTER, HOLE], [OTHER]]
    assert zone_bounds(MULTI) == (0.0, -3.0, 25.0, 8.0)
    feature = {"type": "Feature", "properties": {"name": "z"}, "geometry": POLYGON}
    assert shapes(zone_rings(feature)) == [[OUTER, HOLE]]
    fc = {"type": "FeatureCollection", "features": [feature, {"type": "Feature", "properties": {},
                                                              "geometry": {"type": "Polygon", "coordinates": [OTHER]}}]}
    assert shapes(zone_rings(fc)) == [[OUTER, HOLE], [OTHER]]
    assert zone_bounds(fc) == (0.0, -3.0, 25.0, 8.0)
    gc = {"type": "GeometryCollection", "geometries": [MULTI, {"type": "Polygon", "coordinates": [OTHER]}]}
    assert shapes(zone_rings(gc)) == [[OUTER, HOLE], [OTHER], [OTHER]]


def test_three_dimensional_positions_lose_z():
    from flair_zonal_detection.zone import zone_rings
    ring3 = [[x, y, 7.0] for x, y in OTHER]
    assert shapes(zone_rings({"type": "Polygon", "coordinates": [ring3]})) == [[OTHER]]


def test_geojson_file(tmp_path):
    from flair_zonal_detection.zone import zone_bounds, zone_rings
    path = tmp_path / "zone.geojson"
    path.write_text(json.dumps({"type": "Feature", "properties": {}, "geometry": MULTI}))
    assert shapes(zone_rings(str(path))) == [[OUTER, HOLE], [OTHER]]
    assert shapes(zone_rings(path)) == [[OUTER, HOLE], [OTHER]]
    assert zone_bounds(str(path)) == (0.0, -3.0, 25.0, 8.0)
    with pytest.raises(ValueError):
        zone_rings(str(tmp_path / "zone.shp"))


def test_geo_interface_objects():
    from flair_zonal_detection.zone import zone_bounds, zone_rings

    class Duck:
        def __init__(self, geo):
            self.__geo_interface__ = geo

    # shapely hands out tuples, not lists
    geo = {"type": "Polygon", "coordinates": (tuple(map(tuple, OUTER)), tuple(map(tuple, HOLE)))}
    assert shapes(zone_rings(Duck(geo))) == [[OUTER, HOLE]]
    assert zone_bounds(Duck(MULTI)) == (0.0, -3.0, 25.0, 8.0)


def test_bounds_tuple_is_a_box():
    from flair_zonal_detection.zone import zone_bounds, zone_rings
    polys = zone_rings((1.0, 2.0, 5.0, 9.0))
    assert shapes(polys) == [[[[1.0, 2.0], [5.0, 2.0], [5.0, 9.0], [1.0, 9.0]]]]
    assert zone_bounds((1.0, 2.0, 5.0, 9.0)) == (1.0, 2.0, 5.0, 9.0)
    assert zone_bounds([1, 2, 5, 9]) == (1.0, 2.0, 5.0, 9.0)


def test_nested_sequences(tmp_path):
    from flair_zonal_detection.zone import zone_bounds, zone_rings
    path = tmp_path / "z.json"
    path.write_text(json.dumps({"type": "Polygon", "coordinates": [OTHER]}))
    nested = [POLYGON, [(30.0, 30.0, 31.0, 32.0), [str(path)]]]
    polys = zone_rings(nested)
    assert shapes(polys)[0] == [OUTER, HOLE] and shapes(polys)[2] == [OTHER] and len(polys) == 3
    assert zone_bounds(nested) == (0.0, -3.0, 31.0, 32.0)
    assert zone_rings([]) == []
    with pytest.raises(ValueError):
        zone_bounds([])


@pytest.mark.parametrize("bad", [
    {"type": "LineString", "coordinates": [[0.0, 0.0], [1.0, 1.0]]},
    {"type": "Feature", "properties": {}, "geometry": {"type": "Point", "coordinates": [0.0, 0.0]}},
    {"type": "Feature", "properties": {}, "geometry": None},
    {"type": "Polygon", "coordinates": [[[0.0, 0.0], [1.0, 1.0]]]},
    {"no": "type"},
    42,
    3.5,
    object(),
    b"bytes",
    [POLYGON, 42],
], ids=["linestring", "point-feature", "empty-feature", "two-point-ring", "untyped-dict", "int", "float", "object",
        "bytes", "sequence-with-garbage"])
def test_garbage_raises_value_error(bad):
    from flair_zonal_detection.zone import zone_rings
    with pytest.raises(ValueError):
        zone_rings(bad)


def test_error_names_the_type():
    from flair_zonal_detection.zone import zone_rings
    with pytest.raises(ValueError, match="complex"):
        zone_rings(1j)


def test_rings_to_pixels():
    from flair_zonal_detection.zone import rings_to_pixels
    rings = [np.array(OUTER), np.array(OTHER)]
    pix, offsets = rings_to_pixels(rings, left=-2.0, top=10.0, xres=0.5, yres=0.25)
    assert offsets.tolist() == [0, 5, 8] and offsets.dtype == np.int32
    assert pix.dtype == np.float64 and pix[1].tolist() == [24.0, 40.0] and pix[7].tolist() == [48.0, 20.0]


def test_slicing_zone_bounds_reads_every_form(tmp_path):
    """slicing._zone_bounds: objects with .bounds and bounds tuples as before, every other form through zone_bounds"""
    from flair_zonal_detection.raster import ArrayRaster
    from flair_zonal_detection.slicing import _zone_bounds
    ras = ArrayRaster(np.zeros((1, 100, 200), np.uint8), 1000.0, 5000.0, 0.5)   # x 1000..1100, y 4950..5000
    box = (1010.2, 4960.3, 1030.7, 4990.1)
    want = _zone_bounds(ras, box)
    l, b, r, t = box
    poly = {"type": "Polygon", "coordinates": [[[l, b], [r, b], [r, t], [l, t], [l, b]]]}
    path = tmp_path / "z.geojson"
    path.write_text(json.dumps(poly))

    class WithBounds:
        bounds = box

    class Duck:
        __geo_interface__ = poly

    for form in (poly, str(path), Duck(), WithBounds(), [WithBounds()], [poly], [Duck(), poly]):
        assert _zone_bounds(ras, form) == want
    assert _zone_bounds(ras, {"type": "Polygon", "coordinates": [[[0, 0], [1, 0], [1, 1]]]}) is None


@pytest.mark.parametrize("bad", [1, 0, "true", "yes", None, [True]])
def test_skip_tiles_outside_zone_must_be_a_bool(bad):
    from flair_zonal_detection.config import validate_config, validate_skip_tiles_outside_zone
    with pytest.raises(ValueError, match="skip_tiles_outside_zone"):
        validate_skip_tiles_outside_zone({"skip_tiles_outside_zone": bad})
    cfg = {k: 1 for k in ("output_path", "output_name", "model_weights", "img_pixels_detection", "margin",
                          "modalities", "tasks", "output_px_meters")}
    cfg["skip_tiles_outside_zone"] = bad
    with pytest.raises(ValueError, match="skip_tiles_outside_zone"):
        validate_config(cfg)


def test_skip_tiles_outside_zone_defaults_to_false():
    from flair_zonal_detection.config import validate_skip_tiles_outside_zone
    assert validate_skip_tiles_outside_zone({}) is False
    assert validate_skip_tiles_outside_zone({"skip_tiles_outside_zone": True}) is True
    assert validate_skip_tiles_outside_zone({"skip_tiles_outside_zone": False}) is False


def test_tile_zone_windows_snap_outward_and_grow_by_a_pixel():
    import pandas as pd
    from flair_zonal_detection.inference import tile_zone_windows
    tiles = pd.DataFrame({"left": [10.0, 10.25], "bottom": [80.0, 79.9], "right": [20.0, 20.1], "top": [90.0, 90.0]})
    win = tile_zone_windows(tiles, left=0.0, top=100.0, xres=0.5, yres=0.5)
    # rows from the top: y 90 -> row 20, y 80 -> row 40, y 79.9 -> 40.2 -> 41; columns: x 10 -> 20, 10.25 -> 20.5 -> 20
    assert win.tolist() == [[19, 19, 41, 41], [19, 19, 42, 42]]
