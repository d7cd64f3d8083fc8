"""The host side of zonal statistics: zone.zone_features, the window rule, the chunk list, the batch split
(flairhip.ops.zone_stats_*), the table arithmetic and the writers of flair_zonal_detection.zonal_stats.  No GPU: nothing
here loads the library."""
import csv
import json

import numpy as np
import pytest

from zone_stats_oracle import CENTRE_BOX, H0, STAR, STAR_HOLE, W0, oracle_masks, parcel_grid, random_polygons, window_rule


def closed(ring):
    return np.vstack([ring, ring[:1]]).tolist()


# ---- zone_features -----------------------------------------------------------------------------------------------------

def test_zone_features_reads_features_multipolygons_collections_bounds_and_sequences(tmp_path):
    from flair_zonal_detection.zone import zone_features, zone_rings
    poly = {"type": "Polygon", "coordinates": [closed(STAR), closed(STAR_HOLE)]}
    multi = {"type": "MultiPolygon", "coordinates": [[closed(CENTRE_BOX)], [closed(CENTRE_BOX + 50.0)]]}
    f1 = {"type": "Feature", "properties": {"id": "A7", "owner": 3}, "geometry": poly}
    f2 = {"type": "Feature", "properties": None, "geometry": multi}
    (props, rings), = zone_features(f1)
    assert props == {"id": "A7", "owner": 3} and len(rings) == 2
    assert np.array_equal(rings[0], np.asarray(closed(STAR))) and rings[0].dtype == np.float64
    (props, rings), = zone_features(f2)  # a MultiPolygon is one zone holding the rings of all its parts
    assert props == {} and len(rings) == 2 and np.array_equal(rings[1][:4], CENTRE_BOX + 50.0)
    coll = {"type": "FeatureCollection", "features": [f1, f2]}
    got = zone_features(coll)
    assert [p for p, _ in got] == [{"id": "A7", "owner": 3}, {}] and [len(r) for _, r in got] == [2, 2]
    # a bare geometry and a bounds tuple: one zone each, no properties
    (props, rings), = zone_features(multi)
    assert props == {} and len(rings) == 2
    (props, rings), = zone_features((1.0, 2.0, 5.0, 7.0))
    assert props == {} and np.array_equal(rings[0], [[1, 2], [5, 2], [5, 7], [1, 7]])
    # sequences concatenate; a file reads like its dict
    path = tmp_path / "zones.geojson"
    path.write_text(json.dumps(coll))
    got = zone_features([str(path), (0.0, 0.0, 1.0, 1.0), f1])
    assert [len(r) for _, r in got] == [2, 2, 1, 2] and got[3][0]["id"] == "A7"
    assert zone_features([]) == [] and zone_features({"type": "FeatureCollection", "features": []}) == []
    # zone_rings stays as it is: the same layer as one contour, polygon by polygon
    assert [len(p) for p in zone_rings(coll)] == [2, 1, 1]


def test_zone_features_refuses_what_is_not_polygonal():
    from flair_zonal_detection.zone import zone_features
    with pytest.raises(ValueError, match="Polygon"):
        zone_features({"type": "Feature", "properties": {}, "geometry": {"type": "Point", "coordinates": [1.0, 2.0]}})
    with pytest.raises(ValueError, match="polygonal"):
        zone_features({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})
    with pytest.raises(ValueError, match="geometry"):
        zone_features({"type": "Feature", "properties": {}, "geometry": None})
    with pytest.raises(ValueError):
        zone_features(3.5)
    with pytest.raises(ValueError, match="geojson"):
        zone_features("zones.gpkg")


# ---- windows -----------------------------------------------------------------------------------------------------------

def mixed_zones():
    outside = CENTRE_BOX + [500.0, 0.0]
    larger = np.array([[-9.0, -7.0], [W0 + 8.0, -7.0], [W0 + 8.0, H0 + 6.0], [-9.0, H0 + 6.0]])
    return [[STAR, STAR_HOLE], [CENTRE_BOX], [outside], [larger], []] + [[p] for p in random_polygons()]


def test_window_rule_alignment_and_clamping():
    from flairhip import ops
    zones = mixed_zones()
    xy, ro, zro = ops.zone_stats_flatten(zones)
    assert xy.dtype == np.float64 and ro.dtype == np.int32 and zro.dtype == np.int32
    assert zro.tolist()[:6] == [0, 2, 3, 4, 5, 5] and ro[-1] == len(xy) and len(zro) == len(zones) + 1
    win = ops.zone_stats_windows(xy, ro, zro, H0, W0)
    assert win.dtype == np.int32 and win.shape == (len(zones), 4)
    for z, rings in enumerate(zones):
        want = window_rule(rings, H0, W0)
        assert tuple(win[z]) == (want if want is not None else (0, 0, 0, 0)), z
    assert np.all(win[:, 1] % 32 == 0) and np.all(win >= 0)
    assert np.all(win[:, 2] <= H0) and np.all(win[:, 3] <= W0)
    # corners on pixel centres (10.5, 20.5) .. (30.5, 40.5): rows 20..39, columns 11..30 lie inside the window
    assert tuple(win[1]) == (20, 0, 41, 32)
    assert tuple(win[3]) == (0, 0, H0, W0)            # larger than the raster: clamped to it
    assert tuple(win[2]) == (20, 128, 41, W0)          # wholly to the right: the aligned c0 leaves the last word
    rows, ww, words = ops.zone_stats_plane_words(win)
    assert words[2] == 21 and words[4] == 0 and rows[4] == 0 and ww[4] == 0
    below = ops.zone_stats_windows(*ops.zone_stats_flatten([[CENTRE_BOX + [0.0, 300.0]]]), H0, W0)
    assert below[0][0] == below[0][2] == H0 and ops.zone_stats_plane_words(below)[2][0] == 0  # below: no rows
    assert words[3] == H0 * 5 and words[1] == 21
    # the rule loses no member pixel
    for z, m in enumerate(oracle_masks(zones, H0, W0)):
        r0, c0, r1, c1 = win[z]
        m = m.copy()
        m[r0:r1, c0:c1] = False
        assert not m.any(), z
    # coordinates far beyond int32 clamp, they do not wrap
    far = [[np.array([[-1e300, -1e18], [1e300, -1e18], [1e300, 1e18], [-1e300, 1e18]])]]
    assert tuple(ops.zone_stats_windows(*ops.zone_stats_flatten(far), 7, 40)[0]) == (0, 0, 7, 40)
    with pytest.raises(ValueError, match="zone 1"):
        ops.zone_stats_flatten([[CENTRE_BOX], [np.zeros((4, 3))]])


# ---- chunks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 7, 64, 2048])
def test_chunks_cover_every_word_once_within_one_zone_and_the_cap(cap):
    from flairhip import ops
    Wb = 420  # wide enough for a window beyond the lane-per-row regime of the scan
    across = np.array([[-9.0, -7.0], [Wb + 8.0, -7.0], [Wb + 8.0, H0 + 6.0], [-9.0, H0 + 6.0]])
    zones = mixed_zones() + parcel_grid()[:40] + [[across]]
    win = ops.zone_stats_windows(*ops.zone_stats_flatten(zones), H0, Wb)
    rows, ww, words = ops.zone_stats_plane_words(win)
    offsets, total, scan_starts, chunks = ops.zone_stats_plan(win, cap)
    assert offsets.dtype == np.int64 and scan_starts.dtype == np.int64 and chunks.dtype == np.int32
    assert total == int(words.sum()) and offsets.tolist() == (np.cumsum(words) - words).tolist()
    assert chunks.shape[1] == 3 and np.all(chunks[:, 2] >= 1) and np.all(chunks[:, 2] <= cap)
    seen = np.zeros(total, np.int64)
    for z, first, n in chunks:
        assert 0 <= first and first + n <= words[z]  # none crosses its zone
        seen[offsets[z] + first:offsets[z] + first + n] += 1
    assert np.all(seen == 1)
    assert np.all(np.diff(chunks[:, 0]) >= 0)
    # row-scan items: a lane per row up to NARROW words per row, a wave per row beyond
    items = np.diff(scan_starts)
    assert scan_starts[0] == 0 and len(scan_starts) == len(zones) + 1
    narrow = (ww > 0) & (ww <= ops.ZONE_STATS_NARROW_WORDS)
    assert narrow.any() and (ww > ops.ZONE_STATS_NARROW_WORDS).any()
    assert np.array_equal(items[narrow], (rows[narrow] + 63) // 64)
    assert np.array_equal(items[ww > ops.ZONE_STATS_NARROW_WORDS], rows[ww > ops.ZONE_STATS_NARROW_WORDS])
    assert np.all(items[ww == 0] == 0)


def test_plan_of_no_zone_and_of_empty_zones():
    from flairhip import ops
    offsets, total, scan_starts, chunks = ops.zone_stats_plan(np.zeros((0, 4), np.int32))
    assert total == 0 and len(offsets) == 0 and scan_starts.tolist() == [0] and chunks.shape == (0, 3)
    offsets, total, scan_starts, chunks = ops.zone_stats_plan(np.array([[0, 0, 0, 0], [5, 32, 5, 64], [3, 64, 9, 64]]))
    assert total == 0 and offsets.tolist() == [0, 0, 0] and scan_starts.tolist() == [0, 0, 0, 0] and len(chunks) == 0


# ---- batches -----------------------------------------------------------------------------------------------------------

def test_batch_split():
    from flairhip import ops
    words = np.array([10, 0, 20, 30, 0, 0, 5, 40, 1])
    assert ops.zone_stats_batches(words, 4 * 1000) == [(0, 9)]
    assert ops.zone_stats_batches(words, 4 * 40) == [(0, 3), (3, 7), (7, 8), (8, 9)]
    assert ops.zone_stats_batches(words, 4 * 40 + 3) == [(0, 3), (3, 7), (7, 8), (8, 9)]  # whole words only
    assert ops.zone_stats_batches(words, 4 * 60) == [(0, 6), (6, 9)]  # 10 + 0 + 20 + 30 + 0 + 0, then 5 + 40 + 1
    assert ops.zone_stats_batches([], 0) == [] and ops.zone_stats_batches([0, 0], 0) == [(0, 2)]
    for budget in (160, 240, 400, 4000):
        got = ops.zone_stats_batches(words, budget)
        assert got[0][0] == 0 and got[-1][1] == len(words)
        assert all(a[1] == b[0] for a, b in zip(got, got[1:])) and all(a < b for a, b in got)
        assert all(4 * words[a:b].sum() <= budget for a, b in got)
    with pytest.raises(ValueError, match="zone 7"):
        ops.zone_stats_batches(words, 4 * 39)


# ---- the table ---------------------------------------------------------------------------------------------------------

COUNTS = np.array([[5, 9, 9, 2],      # a tie between classes 1 and 2: the smaller wins
                   [0, 0, 0, 0],      # empty
                   [0, 0, 0, 6],      # only "other" pixels: no class has the majority
                   [7, 0, 1, 0]], dtype=np.int64)
SUMS = np.array([[500, 2295, 0, 510], [0, 0, 0, 0], [0, 0, 0, 1530], [1785, 0, 100, 0]], dtype=np.int64)


def test_table_arithmetic():
    from flair_zonal_detection.zonal_stats import stats_table
    t = stats_table(np.array(["a", "b", "c", "d"]), COUNTS, SUMS, pixel_area=-0.2 * 0.2, class_names=["x", "y", "z"],
                    crs="EPSG:2154")
    assert t.columns == ["zone", "pixels", "area", "pixels_0", "area_0", "pixels_1", "area_1", "pixels_2", "area_2",
                         "other", "majority", "confidence", "confidence_0", "confidence_1", "confidence_2"]
    assert t.n_zones == 4 and t.n_classes == 3 and t.class_names == {0: "x", 1: "y", 2: "z"} and t.crs == "EPSG:2154"
    assert t["zone"].tolist() == ["a", "b", "c", "d"]
    assert t["pixels"].tolist() == [25, 0, 6, 8] and t["pixels"].dtype == np.int64
    assert t["area"].tolist() == [25 * (0.2 * 0.2), 0.0, 6 * (0.2 * 0.2), 8 * (0.2 * 0.2)]
    assert t["pixels_1"].tolist() == [9, 0, 0, 0] and t["area_2"].tolist() == [9 * (0.2 * 0.2), 0.0, 0.0, 0.2 * 0.2]
    assert t["other"].tolist() == [2, 0, 6, 0]
    assert t["majority"].tolist() == [1, -1, -1, 0]
    conf = t["confidence"]
    assert conf[0] == 3305 / (255.0 * 25) and np.isnan(conf[1]) and conf[2] == 1.0 and conf[3] == 1885 / (255.0 * 8)
    assert t["confidence_1"][0] == 1.0 and t["confidence_2"][0] == 0.0 and np.isnan(t["confidence_2"][1])
    assert np.isnan(t["confidence_0"][2]) and t["confidence_0"][3] == 1.0
    # without confidence sums the confidence columns are absent
    plain = stats_table(np.arange(4), COUNTS)
    assert plain.columns == t.columns[:11] and plain["zone"].tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        stats_table(np.arange(3), COUNTS)
    with pytest.raises(ValueError):
        stats_table(np.arange(4), COUNTS, SUMS[:, :3])


def test_csv_and_json_writers(tmp_path):
    from flair_zonal_detection.zonal_stats import stats_table, write_zone_stats_csv, write_zone_stats_json
    t = stats_table(np.array(["a,1", "b", "c", "d"]), COUNTS, SUMS, pixel_area=0.2 * 0.2, class_names={0: "x", 2: "z"})
    path = write_zone_stats_csv(t, str(tmp_path / "t.csv"))
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == t.columns and len(rows) == 5
    for c, name in enumerate(t.columns):
        col = [r[c] for r in rows[1:]]
        if name == "zone":
            assert col == ["a,1", "b", "c", "d"]
        elif t[name].dtype.kind == "i":
            assert [int(v) for v in col] == t[name].tolist()
        else:  # floats read back as the same float64; NaN as nan
            assert np.array_equal(np.array([float(v) for v in col]), t[name], equal_nan=True), name
    assert rows[2][t.columns.index("confidence")] == "nan"
    doc = json.load(open(write_zone_stats_json(t, str(tmp_path / "t.json"))))
    assert doc["columns"] == t.columns and doc["n_classes"] == 3 and doc["class_names"] == {"0": "x", "2": "z"}
    assert doc["zones"][0]["pixels"] == 25 and doc["zones"][1]["confidence"] is None and doc["zones"][1]["majority"] == -1
    assert doc["zones"][3]["confidence_0"] == 1.0 and doc["zones"][0]["zone"] == "a,1"


def test_zone_stats_config_keys():
    from flair_zonal_detection.config import validate_zone_stats
    from flair_zonal_detection.main import build_parser
    assert validate_zone_stats({}) == (None, None, None)
    assert validate_zone_stats({"zone_stats": "p.geojson", "zone_stats_id": "id", "zone_stats_crs": "EPSG:4326"}) == (
        "p.geojson", "id", "EPSG:4326")
    assert validate_zone_stats({"zone_stats_crs": "auto"})[2] == "auto"
    for bad in ({"zone_stats": 3}, {"zone_stats_id": 7}, {"zone_stats_crs": True}, {"zone_stats_crs": "EPSG:1"}):
        with pytest.raises(ValueError):
            validate_zone_stats(bad)
    args = build_parser().parse_args(["--config", "c.yaml", "--zone-stats", "z.geojson", "--zone-stats-id", "id",
                                      "--zone-stats-crs", "EPSG:4326"])
    assert (args.zone_stats, args.zone_stats_id, args.zone_stats_crs) == ("z.geojson", "id", "EPSG:4326")
    none = build_parser().parse_args(["--config", "c.yaml"])
    assert (none.zone_stats, none.zone_stats_id, none.zone_stats_crs) == (None, None, None)
