"""The host side of land-cover change without a GPU: transition tables, the per-zone table from a hand-written matrix,
the config keys and the command-line options."""
import numpy as np
import pytest


def test_transition_lut_parsing_wildcards_and_precedence():
    from flair_zonal_detection.change import parse_transition, transition_lut
    assert parse_transition("*:6") == ("*", 6) and parse_transition("6:*") == (6, "*")
    assert parse_transition(" 4 : 0 ") == (4, 0) and parse_transition((4, "*")) == (4, "*")
    lut, specs = transition_lut(None, 3)  # code k = "became k"
    assert specs == [("*", 0), ("*", 1), ("*", 2)] and lut.dtype == np.uint8 and lut.shape == (4, 4)
    assert lut.tolist() == [[255, 1, 2, 255], [0, 255, 2, 255], [0, 1, 255, 255], [255, 255, 255, 255]]
    # a wildcard never covers from == to, on either side or on both
    for spec in ("*:*", "*:1", "1:*"):
        lut, _ = transition_lut([spec], 3)
        assert (np.diagonal(lut) == 255).all(), spec
    lut, _ = transition_lut(["*:*"], 3)
    assert (lut[:3, :3][~np.eye(3, dtype=bool)] == 0).all() and (lut[3] == 255).all() and (lut[:, 3] == 255).all()
    # an explicit pair means that pair, the diagonal included
    lut, _ = transition_lut(["1:1"], 3)
    assert lut[1, 1] == 0 and (lut == 0).sum() == 1
    # the earlier spec wins where two overlap
    lut, specs = transition_lut(["*:2", "1:*", "1:2", "0:1"], 3)
    assert specs == [("*", 2), (1, "*"), (1, 2), (0, 1)]
    assert lut.tolist() == [[255, 3, 0, 255], [1, 255, 0, 255], [255, 255, 255, 255], [255, 255, 255, 255]]
    assert transition_lut([], 2)[0].tolist() == [[255] * 3] * 3
    assert transition_lut(None, 32)[0].shape == (33, 33)


def test_transition_lut_errors():
    from flair_zonal_detection.change import transition_lut
    for bad in ("6", "1:2:3", "a:1", "1:-2", ":", "*:", "1.5:2", 7, ("1",), None):
        with pytest.raises(ValueError, match="transition"):
            transition_lut([bad], 19)
    with pytest.raises(ValueError, match="class 19 is not below n_classes = 19"):
        transition_lut(["*:19"], 19)
    with pytest.raises(ValueError, match="class 3"):
        transition_lut([(3, 0)], 3)
    with pytest.raises(ValueError, match="256 transitions"):
        transition_lut(["0:1"] * 256, 19)
    assert len(transition_lut(["0:1"] * 255, 19)[1]) == 255
    for K in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_classes"):
            transition_lut(None, K)
    with pytest.raises(ValueError, match="list of specs"):
        transition_lut("*:6", 19)


def test_change_table_from_a_hand_written_matrix():
    from flair_zonal_detection.change import change_table
    from flair_zonal_detection.zonal_stats import ZoneStatsTable
    counts = np.zeros((2, 3, 3), np.int64)  # K = 2; zone "b" is empty
    counts[0] = [[5, 1, 0],
                 [2, 7, 3],
                 [0, 0, 4]]
    sums = counts * 100
    sums[0, 1, 0] = 510
    t = change_table(["a", "b"], counts, sums, pixel_area=-0.04, class_names=["x", "y"], crs="EPSG:2154")
    assert isinstance(t, ZoneStatsTable) and t.n_classes == 2 and t.crs == "EPSG:2154" and t.class_names == {0: "x", 1: "y"}
    assert list(t) == ["zone", "pixels", "area", "changed", "changed_area", "changed_fraction", "stable", "gain_0",
                       "loss_0", "net_0", "gain_1", "loss_1", "net_1", "confidence_changed"]
    assert t["zone"].tolist() == ["a", "b"] and t["pixels"].tolist() == [22, 0] and t["stable"].tolist() == [16, 0]
    assert t["changed"].tolist() == [6, 0] and t["area"].tolist() == [22 * 0.04, 0.0]
    assert t["changed_area"].tolist() == [6 * 0.04, 0.0]
    assert t["changed_fraction"][0] == 6 / 22 and np.isnan(t["changed_fraction"][1])
    assert t["gain_0"].tolist() == [2, 0] and t["loss_0"].tolist() == [1, 0] and t["net_0"].tolist() == [1, 0]
    assert t["gain_1"].tolist() == [1, 0] and t["loss_1"].tolist() == [5, 0] and t["net_1"].tolist() == [-4, 0]
    assert t["confidence_changed"][0] == (100 + 510 + 300) / (255.0 * 6) and np.isnan(t["confidence_changed"][1])
    for name in ("pixels", "changed", "stable", "gain_0", "net_1"):
        assert t[name].dtype == np.int64
    long = t.transitions
    assert list(long) == ["zone", "from", "to", "pixels", "area", "confidence"]
    assert long["zone"].tolist() == ["a"] * 6
    assert long["from"].tolist() == [0, 0, 1, 1, 1, -1] and long["to"].tolist() == [0, 1, 0, 1, -1, -1]
    assert long["pixels"].tolist() == [5, 1, 2, 7, 3, 4] and long["area"].tolist() == [n * 0.04 for n in (5, 1, 2, 7, 3, 4)]
    assert long["confidence"].tolist() == [500 / (255.0 * 5), 100 / 255.0, 510 / (255.0 * 2), 700 / (255.0 * 7),
                                           300 / (255.0 * 3), 400 / (255.0 * 4)]
    plain = change_table([7, 8], counts)
    assert "confidence_changed" not in plain and "confidence" not in plain.transitions and plain["area"].tolist() == [22.0, 0.0]
    for bad in (np.zeros((2, 3)), np.zeros((2, 3, 4)), np.zeros((2, 1, 1))):
        with pytest.raises(ValueError, match="counts"):
            change_table([0, 1], bad)
    with pytest.raises(ValueError, match="identifiers"):
        change_table([0], counts)
    with pytest.raises(ValueError, match="conf_sums"):
        change_table([0, 1], counts, np.zeros((2, 3)))


def test_the_csv_writers_round_trip(tmp_path):
    import csv
    from flair_zonal_detection.change import change_table, write_change_csv, write_transitions_csv
    counts = np.zeros((2, 3, 3), np.int64)
    counts[0] = [[5, 1, 0], [2, 7, 3], [0, 0, 4]]
    t = change_table(["a", "b"], counts, counts * 7, 0.04)
    with open(write_change_csv(t, str(tmp_path / "w.csv")), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(t) and len(rows) == 3 and rows[2][0] == "b"
    assert rows[2][rows[0].index("changed_fraction")] == "nan" and int(rows[1][rows[0].index("changed")]) == 6
    assert float(rows[1][rows[0].index("changed_fraction")]) == 6 / 22
    with open(write_transitions_csv(t, str(tmp_path / "l.csv")), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["zone", "from", "to", "pixels", "area", "confidence"] and len(rows) == 7
    assert rows[5][:4] == ["a", "1", "-1", "3"] and float(rows[5][5]) == 21 / (255.0 * 3)


def test_validate_change():
    from flair_zonal_detection.config import validate_change
    assert validate_change({}) == (None, None)
    assert validate_change({"change_from": "old.tif"}) == ("old.tif", None)
    assert validate_change({"change_from": {"T": "old.tif"}, "change_transitions": ["*:6", "4:0"]}) == (
        {"T": "old.tif"}, ["*:6", "4:0"])
    for bad in (5, ["old.tif"], {"T": 5}, {3: "old.tif"}, True):
        with pytest.raises(ValueError, match="change_from"):
            validate_change({"change_from": bad})
    for bad in ("*:6", [6], ["6"], ["*:x"], {"a": 1}):
        with pytest.raises(ValueError, match="transition"):
            validate_change({"change_from": "old.tif", "change_transitions": bad})
    with pytest.raises(ValueError, match="change_transitions needs change_from"):
        validate_change({"change_transitions": ["*:6"]})


def test_validate_config_calls_validate_change(tmp_path):
    from flair_zonal_detection import config as C
    weights = tmp_path / "w.ckpt"
    weights.write_bytes(b"")
    cfg = {k: None for k in C.REQUIRED_KEYS}
    cfg.update(model_weights=str(weights), output_path=str(tmp_path / "out"))
    C.validate_config(dict(cfg))
    C.validate_config(dict(cfg, change_from="old.tif"))
    with pytest.raises(ValueError, match="change_from"):
        C.validate_config(dict(cfg, change_from=5))


def test_one_path_cannot_serve_two_class_rasters():
    from flair_zonal_detection.inference import change_source
    assert change_source("old.tif", "A", ["A"]) == "old.tif"
    assert change_source({"A": "a.tif"}, "A", ["A", "B"]) == "a.tif" and change_source({"A": "a.tif"}, "B", ["A", "B"]) is None
    with pytest.raises(ValueError, match="2 class rasters"):
        change_source("old.tif", "A", ["A", "B"])


def test_parser_options_and_errors(tmp_path, capsys):
    import yaml
    from flair_zonal_detection.main import build_parser, main
    none = build_parser().parse_args(["--config", "c.yaml"])
    assert none.change_from is None and none.change_polygons is None and none.change_transitions is None
    args = build_parser().parse_args(["--config", "c.yaml", "--change-from", "old.tif", "--change-polygons", "c.gpkg",
                                      "--change-transitions", "*:6,4:0"])
    assert (args.change_from, args.change_polygons, args.change_transitions) == ("old.tif", "c.gpkg", "*:6,4:0")
    plain = str(tmp_path / "plain.yaml")
    with open(plain, "w") as f:
        yaml.safe_dump({"output_type": "argmax"}, f)
    for argv, text in ((["--change-polygons", "c.gpkg"], "--change-polygons needs --change-from"),
                       (["--change-transitions", "*:6"], "--change-transitions needs --change-from"),
                       (["--change-from", "old.tif", "--change-transitions", "6"], "--change-transitions: transition '6'")):
        with pytest.raises(SystemExit) as exc:
            main(["--config", plain] + argv)
        assert exc.value.code == 2 and text in capsys.readouterr().err
