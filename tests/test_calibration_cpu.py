"""flairhip.calibration (numpy on the [K, 2, 256] score histograms, the threshold file) and the zonal configuration keys
that put a threshold file into effect.  No GPU."""
import logging
import os

import numpy as np
import pytest
import yaml

import helpers  # noqa: F401  (puts the package on the path)
from flairhip import calibration as cal


def _random_hist(seed, K=5, top=40):
    g = np.random.default_rng(seed)
    h = g.integers(0, top, (K, 2, 256)).astype(np.int64)
    h[g.random((K, 2, 256)) < 0.6] = 0  # sparse, like real score histograms
    return h


# ---- sweep ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sweep_equals_a_brute_force_loop(seed):
    h = _random_hist(seed)
    h[3] = 0  # a class without any pixel: every ratio is 0 / 0 = 0
    s = cal.sweep(h)
    q = np.arange(256)
    for k in range(h.shape[0]):
        for t in range(256):
            tp = int(h[k, 1][q >= t].sum())
            fp = int(h[k, 0][q >= t].sum())
            fn = int(h[k, 1][q < t].sum())
            assert (s["tp"][k, t], s["fp"][k, t], s["fn"][k, t]) == (tp, fp, fn)
            want = {"iou": (tp, tp + fp + fn), "precision": (tp, tp + fp), "recall": (tp, tp + fn),
                    "f1": (2 * tp, 2 * tp + fp + fn)}
            for name, (num, den) in want.items():
                assert s[name][k, t] == (num / den if den else 0.0), (name, k, t)
    assert s["tp"].dtype == np.int64 and s["iou"].dtype == np.float64
    assert not s["iou"][3].any()


def test_sweep_refuses_other_shapes_and_floats():
    with pytest.raises(ValueError):
        cal.sweep(np.zeros((3, 256), dtype=np.int64))
    with pytest.raises(ValueError):
        cal.sweep(np.zeros((3, 2, 256), dtype=np.float64))


# ---- best_thresholds -----------------------------------------------------------------------------------------------------

def test_best_thresholds_finds_a_planted_optimum():
    h = np.zeros((4, 2, 256), dtype=np.int64)
    h[0, 1, 180:] = 7   # class 0: the class's pixels at q >= 180, the others below: a perfect split at 180
    h[0, 0, :180] = 5
    h[1, 1, 200] = 10   # class 1: IoU is 1 for every t in 1..200 (no other pixel scores above 0): the smallest wins
    h[1, 0, 0] = 50
    h[2, 0, 10:90] = 3  # class 2: no target pixel at all
    h[3, 1, 255] = 4    # class 3: only the top bin; and negatives right below it
    h[3, 0, 254] = 9
    for objective in ("iou", "f1"):
        thr = cal.best_thresholds(h, objective)
        assert thr.dtype == np.uint8 and thr.tolist() == [180, 1, 0, 255], objective
    assert cal.best_thresholds(h, min_support=41).tolist() == [180, 0, 0, 0]  # supports: 532, 10, 0, 4
    assert cal.best_thresholds(h, min_support=0).tolist() == [180, 1, 0, 255]  # zero support stays unconstrained
    with pytest.raises(ValueError):
        cal.best_thresholds(h, "accuracy")


def test_best_thresholds_is_the_first_maximum_of_the_sweep():
    h = _random_hist(7, K=6)
    s = cal.sweep(h)
    for objective in ("iou", "f1"):
        thr = cal.best_thresholds(h, objective)
        for k in range(6):
            curve = s[objective][k, 1:]
            assert thr[k] >= 1 and curve[thr[k] - 1] == curve.max()
            assert not (curve[:thr[k] - 1] == curve.max()).any()


# ---- ECE -----------------------------------------------------------------------------------------------------------------

def test_ece_of_a_perfectly_calibrated_histogram_is_exactly_zero():
    h = np.zeros((3, 2, 256), dtype=np.int64)
    for k, bins in enumerate(([0, 51, 255], [85, 170, 102], [17])):
        for q in bins:  # n = 255 m pixels of which q m are the class's: pos * 255 == q * n
            m = 1 + q % 3
            h[k, 1, q], h[k, 0, q] = q * m, (255 - q) * m
    for k in range(3):
        q = np.nonzero(h[k].sum(0))[0]
        assert (h[k, 1, q] * 255 == q * h[k].sum(0)[q]).all()
    assert cal.expected_calibration_error(h).tolist() == [0.0, 0.0, 0.0]


def test_ece_of_a_known_gap():
    h = np.zeros((2, 2, 256), dtype=np.int64)
    h[0, 0, 255] = 10  # scored 1.0, never right: gap 1
    h[0, 1, 0] = 30    # scored 0.0, always right: gap 1
    assert cal.expected_calibration_error(h).tolist() == [1.0, 0.0]  # class 1 has no pixel: 0


# ---- the file -------------------------------------------------------------------------------------------------------------

def test_the_file_round_trips_bytes_through_floats(tmp_path):
    path = str(tmp_path / cal.FILE_NAME)
    thr = np.arange(256, dtype=np.uint8)
    names = [f"c{i}" for i in range(256)]
    cal.write_thresholds(path, thr, names, {"objective": "iou", "fallback": 18, "iou_argmax": np.linspace(0, 1, 256)},
                         task="T")
    doc = yaml.safe_load(open(path))
    assert list(doc) == ["T"]
    entry = doc["T"]
    assert entry["thresholds_u8"] == thr.tolist() and entry["thresholds"] == [t / 255.0 for t in range(256)]
    assert entry["class_names"] == names and entry["objective"] == "iou" and entry["fallback"] == 18
    assert entry["iou_argmax"] == np.linspace(0, 1, 256).tolist()
    read = cal.read_thresholds(path, 256, task="T")
    assert read["thresholds_u8"].dtype == np.uint8 and np.array_equal(read["thresholds_u8"], thr)
    assert read["fallback"] == 18
    # the floats alone give the same bytes: every t / 255 reads back as t
    del entry["thresholds_u8"]
    floats = str(tmp_path / "floats.yaml")
    yaml.safe_dump({"T": entry}, open(floats, "w"))
    assert np.array_equal(cal.read_thresholds(floats, 256)["thresholds_u8"], thr)
    # a second task is added to the file, the first stays
    cal.write_thresholds(path, [3, 4], task="U")
    assert cal.read_thresholds(path, 2, task="U")["thresholds_u8"].tolist() == [3, 4]
    assert np.array_equal(cal.read_thresholds(path, 256, task="T")["thresholds_u8"], thr)
    with pytest.raises(ValueError, match="no thresholds for task 'V'"):
        cal.read_thresholds(path, 2, task="V")


def test_float_thresholds_read_as_the_smallest_passing_byte(tmp_path):
    path = str(tmp_path / "t.yaml")
    yaml.safe_dump({"thresholds": [0.0, 0.5, 0.7, 1.0, 0.0039, 128 / 255]}, open(path, "w"))  # a bare mapping
    # q / 255 >= 0.5 from q = 128 on; >= 0.7 from 179 (178.5 up); 0.0039 * 255 = 0.9945 -> 1
    assert cal.read_thresholds(path, 6)["thresholds_u8"].tolist() == [0, 128, 179, 255, 1, 128]
    assert cal.read_thresholds(path, 6)["fallback"] is None
    yaml.safe_dump({"thresholds": [0.2, 1.5]}, open(path, "w"))
    with pytest.raises(ValueError):
        cal.read_thresholds(path, 2)


def test_thresholds_u8_alone_are_accepted_and_a_wrong_length_names_both_numbers(tmp_path):
    path = str(tmp_path / "t.yaml")
    yaml.safe_dump({"any": {"thresholds_u8": [0, 17, 255]}}, open(path, "w"))
    assert cal.read_thresholds(path, 3, task="other")["thresholds_u8"].tolist() == [0, 17, 255]  # one mapping serves all
    with pytest.raises(ValueError, match=r"3 thresholds for 19 classes"):
        cal.read_thresholds(path, 19)
    yaml.safe_dump({"any": {"thresholds_u8": [0, 256]}}, open(path, "w"))
    with pytest.raises(ValueError):
        cal.read_thresholds(path, 2)
    with pytest.raises(ValueError):
        cal.write_thresholds(path, [0, 300])
    yaml.safe_dump([1, 2], open(path, "w"))
    with pytest.raises(ValueError, match="not a threshold file"):
        cal.read_thresholds(path, 2)


def test_iou_from_confmat_counts_pixels_without_a_column_as_misses():
    cm = np.array([[5, 1], [2, 4]])
    assert cal.iou_from_confmat(cm).tolist() == [5 / 8, 4 / 7]
    # three more pixels of class 0 got a fallback label outside the matrix
    assert cal.iou_from_confmat(cm, support=[9, 6]).tolist() == [5 / 11, 4 / 7]
    assert cal.iou_from_confmat(np.zeros((2, 2), dtype=np.int64)).tolist() == [0.0, 0.0]


# ---- the zonal configuration ---------------------------------------------------------------------------------------------

def test_a_missing_threshold_file_warns_and_is_not_in_effect(tmp_path, caplog):
    from flair_zonal_detection.config import threshold_file
    assert threshold_file({}) is None and threshold_file({"model_threshold_filepath": None}) is None
    assert not caplog.records  # no key: nothing to say
    with caplog.at_level(logging.WARNING):
        assert threshold_file({"model_threshold_filepath": str(tmp_path / "nowhere.yaml")}) is None
    assert len(caplog.records) == 1 and "does not exist" in caplog.text
    caplog.clear()
    path = str(tmp_path / cal.FILE_NAME)
    cal.write_thresholds(path, [0] * 19)
    assert threshold_file({"model_threshold_filepath": path}) == path
    assert threshold_file({"model_threshold_filepath": path, "output_type": "argmax"}) == path
    assert not caplog.records
    with caplog.at_level(logging.WARNING):
        assert threshold_file({"model_threshold_filepath": path, "output_type": "class_prob"}) is None
    assert len(caplog.records) == 1 and "label output" in caplog.text


def test_the_tile_loop_takes_the_thresholded_entries_only_with_a_file_in_effect():
    """inference_and_write switches on threshold_file(config) alone: with None, the calls are the plain ones"""
    import inspect
    from flair_zonal_detection import inference
    src = inspect.getsource(inference.inference_and_write)
    assert "thr_path = threshold_file(config)" in src
    assert src.count("if thr_path is not None:") == 2  # the plain path and the TTA path
    assert src.count("ops.predict_u8(") == 1 and src.count("ops.tta_predict_u8(") == 1


@pytest.mark.parametrize("bad", [-1, 256, 18.0, "18", True, None])
def test_a_bad_threshold_fallback_raises(bad):
    from flair_zonal_detection.config import validate_config, validate_threshold_fallback
    with pytest.raises(ValueError, match="threshold_fallback"):
        validate_threshold_fallback({"threshold_fallback": bad})
    cfg = {k: "x" for k in ("output_path", "output_name", "model_weights", "img_pixels_detection", "margin",
                            "modalities", "tasks", "output_px_meters")}
    with pytest.raises(ValueError, match="threshold_fallback"):
        validate_config(dict(cfg, threshold_fallback=bad))


def test_threshold_fallback_defaults_to_the_polygon_background():
    import inspect
    from flair_zonal_detection.config import validate_threshold_fallback
    from flair_zonal_detection.inference import raster_to_polygons
    assert validate_threshold_fallback({}) == 18 == inspect.signature(raster_to_polygons).parameters[
        "background_value"].default
    assert validate_threshold_fallback({"threshold_fallback": 0}) == 0
    assert validate_threshold_fallback({"threshold_fallback": 255}) == 255


def test_the_cli_takes_the_two_flags():
    from flair_zonal_detection.main import build_parser
    args = build_parser().parse_args(["--config", "c.yaml", "--thresholds", "t.yaml", "--threshold-fallback", "7"])
    assert (args.thresholds, args.threshold_fallback) == ("t.yaml", 7)
    args = build_parser().parse_args(["--config", "c.yaml"])
    assert (args.thresholds, args.threshold_fallback) == (None, None)
