"""flair_hub.writer.metrics_utils.compute_and_save_metrics against what the reference's own function wrote for the same
confusion matrices and configurations (tests/golden/metrics_writer.json, made by gen_metrics_writer_golden.py): the
keys of metrics.json in the same order, every number to 1e-12 relative (NaN where the reference has NaN), the stored
matrix exactly.  Cases: six classes with an absent class, a zero-weight class and per-modality exceptions; nineteen
classes with 15-18 at weight 0; a matrix of zeros.  numpy only, no GPU."""
import json
import math
import os
import warnings

import numpy as np
import pytest

from helpers import ROOT

TASK = "AERIAL_LABEL-COSIA"
with open(os.path.join(ROOT, "tests", "golden", "metrics_writer.json")) as f:
    CASES = json.load(f)


def config_of(case):
    vw = {}
    for k, v in case["value_weights"].items():
        if k == "default_exceptions" and v is not None:
            v = {int(a): b for a, b in v}
        elif k == "per_modality_exceptions" and v is not None:
            v = {mod: {int(a): b for a, b in ex} for mod, ex in v}
        vw[k] = v
    return {"labels_configs": {TASK: {"value_name": dict(enumerate(case["value_name"])), "value_weights": vw}},
            "modalities": {"inputs": dict(map(tuple, case["inputs"]))}, "paths": {"out_model_name": "golden"}}


def assert_same(got, want, where):
    """`want` is the golden's form: dictionaries as [key, value] pairs in order, NaN as "nan" """
    if isinstance(got, dict):
        assert [k for k in got] == [k for k, _ in want], where
        for (k, g), (_, w) in zip(got.items(), want):
            assert_same(g, w, f"{where}.{k}")
    elif isinstance(got, list):
        assert isinstance(want, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{where}[{i}]")
    elif want == "nan":
        assert isinstance(got, float) and math.isnan(got), (where, got)
    elif isinstance(want, str):
        assert got == want, where
    else:
        assert type(got) is type(want), (where, got, want)  # an integer weight stays an integer
        assert abs(got - want) <= 1e-12 * abs(want), (where, got, want)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_metrics_json_and_matrix_equal_the_reference(case, tmp_path):
    from flair_hub.writer.metrics_utils import compute_and_save_metrics
    cm = np.array(case["confmat"], dtype=int)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no warning escapes
        compute_and_save_metrics(cm, config_of(case), str(tmp_path), TASK, mode="predict")
    folder = tmp_path / "metrics_golden" / TASK
    assert sorted(p.name for p in folder.iterdir()) == ["confmat_predict.npy", "metrics.json"]
    saved = np.load(folder / "confmat_predict.npy")
    assert saved.dtype == cm.dtype and np.array_equal(saved, cm)  # the full matrix, zero-weight classes included
    with open(folder / "metrics.json") as f:
        got = json.load(f)
    assert_same(got, case["metrics"], case["name"])


def test_the_cases_cover_what_they_claim():
    by = {c["name"]: c for c in CASES}
    six = dict(by["six_classes"]["metrics"])
    assert six["classes"] == ["building", "water", "soil", "grass", "snow"]          # "other" (weight 0) is gone
    assert six["per_class_iou"][4] == 0 and six["per_class_fscore"][4] == 0          # the absent class: NaN -> 0
    assert [m for m, _ in six["per_class_modality_weights"]] == ["AERIAL_RGBI", "SENTINEL2_TS"]  # active inputs only
    assert dict(six["per_class_modality_weights"])["AERIAL_RGBI"] == [1, 2.5, 0.5, 1, 1]
    assert len(dict(by["nineteen_classes"]["metrics"])["classes"]) == 15
    assert dict(by["all_zero"]["metrics"])["Avg_metrics"][1] == "nan"


def test_mode_names_the_matrix_file(tmp_path):
    from flair_hub.writer.metrics_utils import compute_and_save_metrics
    case = CASES[0]
    compute_and_save_metrics(np.array(case["confmat"]), config_of(case), str(tmp_path), TASK, mode="metrics_only")
    assert (tmp_path / "metrics_golden" / TASK / "confmat_metrics_only.npy").exists()
