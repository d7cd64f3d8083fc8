#!/usr/bin/env python
"""tests/golden/metrics_writer.json: inputs and outputs of the reference's own compute_and_save_metrics
(flair_hub/writer/metrics_utils.py of a FLAIR-HUB checkout, numpy only) for three confusion matrices.

    python tests/golden/gen_metrics_writer_golden.py <FLAIR-HUB checkout>

Stored: the matrix, the part of the config the function reads (dictionaries with integer keys as [key, value] pairs) and
the metrics.json it wrote, as [key, value] pairs in file order (NaN as the string "nan").  Nothing of the reference's
text is stored."""
import json
import math
import os
import sys
import tempfile
import warnings

import numpy as np

sys.path.insert(0, sys.argv[1] if len(sys.argv) > 1 else os.environ["FLAIR_HUB_REFERENCE"])
from flair_hub.writer.metrics_utils import compute_and_save_metrics  # noqa: E402

TASK = "AERIAL_LABEL-COSIA"


def config_of(names, value_weights, inputs, model="golden"):
    return {"labels_configs": {TASK: {"value_name": dict(enumerate(names)), "value_weights": value_weights}},
            "modalities": {"inputs": inputs}, "paths": {"out_model_name": model}}


def pairs(d):
    return [[k, v] for k, v in d.items()]


def plain(v):
    if isinstance(v, float) and math.isnan(v):
        return "nan"
    if isinstance(v, list):
        return [plain(x) for x in v]
    if isinstance(v, dict):
        return pairs({k: plain(x) for k, x in v.items()})
    return v


rng = np.random.default_rng(7)
cases = []

# six classes: class 4 never occurs (neither target nor prediction), class 5 has weight 0, one per-modality exception
cm6 = rng.integers(0, 500, (6, 6))
cm6[4, :] = 0
cm6[:, 4] = 0
cases.append(("six_classes", cm6, ["building", "water", "soil", "grass", "snow", "other"],
              {"default": 1, "default_exceptions": {5: 0, 1: 2.5},
               "per_modality_exceptions": {"AERIAL_RGBI": {2: 0.5}, "DEM_ELEV": {0: 3}}},
              {"AERIAL_RGBI": True, "DEM_ELEV": False, "SENTINEL2_TS": True}))
# nineteen classes, 15-18 at weight 0 (the supervision of the reference's default configuration)
cm19 = rng.integers(0, 10000, (19, 19))
cm19[np.arange(19), np.arange(19)] += 50000
cases.append(("nineteen_classes", cm19, [f"class {i}" for i in range(19)],
              {"default": 1, "default_exceptions": {15: 0, 16: 0, 17: 0, 18: 0}, "per_modality_exceptions": None},
              {"AERIAL_RGBI": True}))
# nothing counted at all
cases.append(("all_zero", np.zeros((4, 4), dtype=int), ["a", "b", "c", "d"], {"default": 1}, {"AERIAL_RGBI": True}))

out = []
for name, cm, names, vw, inputs in cases:
    cfg = config_of(names, vw, inputs)
    with tempfile.TemporaryDirectory() as d, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        compute_and_save_metrics(cm, cfg, d, TASK, mode="predict")
        folder = os.path.join(d, "metrics_golden", TASK)
        assert sorted(os.listdir(folder)) == ["confmat_predict.npy", "metrics.json"]
        assert np.array_equal(np.load(os.path.join(folder, "confmat_predict.npy")), cm)
        with open(os.path.join(folder, "metrics.json")) as f:
            metrics = json.load(f)
    out.append({"name": name, "confmat": cm.tolist(), "value_name": names,
                "value_weights": {k: (pairs({a: (pairs(b) if isinstance(b, dict) else b) for a, b in v.items()})
                                      if isinstance(v, dict) else v) for k, v in vw.items()},
                "inputs": pairs(inputs), "metrics": plain(metrics)})
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "metrics_writer.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1, allow_nan=False)
print(path, os.path.getsize(path), "bytes")
