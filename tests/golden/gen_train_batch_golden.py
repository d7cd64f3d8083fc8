#!/usr/bin/env python
"""tests/golden/train_batch.npz / .json: inputs and outputs of the reference's own data side -- flair_dataset's
__getitem__ (/root/reference/flair_hub/data/dataloader.py:105-257) with its norm, calc_elevation and
reshape_label_ohe, and pad_collate_flair over the four samples -- for 4 patches of aerial 5 x 64 x 64 uint8, DEM
2 x 16 x 16 float32 and labels 64 x 64 uint8 (values above K - 1 and a 255 among them), under 'custom' normalisation,
in four settings: the DEM as stored, calc_elevation, calc_elevation_stack_dsm, and aerial + a Sentinel-2 series of
ragged length with its dates.  rasterio and skimage are absent: rasterio.open is stubbed to serve the arrays below by
file name, skimage.img_as_float is never reached.  Only the arrays and the settings are stored."""
import datetime
import json
import os
import sys
import types

import numpy as np
import torch

PATCHES = {}


class _Src:
    def __init__(self, arr):
        self.arr = arr

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def read(self, channels=None):
        return self.arr.copy() if channels is None else self.arr[[c - 1 for c in channels]].copy()


rasterio = types.ModuleType("rasterio")
rasterio.open = lambda path: _Src(PATCHES[os.path.basename(path)])
sys.modules["rasterio"] = rasterio
skimage = types.ModuleType("skimage")
skimage.img_as_float = None
sys.modules["skimage"] = skimage

sys.path.insert(0, "/root/reference")
from flair_hub.data.dataloader import flair_dataset  # noqa: E402
from flair_hub.data.utils_data.padding import pad_collate_flair  # noqa: E402

TASK, K = "AERIAL_LABEL-COSIA", 19
AREAS = ["D004-2021_UU-S2-32_3-5", "D004-2021_UU-S2-32_3-6", "D012-2019_FF-S1-7_10-2", "D012-2019_FF-S1-7_0-11"]
T_LEN = [3, 5, 2, 4]
r = np.random.RandomState(11)
names = {"AERIAL_RGBI": [], "DEM_ELEV": [], "SENTINEL2_TS": [], "SENTINEL2_MSK-SC": [], TASK: []}
dates = {}
for area, t in zip(AREAS, T_LEN):
    dom, rest = area.split("_", 1)
    for mod, arr in (
            ("AERIAL_RGBI", r.randint(0, 256, (5, 64, 64)).astype(np.uint8)),
            ("DEM_ELEV", np.stack([(z := (r.randn(16, 16) * 40 + 350)) + np.abs(r.randn(16, 16)) * 12, z]).astype(np.float32)),
            ("SENTINEL2_TS", r.randint(0, 9000, (t * 10, 10, 10)).astype(np.uint16)),
            ("SENTINEL2_MSK-SC", r.randint(0, 100, (t * 2, 10, 10)).astype(np.uint8)),
            (TASK, r.randint(0, 24, (1, 64, 64)).astype(np.uint8))):
        name = f"{dom}_{mod}_{rest}.tif" if mod == TASK else f"{area}_{mod}.tif"
        PATCHES[name] = arr
        names[mod].append(name)
    PATCHES[names[TASK][-1]][0, 0, :3] = [K - 1, K, 255]
    days = [datetime.datetime(int(dom[-4:]), 1, 1) + datetime.timedelta(days=int(d))
            for d in sorted(r.choice(360, t, replace=False))]
    dates[area] = {"dates": np.array(days),
                   "diff_dates": np.array([(d - datetime.datetime(d.year, 5, 15)).days for d in days])}

NORM = {"norm_type": "custom",
        "AERIAL_RGBI_means": [105.08, 110.87, 101.82, 106.38, 53.26], "AERIAL_RGBI_stds": [52.17, 45.38, 44.0, 39.69, 79.3]}
DEM_NORM = {0: ([360.0, 350.0], [45.0, 40.0]), 1: ([9.5], [7.25]), 2: ([360.0, 9.5], [45.0, 7.25])}
ALL = ["AERIAL_RGBI", "AERIAL-RLT_PAN", "DEM_ELEV", "SPOT_RGBI", "SENTINEL2_TS", "SENTINEL1-ASC_TS", "SENTINEL1-DESC_TS"]


def config(setting):
    on = {"AERIAL_RGBI"} | ({"SENTINEL2_TS"} if setting == "s2" else {"DEM_ELEV"})
    mode = {"dem_raw": 0, "dem_elev": 1, "dem_stack": 2, "s2": 0}[setting]
    norm = dict(NORM)
    norm["DEM_ELEV_means"], norm["DEM_ELEV_stds"] = DEM_NORM[mode]
    return {
        "labels": [TASK],
        "labels_configs": {TASK: {"value_name": {i: f"c{i}" for i in range(K)}, "label_channel_nomenclature": 1}},
        "modalities": {
            "inputs": {m: m in on for m in ALL},
            "inputs_channels": {"AERIAL_RGBI": [1, 2, 3, 4, 5], "SENTINEL2_TS": [2, 3, 8]},
            "normalization": norm,
            "pre_processings": {"calc_elevation": mode > 0, "calc_elevation_stack_dsm": mode == 2,
                                "filter_sentinel2": False, "temporal_average_sentinel2": False,
                                "temporal_average_sentinel1": False, "use_augmentation": False},
        },
        "models": {"multitemp_model": {"ref_date": "05-15"}},
    }


save = {"in/" + k: v for k, v in PATCHES.items()}
meta = {"task": TASK, "areas": AREAS, "files": names, "settings": {},
        "dates": {a: [d.strftime("%Y%m%d") for d in v["dates"]] for a, v in dates.items()}}
for setting in ("dem_raw", "dem_elev", "dem_stack", "s2"):
    cfg = config(setting)
    paths = {k: ["/data/" + n for n in v] for k, v in names.items()}
    paths["DATES_S2"] = dates
    ds = flair_dataset(cfg, paths, use_augmentations=None)
    samples = [ds[i] for i in range(len(ds))]
    meta["settings"][setting] = {"config": cfg, "keys": list(samples[0].keys()),
                                 "ids": [s[f"ID_{TASK}"] for s in samples]}
    for i, s in enumerate(samples):
        for k, v in s.items():
            if torch.is_tensor(v):
                assert v.dtype == torch.float32
                if k == "AERIAL_RGBI" and setting != "dem_raw":  # the same arrays in every setting: stored once
                    assert np.array_equal(v.numpy(), save[f"dem_raw/{i}/{k}"])
                    continue
                save[f"{setting}/{i}/{k}"] = v.numpy()
    out = pad_collate_flair(samples)
    meta["settings"][setting]["collate_keys"] = list(out.keys())
    for k, v in out.items():
        if torch.is_tensor(v):
            if k == "AERIAL_RGBI":  # a plain stack of the samples above (the file stays under the size limit)
                assert torch.equal(v, torch.stack([s[k] for s in samples]))
                continue
            save[f"{setting}/collate/{k}"] = v.numpy()
    # the label rule the device kernel implements: argmax over the one-hot planes (tasks_module.py:153)
    save[f"{setting}/collate/argmax_{TASK}"] = out[TASK].argmax(1).numpy().astype(np.uint8)

here = os.path.dirname(os.path.abspath(__file__))
# labels are stored as indices next to the one-hot planes' argmax; the one-hot planes themselves are K x larger
for k in [k for k in save if k.endswith("/" + TASK) and not k.startswith("in/")]:
    save[k] = np.packbits(save[k].astype(bool), axis=None)
np.savez_compressed(os.path.join(here, "train_batch.npz"), **save)
with open(os.path.join(here, "train_batch.json"), "w") as f:
    json.dump(meta, f, indent=1, sort_keys=True, default=lambda o: {str(k): v for k, v in o.items()})
print(os.path.getsize(os.path.join(here, "train_batch.npz")), "bytes;", {s: m["keys"] for s, m in meta["settings"].items()})
