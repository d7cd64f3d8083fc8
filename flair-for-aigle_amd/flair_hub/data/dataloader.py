"""flair_dataset -- counterpart of the reference's flair_hub/data/dataloader.py (flair_dataset :19-257).

Two sample schemas:

``device_prepare=False``: the reference's ``__getitem__``, key for key -- normalised inputs and one-hot labels as
float32 tensors, ``ID_<task>`` paths, the Sentinel series filtered / averaged on the host with their date offsets, the
host augmentation applied to the arrays.

``device_prepare=True``: what was decoded and nothing more -- the raw bands of every mono-temporal modality in the
file's sample type (uint8 aerial, the 2-band float32 DEM), the raw label channel as uint8 [H, W] and ``ID_<task>``.
Normalisation, the elevation difference, the label rule and the augmentation then happen in the kernels of
csrc/sample_gather.hip on the device; the ``<MOD>_NORM`` vectors those kernels need are supplied once by the data
module (``norm_vectors``), not per sample.  Time series keep the host schema (filtered / averaged on the host, float32)
on the streamed path; while the data module fills a store that takes them (``keep_series_raw``) they are handed out as
the numpy arrays they are before that cast, so that the store can keep the decoded sample type."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
from torch.utils.data import Dataset

from flair_hub.data.utils_data.augmentations import apply_numpy_augmentations
from flair_hub.data.utils_data.elevation import calc_elevation
from flair_hub.data.utils_data.io import read_patch
from flair_hub.data.utils_data.label import reshape_label_ohe
from flair_hub.data.utils_data.norm import norm
from flair_hub.data.utils_data.sentinel import filter_time_series, reshape_sentinel, temporal_average

MONO_KEYS = ("AERIAL_RGBI", "AERIAL-RLT_PAN", "DEM_ELEV", "SPOT_RGBI")
SENTINEL1_KEYS = ("SENTINEL1-ASC_TS", "SENTINEL1-DESC_TS")
DATES_OF = {"SENTINEL2_TS": "DATES_S2", "SENTINEL1-ASC_TS": "DATES_S1_ASC", "SENTINEL1-DESC_TS": "DATES_S1_DESC"}


def elevation_mode(config: Dict) -> int:
    """flairhip.ops.ELEV_*: what the pre_processings keys ask of a DEM_ELEV patch"""
    pp = config["modalities"].get("pre_processings", {})
    if not pp.get("calc_elevation", False):
        return 0
    return 2 if pp.get("calc_elevation_stack_dsm", False) else 1


class flair_dataset(Dataset):
    def __init__(self, config: Dict, dict_paths: Dict, use_augmentations=None, device_prepare: bool = False) -> None:
        self.config = config
        self.device_prepare = bool(device_prepare)
        self.keep_dem_bands = False  # set by the data module while it fills a device-resident store
        self.keep_series_raw = False  # likewise: '<SENSOR>_TS' / '<SENSOR>_DATES' stay numpy arrays, uncast
        self.use_augmentations = apply_numpy_augmentations if use_augmentations is True else use_augmentations
        mods = config["modalities"]
        enabled = mods["inputs"]
        self.list_patch = {}
        for mod, on in enabled.items():
            if on and mod in dict_paths:
                self.list_patch[mod] = np.array(dict_paths[mod])
                if mod == "SENTINEL2_TS":
                    self.list_patch["SENTINEL2_MSK-SC"] = np.array(dict_paths["SENTINEL2_MSK-SC"])
        self.dict_dates = {mod: dict_paths.get(key, {}) for mod, key in DATES_OF.items() if mod in enabled}
        self.tasks = {}
        for task in config["labels"]:
            lc = config["labels_configs"][task]
            self.tasks[task] = {"data_paths": np.array(dict_paths[task]), "num_classes": len(lc["value_name"]),
                                "channels": [lc.get("label_channel_nomenclature", 1)]}
        normalization = mods.get("normalization", {})
        self.norm_type = normalization.get("norm_type")
        self.channels = {m: mods.get("inputs_channels", {}).get(m, []) for m, on in enabled.items() if on}
        self.normalization = {m: {"mean": normalization.get(f"{m}_means", []), "std": normalization.get(f"{m}_stds", [])}
                              for m, on in enabled.items() if on}
        self.ref_date = config["models"]["multitemp_model"]["ref_date"]

    def __len__(self) -> int:
        for info in self.tasks.values():
            if len(info["data_paths"]) > 0:
                return len(info["data_paths"])
        return 0

    # ---- what the device needs to know once -----------------------------------------------------------------------

    def norm_vectors(self) -> Dict[str, Optional[torch.Tensor]]:
        """{modality: f32 [2, C_out] (mean, std) or None} for the mono-temporal modalities of a device_prepare dataset.
        'custom' gives the configured vectors (one entry per OUTPUT channel: after the elevation pre-processing for
        DEM_ELEV), 'scaling' of uint8 samples mean 0 / std 255, 'without' none."""
        out = {}
        for mod in MONO_KEYS:
            if mod not in self.list_patch:
                continue
            if self.norm_type == "custom":
                mean, std = self.normalization[mod]["mean"], self.normalization[mod]["std"]
                if len(mean) != len(std) or not len(mean):
                    raise SystemExit(f"norm_type 'custom' needs {mod}_means and {mod}_stds of the same length")
                out[mod] = torch.tensor([list(mean), list(std)], dtype=torch.float32)
            elif self.norm_type == "without":
                out[mod] = None
            elif self.norm_type == "scaling":
                out[mod] = "scaling"  # resolved against the sample type by the data module
            else:
                raise SystemExit("Normalization argument should be 'scaling', 'custom', or 'without'.")
        return out

    # ---- samples --------------------------------------------------------------------------------------------------------

    def _area_key(self, index: int) -> Optional[str]:
        key = None
        for info in self.tasks.values():
            parts = info["data_paths"][index].split("/")[-1].split("_")
            key = "_".join([parts[0], parts[-2], parts[-1].split(".")[0]])
        return key

    def _sentinel(self, batch: Dict, key: str, index: int, area: str) -> None:
        pp = self.config["modalities"]["pre_processings"]
        s2 = key == "SENTINEL2_TS"
        data = reshape_sentinel(read_patch(self.list_patch[key][index]), chunk_size=10 if s2 else 2)
        data = data[:, [c - 1 for c in self.channels[key]], :, :]
        entry = self.dict_dates[key][area]
        dates, diffs = entry["dates"], entry["diff_dates"]
        if s2 and pp.get("filter_sentinel2"):
            msk = reshape_sentinel(read_patch(self.list_patch["SENTINEL2_MSK-SC"][index]), chunk_size=2)
            keep = np.where(filter_time_series(msk, max_cloud_value=pp["filter_sentinel2_max_cloud"],
                                               max_snow_value=pp["filter_sentinel2_max_snow"],
                                               max_fraction_covered=pp["filter_sentinel2_max_frac_cover"]))[0]
            data, dates, diffs = data[keep], dates[keep], diffs[keep]
        period = pp.get("temporal_average_sentinel2" if s2 else "temporal_average_sentinel1")
        if period:
            data, diffs = temporal_average(data, dates, period=period, ref_date=self.ref_date)
        batch[key] = data
        batch[key.replace("_TS", "_DATES")] = diffs

    def __getitem__(self, index: int) -> Dict:
        batch = {}
        for task, info in self.tasks.items():
            batch[f"ID_{task}"] = info["data_paths"][index]
        area = self._area_key(index)
        raw = self.device_prepare
        mode = elevation_mode(self.config)

        for key in MONO_KEYS:
            if key not in self.list_patch or self.list_patch[key][index] is None:
                continue
            if key == "DEM_ELEV":
                data = read_patch(self.list_patch[key][index])
                # raw samples keep both bands where a kernel takes the difference: always for the store, and on the
                # streamed path for calc_elevation alone (a 2-band batch into the 1-channel encoder says so by itself)
                if mode and not (raw and (mode == 1 or self.keep_dem_bands)):
                    elev = calc_elevation(data)
                    data = np.stack((data[0], elev[0]), axis=0) if mode == 2 else elev
            else:
                data = read_patch(self.list_patch[key][index], self.channels[key])
            if raw:
                batch[key] = np.ascontiguousarray(data)
            else:
                n = self.normalization[key]
                batch[key] = norm(data, self.norm_type, n["mean"], n["std"])

        if "SENTINEL2_TS" in self.list_patch:
            self._sentinel(batch, "SENTINEL2_TS", index, area)
        for key in SENTINEL1_KEYS:
            if key in self.list_patch and self.list_patch[key][index] is not None:
                self._sentinel(batch, key, index, area)

        for task, info in self.tasks.items():
            label = read_patch(info["data_paths"][index], info["channels"])
            if raw:
                if label.dtype != np.uint8:
                    if label.min() < 0 or label.max() > 255:
                        raise ValueError(f"{info['data_paths'][index]}: label values outside 0..255")
                    label = label.astype(np.uint8)
                batch[task] = np.ascontiguousarray(label[0])
            else:
                batch[task] = reshape_label_ohe(label, info["num_classes"])

        if raw:
            # no host augmentation: the codes ride along as batch['AUG'] (the trainer draws them), the kernels apply them
            out = {}
            for k, v in batch.items():
                if k in MONO_KEYS or k in self.tasks:
                    out[k] = torch.from_numpy(v)  # the sample type as decoded
                elif self.keep_series_raw and k.endswith(("_TS", "_DATES")):
                    out[k] = np.asarray(v)
                elif isinstance(v, (np.ndarray, list)) and "ID_" not in k:
                    out[k] = torch.tensor(v, dtype=torch.float32)
                else:
                    out[k] = v
            return out

        if callable(self.use_augmentations):
            input_keys = [k for k, v in self.config["modalities"]["inputs"].items() if v]
            batch = self.use_augmentations(batch, input_keys, list(self.config["labels"]))
        return {k: (torch.tensor(v, dtype=torch.float32) if isinstance(v, (np.ndarray, list)) and "ID_" not in k else v)
                for k, v in batch.items()}
