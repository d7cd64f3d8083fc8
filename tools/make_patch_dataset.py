#!/usr/bin/env python
"""A synthetic dataset in the FLAIR-HUB layout: GeoTIFF patches (aerial 5-band uint8, 2-band float32 DEM, uint8 labels)
and the train / val / test CSVs that name them, plus a directory of YAML files for ``python -m flair_hub.main``.  The
data are random and never all zero (a constant patch would make every normalisation and loss trivially equal).

  python tools/make_patch_dataset.py DIR [--patches 64] [--size 512] [--dem-size 512] [--val 16] [--seed 0]
                                         [--cache none|device] [--batch 8] [--epochs 1] [--precision bf16]

DIR/patches/*.tif, DIR/{train,val,test}.csv, DIR/config/*.yaml."""
from __future__ import annotations

import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

MOD, DEM, TASK = "AERIAL_RGBI", "DEM_ELEV", "AERIAL_LABEL-COSIA"
NORMALIZATION = {"norm_type": "custom", f"{MOD}_means": [105.08, 110.87, 101.82, 106.38, 53.26],
                 f"{MOD}_stds": [52.17, 45.38, 44.0, 39.69, 79.3], f"{DEM}_means": [9.5], f"{DEM}_stds": [7.25]}


def write_tif(path: str, arr: np.ndarray) -> None:
    from flair_zonal_detection.geotiff import GeoTiffWriter
    w = GeoTiffWriter(path, arr.shape[2], arr.shape[1], arr.shape[0], 800000.0, 6500000.0, 0.2, crs="EPSG:2154",
                      dtype=arr.dtype)
    w.data[:] = arr
    w.close()


def write_dataset(root: str, patches: int = 64, size: int = 512, dem_size: int = 512, val: int = 16, seed: int = 0,
                  dem: bool = True) -> dict:
    """-> {'train' / 'val' / 'test': csv path}; the last ``val`` patches are the validation and test splits"""
    os.makedirs(os.path.join(root, "patches"), exist_ok=True)
    r = np.random.RandomState(seed)
    rows = []
    for i in range(patches):
        area = f"D{i // 100:03d}-2021_UU-S2-{i % 100}_{i}-{i + 1}"
        dom, rest = area.split("_", 1)
        files = {MOD: f"{area}_{MOD}.tif", TASK: f"{dom}_{TASK}_{rest}.tif"}
        write_tif(os.path.join(root, "patches", files[MOD]), r.randint(1, 256, (5, size, size)).astype(np.uint8))
        if dem:
            files[DEM] = f"{area}_{DEM}.tif"
            z = r.randn(dem_size, dem_size) * 40 + 350
            write_tif(os.path.join(root, "patches", files[DEM]),
                      np.stack([z + np.abs(r.randn(dem_size, dem_size)) * 12, z]).astype(np.float32))
        write_tif(os.path.join(root, "patches", files[TASK]), r.randint(0, 19, (1, size, size)).astype(np.uint8))
        rows.append({k: os.path.join(root, "patches", v) for k, v in files.items()})
    out = {}
    for split, part in (("train", rows[:patches - val]), ("val", rows[patches - val:]), ("test", rows[patches - val:])):
        out[split] = os.path.join(root, f"{split}.csv")
        with open(out[split], "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(part)
    return out


def make_config(root: str, csvs: dict, cache: str = "none", batch: int = 8, epochs: int = 1, precision: str = "bf16",
                dem: bool = True, hip_graph: bool = True) -> dict:
    from flairhip.configs import unet_resnet34_config
    cfg = unet_resnet34_config(in_channels=5, precision=precision, batch_size=batch)
    mods = cfg["modalities"]
    mods["inputs"][DEM] = bool(dem)
    mods["pre_processings"].update(calc_elevation=bool(dem), use_augmentation=True)
    mods["normalization"] = {k: v for k, v in NORMALIZATION.items() if dem or not k.startswith(DEM)}
    cfg["hyperparams"].update(num_epochs=epochs, scheduler=None)
    cfg["hardware"].update(hip_graph=hip_graph, sample_cache=cache)
    cfg["paths"] = {"train_csv": csvs["train"], "val_csv": csvs["val"], "test_csv": csvs["test"],
                    "out_folder": os.path.join(root, "out"), "out_model_name": "synthetic", "global_mtd_folder": root + os.sep}
    cfg["tasks"] = {"train": True, "predict": True, "write_files": True, "georeferencing_output": False}
    return cfg


def main() -> None:
    import yaml
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dem-size", type=int, default=512)
    ap.add_argument("--val", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cache", choices=("none", "device"), default="none")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--precision", default="bf16")
    args = ap.parse_args()
    root = os.path.abspath(args.dir)
    csvs = write_dataset(root, args.patches, args.size, args.dem_size, args.val, args.seed)
    cfg = make_config(root, csvs, args.cache, args.batch, args.epochs, args.precision)
    os.makedirs(os.path.join(root, "config"), exist_ok=True)
    for key, value in cfg.items():  # one file per top-level key: read_config merges them
        with open(os.path.join(root, "config", f"{key}.yaml"), "w") as f:
            yaml.safe_dump({key: value}, f)
    print(f"{args.patches} patches under {root}/patches; python -m flair_hub.main --config {root}/config")


if __name__ == "__main__":
    main()
