#!/usr/bin/env python
"""A synthetic dataset in the FLAIR-HUB layout: GeoTIFF patches (aerial 5-band uint8, 2-band float32 DEM, uint8 labels)
and the train / val / test CSVs that name them, plus a directory of YAML files for ``python -m flair_hub.main``.  The
data are random and never all zero (a constant patch would make every normalisation and loss trivially equal).

  python tools/make_patch_dataset.py DIR [--patches 64] [--size 512] [--dem-size 512] [--val 16] [--seed 0]
                                         [--cache none|device] [--batch 8] [--epochs 1] [--precision bf16]
                                         [--sentinel2 TMIN TMAX] [--s2-size 10] [--s2-average monthly|semi-monthly]
                                         [--cache-series]

``--sentinel2 TMIN TMAX`` adds a Sentinel-2 branch: per patch a uint16 series of a random length in TMIN..TMAX (10
bands per date, S2_SIZE pixels a side), its SENTINEL2_MSK-SC raster (snow and cloud probabilities, 2 bands per date)
and the acquisition dates in DIR/GLOBAL_SENTINEL2_MTD_DATES.gpkg; the config then enables SENTINEL2_TS (all ten
bands).  ``--s2-average`` sets temporal_average_sentinel2 (every batch then has 12 or 24 dates and a captured step
replays), ``--cache-series`` sets hardware.sample_cache_series.

DIR/patches/*.tif, DIR/{train,val,test}.csv, DIR/config/*.yaml."""
from __future__ import annotations

import argparse
import csv
import datetime
import json
import os
import sqlite3
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

MOD, DEM, TASK = "AERIAL_RGBI", "DEM_ELEV", "AERIAL_LABEL-COSIA"
S2, S2_MSK = "SENTINEL2_TS", "SENTINEL2_MSK-SC"
NORMALIZATION = {"norm_type": "custom", f"{MOD}_means": [105.08, 110.87, 101.82, 106.38, 53.26],
                 f"{MOD}_stds": [52.17, 45.38, 44.0, 39.69, 79.3], f"{DEM}_means": [9.5], f"{DEM}_stds": [7.25]}


def write_tif(path: str, arr: np.ndarray) -> None:
    from flair_zonal_detection.geotiff import GeoTiffWriter
    w = GeoTiffWriter(path, arr.shape[2], arr.shape[1], arr.shape[0], 800000.0, 6500000.0, 0.2, crs="EPSG:2154",
                      dtype=arr.dtype)
    w.data[:] = arr
    w.close()


def write_dates_gpkg(path: str, dates_by_patch: dict) -> None:
    """the GeoPackage the date reader needs and nothing more: gpkg_contents naming one feature table whose rows hold
    patch_id and acquisition_dates, a JSON object of 'YYYYMMDD' strings (the geometry column stays empty)"""
    if os.path.exists(path):
        os.remove(path)
    con = sqlite3.connect(path)
    con.execute("CREATE TABLE gpkg_contents (table_name TEXT PRIMARY KEY, data_type TEXT NOT NULL, identifier TEXT)")
    con.execute("CREATE TABLE sentinel_dates (fid INTEGER PRIMARY KEY, geom BLOB, patch_id TEXT, acquisition_dates TEXT)")
    con.execute("INSERT INTO gpkg_contents VALUES ('sentinel_dates', 'features', 'sentinel_dates')")
    for patch_id, days in dates_by_patch.items():
        con.execute("INSERT INTO sentinel_dates (geom, patch_id, acquisition_dates) VALUES (?, ?, ?)",
                    (b"", patch_id, json.dumps({str(i): d for i, d in enumerate(days)})))
    con.commit()
    con.close()


def write_dataset(root: str, patches: int = 64, size: int = 512, dem_size: int = 512, val: int = 16, seed: int = 0,
                  dem: bool = True, sentinel2=None, s2_size: int = 10) -> dict:
    """-> {'train' / 'val' / 'test': csv path}; the last ``val`` patches are the validation and test splits.
    ``sentinel2`` = (tmin, tmax): a Sentinel-2 series of a random length in that range per patch, its mask raster and
    the dates GeoPackage"""
    os.makedirs(os.path.join(root, "patches"), exist_ok=True)
    r = np.random.RandomState(seed)
    rows, dates = [], {}
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
        if sentinel2:
            t = int(r.randint(int(sentinel2[0]), int(sentinel2[1]) + 1))
            files[S2], files[S2_MSK] = f"{area}_{S2}.tif", f"{area}_{S2_MSK}.tif"
            write_tif(os.path.join(root, "patches", files[S2]),
                      r.randint(1, 10000, (t * 10, s2_size, s2_size)).astype(np.uint16))
            # mostly clear: probabilities 0..100, a few dates cloudy enough for filter_sentinel2 to drop
            msk = r.randint(0, 2, (t * 2, s2_size, s2_size)) * r.randint(0, 101, (t * 2, 1, 1)) * (r.rand(t * 2, 1, 1) < 0.2)
            write_tif(os.path.join(root, "patches", files[S2_MSK]), msk.astype(np.uint8))
            days = np.sort(r.choice(365, t, replace=False))
            dates[area] = [(datetime.date(2021, 1, 1) + datetime.timedelta(days=int(d))).strftime("%Y%m%d") for d in days]
        rows.append({k: os.path.join(root, "patches", v) for k, v in files.items()})
    out = {}
    for split, part in (("train", rows[:patches - val]), ("val", rows[patches - val:]), ("test", rows[patches - val:])):
        out[split] = os.path.join(root, f"{split}.csv")
        with open(out[split], "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0]))
            w.writeheader()
            w.writerows(part)
    if sentinel2:
        write_dates_gpkg(os.path.join(root, "GLOBAL_SENTINEL2_MTD_DATES.gpkg"), dates)
    return out


def make_config(root: str, csvs: dict, cache: str = "none", batch: int = 8, epochs: int = 1, precision: str = "bf16",
                dem: bool = True, hip_graph: bool = True, sentinel2: bool = False, s2_average=None,
                cache_series: bool = False) -> dict:
    from flairhip.configs import unet_resnet34_config
    cfg = unet_resnet34_config(in_channels=5, precision=precision, batch_size=batch)
    mods = cfg["modalities"]
    mods["inputs"][DEM] = bool(dem)
    mods["pre_processings"].update(calc_elevation=bool(dem), use_augmentation=True)
    mods["normalization"] = {k: v for k, v in NORMALIZATION.items() if dem or not k.startswith(DEM)}
    if sentinel2:
        mods["inputs"][S2] = True
        mods["inputs_channels"][S2] = list(range(1, 11))
        mods["pre_processings"].update(filter_sentinel2=False, filter_sentinel2_max_cloud=1, filter_sentinel2_max_snow=1,
                                       filter_sentinel2_max_frac_cover=0.05, temporal_average_sentinel2=s2_average or False,
                                       temporal_average_sentinel1=False)
    cfg["hyperparams"].update(num_epochs=epochs, scheduler=None)
    cfg["hardware"].update(hip_graph=hip_graph, sample_cache=cache, sample_cache_series=bool(cache_series))
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
    ap.add_argument("--sentinel2", type=int, nargs=2, metavar=("TMIN", "TMAX"), default=None)
    ap.add_argument("--s2-size", type=int, default=10)
    ap.add_argument("--s2-average", choices=("monthly", "semi-monthly"), default=None)
    ap.add_argument("--cache-series", action="store_true")
    args = ap.parse_args()
    if args.sentinel2 and not 1 <= args.sentinel2[0] <= args.sentinel2[1] <= 365:
        ap.error("--sentinel2 TMIN TMAX: 1 <= TMIN <= TMAX <= 365")
    root = os.path.abspath(args.dir)
    csvs = write_dataset(root, args.patches, args.size, args.dem_size, args.val, args.seed, sentinel2=args.sentinel2,
                         s2_size=args.s2_size)
    cfg = make_config(root, csvs, args.cache, args.batch, args.epochs, args.precision, sentinel2=bool(args.sentinel2),
                      s2_average=args.s2_average, cache_series=args.cache_series)
    os.makedirs(os.path.join(root, "config"), exist_ok=True)
    for key, value in cfg.items():  # one file per top-level key: read_config merges them
        with open(os.path.join(root, "config", f"{key}.yaml"), "w") as f:
            yaml.safe_dump({key: value}, f)
    print(f"{args.patches} patches under {root}/patches; python -m flair_hub.main --config {root}/config")


if __name__ == "__main__":
    main()
