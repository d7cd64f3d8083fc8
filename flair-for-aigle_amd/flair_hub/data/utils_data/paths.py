"""Dataset file lists -- counterpart of the reference's flair_hub/data/utils_data/paths.py (extract_sentinel_patch_ids
:10-29, get_paths :32-74, get_datasets :77-105).  The split CSVs (one column per modality and label, one row per patch)
are read with the csv module; no pandas."""
from __future__ import annotations

import csv
import logging
import os
from typing import Any, Dict, Iterable, List, Optional, Set, Tuple

from flair_hub.data.utils_data.sentinel_dates import get_sentinel_dates_mtd

logger = logging.getLogger(__name__)

SENTINEL_KEYS = ("SENTINEL2_TS", "SENTINEL1-ASC_TS", "SENTINEL1-DESC_TS")
SPLIT_KEYS = {"train": "train_csv", "val": "val_csv", "test": "test_csv"}


def extract_sentinel_patch_ids(dicts: Iterable[Optional[Dict]]) -> Set[str]:
    """the patch ids of every Sentinel file the splits name: the file name without '_<MODALITY>' and '.tif'"""
    ids: Set[str] = set()
    for d in dicts:
        for key in SENTINEL_KEYS if d is not None else ():
            for path in d.get(key, []):
                ids.add(path.split("/")[-1].replace(f"_{key}", "").replace(".tif", ""))
    return ids


def _read_columns(csv_path: str) -> Dict[str, List[str]]:
    with open(csv_path, newline="") as f:
        rows = list(csv.DictReader(f))
    names = list(rows[0].keys()) if rows else []
    return {n: [r[n] for r in rows] for n in names}


def get_paths(config: Dict[str, Any], split: str = "train") -> Dict:
    """{modality or label: [paths]} of one split; an inactive modality keeps an empty list.  An unknown split or a
    missing CSV ends the program (SystemExit), as in the reference."""
    if split not in SPLIT_KEYS:
        logger.info("Invalid split specified.")
        raise SystemExit()
    csv_path = config["paths"].get(SPLIT_KEYS[split])
    if not (csv_path is not None and os.path.isfile(csv_path) and str(csv_path).endswith(".csv")):
        logger.info("Invalid .csv file path for %s split.", split)
        raise SystemExit()
    columns = _read_columns(csv_path)
    inputs = config["modalities"]["inputs"]
    out: Dict[str, list] = {m: [] for m in inputs}
    for m, on in inputs.items():
        if on is True and m in columns:
            out[m] = columns[m]
    for task in config["labels"]:
        out[task] = columns[task]
    out["SENTINEL2_MSK-SC"] = columns["SENTINEL2_MSK-SC"] if inputs.get("SENTINEL2_TS") else []
    return out


def get_datasets(config: Dict[str, Any]) -> Tuple[Optional[Dict], Optional[Dict], Optional[Dict]]:
    """(train, val, test) file lists as config['tasks'] asks for them, each with the Sentinel acquisition dates of the
    patches in use under DATES_S2 / DATES_S1_ASC / DATES_S1_DESC"""
    train = val = test = None
    if config["tasks"]["train"]:
        train, val = get_paths(config, "train"), get_paths(config, "val")
    if config["tasks"]["predict"]:
        test = get_paths(config, "test")
    splits = [train, val, test]
    s2, s1a, s1d = get_sentinel_dates_mtd(config, extract_sentinel_patch_ids(splits))
    for d in splits:
        if d is not None:
            d["DATES_S2"], d["DATES_S1_ASC"], d["DATES_S1_DESC"] = s2, s1a, s1d
    return train, val, test
