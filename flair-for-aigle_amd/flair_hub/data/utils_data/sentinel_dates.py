"""Sentinel acquisition dates -- counterpart of the reference's flair_hub/data/utils_data/sentinel_dates.py
(prepare_sentinel_dates :10-54, get_sentinel_dates_mtd :57-83).  The GLOBAL_*_MTD_DATES.gpkg files are SQLite
databases: the feature table is found through gpkg_contents and its columns patch_id and acquisition_dates (a JSON
object of 'YYYYMMDD' strings) are read with sqlite3 -- no geopandas, the geometries are never needed."""
from __future__ import annotations

import datetime
import json
import logging
import sqlite3
from typing import Any, Dict, Set, Tuple

import numpy as np

logger = logging.getLogger(__name__)


def _feature_rows(file_path: str):
    """(patch_id, acquisition_dates) of every row of the GeoPackage's feature table"""
    con = sqlite3.connect(f"file:{file_path}?mode=ro", uri=True)
    try:
        tables = [r[0] for r in con.execute(
            "SELECT table_name FROM gpkg_contents WHERE data_type = 'features' ORDER BY table_name")]
        for table in tables:
            cols = {r[1] for r in con.execute(f'PRAGMA table_info("{table}")')}
            if {"patch_id", "acquisition_dates"} <= cols:
                return con.execute(f'SELECT patch_id, acquisition_dates FROM "{table}" ORDER BY rowid').fetchall()
        raise ValueError(f"{file_path}: no feature table with the columns patch_id and acquisition_dates")
    finally:
        con.close()


def prepare_sentinel_dates(config: Dict[str, Any], file_path: str, patch_ids: Set[str]) -> Dict[str, Dict[str, np.ndarray]]:
    """{patch id: {'dates': datetimes, 'diff_dates': days since config's ref_date ('MM-DD') of the same year}} for the
    patches in ``patch_ids``; a date that does not parse is logged and left out"""
    ref_month, ref_day = (int(v) for v in config["models"]["multitemp_model"]["ref_date"].split("-"))
    out: Dict[str, Dict[str, np.ndarray]] = {}
    for patch_id, raw in _feature_rows(file_path):
        if patch_id not in patch_ids:
            continue
        dates, diffs = [], []
        for text in json.loads(raw).values():
            try:
                day = datetime.datetime.strptime(text, "%Y%m%d")
                ref = datetime.datetime(day.year, ref_month, ref_day)
            except ValueError as e:
                logger.info("Invalid date encountered: %s. Error: %s", text, e)
                continue
            dates.append(day)
            diffs.append((day - ref).days)
        out[patch_id] = {"dates": np.array(dates), "diff_dates": np.array(diffs)}
    return out


def get_sentinel_dates_mtd(config: dict, patch_ids: set) -> Tuple[Dict, Dict, Dict]:
    """the three date tables (Sentinel-2, Sentinel-1 ascending, descending) of the active time-series modalities, read
    from config['paths']['global_mtd_folder']; an inactive modality gets an empty table"""
    assert isinstance(config, dict), "config must be a dictionary"
    inputs = config["modalities"]["inputs"]
    tables = []
    for key, stem in (("SENTINEL2_TS", "SENTINEL2"), ("SENTINEL1-ASC_TS", "SENTINEL1-ASC"),
                      ("SENTINEL1-DESC_TS", "SENTINEL1-DESC")):
        if inputs.get(key, False):
            tables.append(prepare_sentinel_dates(
                config, config["paths"]["global_mtd_folder"] + f"GLOBAL_{stem}_MTD_DATES.gpkg", patch_ids))
        else:
            tables.append({})
    return tuple(tables)
