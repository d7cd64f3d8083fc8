"""Configuration files -- counterpart of the reference's flair_hub/utils/config_io.py (read_config :11-37,
setup_environment :40-52): one YAML file, or a directory of them merged by top-level key."""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, Tuple

import yaml


def read_config(path: str) -> Dict[str, dict]:
    if os.path.isfile(path) and str(path).endswith(".yaml"):
        files = [str(path)]
    elif os.path.isdir(path):
        files = [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".yaml")]
    else:
        raise ValueError(f"Invalid path: {path}. Must be a .yaml file or a directory containing .yaml files.")
    merged: Dict[str, dict] = {}
    for file in files:
        with open(file, "r") as f:
            part = yaml.safe_load(f)
        if isinstance(part, dict):
            merged.update(part)
    return merged


def setup_environment(args) -> Tuple[Dict[str, dict], Path]:
    """(config, output directory paths.out_folder / paths.out_model_name, created)"""
    config = read_config(args.config)
    out_dir = Path(config["paths"]["out_folder"], config["paths"]["out_model_name"])
    out_dir.mkdir(parents=True, exist_ok=True)
    return config, out_dir
