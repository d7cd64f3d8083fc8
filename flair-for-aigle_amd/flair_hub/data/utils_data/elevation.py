"""Elevation pre-processing -- counterpart of the reference's flair_hub/data/utils_data/elevation.py (:3-12)."""
from __future__ import annotations

import numpy as np


def calc_elevation(arr: np.ndarray) -> np.ndarray:
    """[1, H, W]: band 0 (surface model) minus band 1 (terrain model), in the array's own type"""
    return (arr[0] - arr[1])[np.newaxis, :, :]
