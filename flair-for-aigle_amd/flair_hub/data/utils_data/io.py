"""Patch reads -- counterpart of the reference's flair_hub/data/utils_data/io.py (read_patch :4-15), over
flair_zonal_detection.raster.open_raster: rasterio when it is installed, the project's own GeoTIFF reader otherwise."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from flair_zonal_detection.raster import open_raster


def read_patch(raster_file: str, channels: Optional[Sequence[int]] = None) -> np.ndarray:
    """[C, H, W] in the file's sample type: the 1-based ``channels``, or every band when none are named"""
    with open_raster(str(raster_file)) as src:
        return src.read(list(channels)) if channels else src.read()
