"""Input normalisation -- counterpart of the reference's flair_hub/data/utils_data/norm.py (norm :8-52)."""
from __future__ import annotations

import logging
from typing import Sequence

import numpy as np

logger = logging.getLogger(__name__)

NORM_TYPES = ("scaling", "custom", "without")


def norm(in_img: np.ndarray, norm_type: str = None, means: Sequence[float] = (), stds: Sequence[float] = ()) -> np.ndarray:
    """``custom``: float64 (x - means[c]) / stds[c] per channel of axis 0, the reference's arithmetic (:41-44);
    ``scaling``: unsigned integers divided by their type's maximum (what skimage.img_as_float does for them), floats
    unchanged -- signed integers raise ValueError, skimage's rule for them is not restated here; ``without``: the input.
    Any other ``norm_type``, or means and stds of different lengths, ends the program as in the reference (SystemExit)."""
    if norm_type not in NORM_TYPES:
        logger.info("Error: Normalization argument should be 'scaling', 'custom', or 'without'.")
        raise SystemExit(1)
    if norm_type == "custom":
        if len(means) != len(stds):
            logger.info("Error: If using 'custom', the provided means and stds must have the same length.")
            raise SystemExit(1)
        out = in_img.astype(np.float64)
        for c in range(out.shape[0]):
            out[c] -= means[c]
            out[c] /= stds[c]
        return out
    if norm_type == "scaling":
        kind = in_img.dtype.kind
        if kind == "f":
            return in_img
        if kind == "u":
            return in_img.astype(np.float64) / float(np.iinfo(in_img.dtype).max)
        raise ValueError(f"norm_type 'scaling' takes unsigned integer or float samples, got {in_img.dtype}")
    return in_img
