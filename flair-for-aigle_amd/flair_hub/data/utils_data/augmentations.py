"""Host-side training augmentation -- counterpart of the reference's flair_hub/data/utils_data/augmentations.py
(apply_numpy_augmentations :6-48), for the reference batch schema (device_prepare=False).  The draws are
flairhip.augment.draw_codes', which consumes np.random exactly as the reference does, and the transform is
flairhip.augment.apply_code -- the gather the device kernels implement."""
from __future__ import annotations

from typing import Dict, List

import numpy as np

from flairhip.augment import apply_code, draw_codes


def apply_numpy_augmentations(batch_dict: Dict[str, np.ndarray], input_keys: List[str], label_keys: List[str],
                              p_flip: float = 0.5, p_rot: float = 0.5) -> Dict[str, np.ndarray]:
    """one flip / rotation choice per sample, applied to every plane of every input and label of the sample"""
    code = int(draw_codes(1, p_flip, p_rot, rng=np.random)[0])
    for key in input_keys + label_keys:
        batch_dict[key] = apply_code(np.asarray(batch_dict[key]), code)
    return batch_dict
