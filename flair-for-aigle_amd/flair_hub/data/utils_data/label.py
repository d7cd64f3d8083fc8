"""Label encoding -- counterpart of the reference's flair_hub/data/utils_data/label.py (reshape_label_ohe :3-14)."""
from __future__ import annotations

import numpy as np


def reshape_label_ohe(arr: np.ndarray, num_classes: int) -> np.ndarray:
    """bool [num_classes, H, W]: plane k is ``label == k``.  A value >= num_classes is true in no plane, so the argmax
    the task takes over the planes (tasks_module.py:153) makes it class 0 -- the rule ops.gather_labels implements."""
    if arr.shape[0] == 1:
        arr = arr.squeeze(0)
    return np.stack([arr == k for k in range(num_classes)], axis=0)

