#!/usr/bin/env python
"""tests/golden/augment_d4.npz: inputs and outputs of the reference's own apply_numpy_augmentations
(/root/reference/flair_hub/data/utils_data/augmentations.py:6-48, numpy only, imports cleanly) for seeds that between
them draw all 16 (hflip, vflip, k) codes of flairhip.augment: per seed the reference's outputs for one small sample
(uint8 aerial, f32 elevation, uint16 Sentinel series, f32 one-hot label) and the next np.random.rand() after the call,
which pins how much of the generator the call consumed."""
import os
import sys

import numpy as np

sys.path.insert(0, "/root/reference")
from flair_hub.data.utils_data.augmentations import apply_numpy_augmentations  # noqa: E402

r = np.random.RandomState(7)
inputs = {
    "AERIAL_RGBI": r.randint(0, 256, (5, 12, 12)).astype(np.uint8),
    "DEM_ELEV": r.randn(2, 9, 9).astype(np.float32),
    "SENTINEL2_TS": r.randint(0, 10000, (3, 4, 10, 10)).astype(np.uint16),
}
cls = r.randint(0, 19, (12, 12))
inputs["AERIAL_LABEL-COSIA"] = np.ascontiguousarray(np.eye(19, dtype=np.float32)[cls].transpose(2, 0, 1))
in_keys, lab_keys = ["AERIAL_RGBI", "DEM_ELEV", "SENTINEL2_TS"], ["AERIAL_LABEL-COSIA"]


def drawn_code(seed):  # which code the seed stands for (bit 0 hflip, bit 1 vflip, bits 2-3 k)
    np.random.seed(seed)
    h, v, rot = np.random.rand() < 0.5, np.random.rand() < 0.5, np.random.rand() < 0.5
    k = np.random.randint(1, 4) if rot else 0
    return int(h) | (int(v) << 1) | (k << 2)


first = {}
for seed in range(400):
    first.setdefault(drawn_code(seed), seed)
assert sorted(first) == list(range(16)), sorted(first)

save = {"in_" + k: v for k, v in inputs.items()}
seeds, codes, nxt = [], [], []
for code in range(16):
    seed = first[code]
    np.random.seed(seed)
    out = apply_numpy_augmentations({k: v.copy() for k, v in inputs.items()}, in_keys, lab_keys)
    nxt.append(np.random.rand())
    seeds.append(seed)
    codes.append(code)
    for k, v in out.items():
        assert v.dtype == inputs[k].dtype and v.shape == inputs[k].shape
        save[f"out{code:02d}_{k}"] = np.ascontiguousarray(v)
save["seeds"] = np.array(seeds, dtype=np.int64)
save["codes"] = np.array(codes, dtype=np.uint8)
save["next_rand"] = np.array(nxt, dtype=np.float64)
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment_d4.npz")
np.savez_compressed(path, **save)
print(dict(zip(codes, seeds)), os.path.getsize(path), "bytes")
