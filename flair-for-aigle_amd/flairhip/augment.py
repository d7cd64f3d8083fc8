"""Training augmentation: per-sample flips and rotations by k * 90 degrees, as the reference draws and applies them
(flair_hub/data/utils_data/augmentations.py:6-48: one random choice per sample, applied to every input modality and
every label).

Here a sample's choice is one uint8 code that rides along in the batch as ``batch["AUG"]`` and steers the gather of the
layout / label kernels on the device (ops.d4_layout, ops.d4_labels, ops.d4_onehot_to_index):

    bit 0     horizontal flip (axis -1)
    bit 1     vertical flip (axis -2)
    bits 2-3  k of np.rot90(k, axes=(-2, -1))

applied in the reference's order: flip axis -1, flip axis -2, rot90.  The 16 codes give the 8 transforms of the square.
This module is the host statement: numpy only, no GPU.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

HFLIP, VFLIP, ROT_SHIFT = 1, 2, 2


def make_code(hflip: bool, vflip: bool, k: int) -> int:
    return (HFLIP if hflip else 0) | (VFLIP if vflip else 0) | ((int(k) & 3) << ROT_SHIFT)


def draw_codes(n: int, p_flip: float = 0.5, p_rot: float = 0.5, rng=np.random) -> np.ndarray:
    """n codes; per sample the generator is consumed exactly as the reference's apply_numpy_augmentations consumes
    np.random (rand, rand, rand, and randint(1, 4) only when the rotation was drawn), so the same seed gives the
    transforms the reference's dataset would draw.  ``rng``: np.random or a np.random.RandomState."""
    codes = np.empty(n, dtype=np.uint8)
    for s in range(n):
        hflip = rng.rand() < p_flip
        vflip = rng.rand() < p_flip
        rot = rng.rand() < p_rot
        k = rng.randint(1, 4) if rot else 0
        codes[s] = make_code(hflip, vflip, k)
    return codes


def d4_source_index(code: int, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(si, sj), each int64 [n, n]: the transformed plane is ``plane[..., si, sj]`` -- the gather the kernels implement"""
    code = int(code) & 15
    si, sj = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for _ in range(code >> ROT_SHIFT):
        si, sj = sj, n - 1 - si
    if code & VFLIP:
        si = n - 1 - si
    if code & HFLIP:
        sj = n - 1 - sj
    return si, sj


def apply_code(arr: np.ndarray, code: int) -> np.ndarray:
    """the transform of ``code`` over the last two axes of ``arr`` (a contiguous copy)"""
    if arr.shape[-1] != arr.shape[-2]:
        raise ValueError(f"rotations need square planes, got {arr.shape[-2]} x {arr.shape[-1]}")
    si, sj = d4_source_index(code, arr.shape[-1])
    return np.ascontiguousarray(arr[..., si, sj])


def rank_epoch_rng(seed: int, rank: int, epoch: int) -> np.random.RandomState:
    """the generator HipTrainer draws a training epoch's codes from: ranks and epochs get streams of their own"""
    return np.random.RandomState([int(seed) & 0xffffffff, int(rank), int(epoch)])
