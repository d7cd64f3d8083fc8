"""Training augmentation: per-sample flips and rotations by k * 90 degrees, as the reference draws and applies them
(flair_hub/data/utils_data/augmentations.py:6-48: one random choice per sample, applied to every input modality and
every label).  The same codes name the views of test-time augmentation (the zonal config key ``tta``): inverse_code,
TTA_VIEWS and tta_mean_probabilities below state the way back from a view to the tile's frame.

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


def inverse_code(code: int) -> int:
    """the code c' in 0..7 with apply_code(apply_code(a, code), c') == a for every square a.  In the closed form of
    d4_source_index -- the source row is the destination row or column (odd k), each source coordinate possibly
    mirrored -- a transform without the swap is its own inverse and one with it exchanges its two mirror flags: codes 4
    and 7 (the quarter turns) are each other's inverses, the other six of 0..7 their own; 8..15 alias 0..7."""
    code = int(code) & 15
    k = code >> ROT_SHIFT
    swap = k & 1
    fi = (k >> 1) ^ ((code >> 1) & 1)         # mirrored source row
    fj = (1 if k in (1, 2) else 0) ^ (code & 1)  # mirrored source column
    if swap:
        fi, fj = fj, fi
        return make_code(not fj, bool(fi), 1)  # with k = 1: fi = vflip, fj = not hflip
    return make_code(bool(fj), bool(fi), 0)


TTA_VIEWS = {"none": (0,), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def tta_views(name: str) -> Tuple[int, ...]:
    """the forward codes of the views of test-time augmentation ``name``: none, flips or d4"""
    if not isinstance(name, str) or name not in TTA_VIEWS:
        raise ValueError(f"tta must be one of {', '.join(TTA_VIEWS)}, got {name!r}")
    return TTA_VIEWS[name]


def tta_mean_probabilities(logits_by_view, codes) -> np.ndarray:
    """Test-time augmentation as a definition, in float64: ``logits_by_view[v]`` is [..., K, n, n], the logits of the
    view made with forward code ``codes[v]``, in that view's frame.  One softmax per view over the class axis (-3),
    each view taken back to the tile's frame with inverse_code, the mean over the views: [..., K, n, n].  The kernels
    behind ops.tta_accumulate_ / tta_predict_u8 / tta_probabilities implement this."""
    if len(logits_by_view) != len(codes) or not len(codes):
        raise ValueError(f"{len(logits_by_view)} views for {len(codes)} codes")
    total = None
    for logits, code in zip(logits_by_view, codes):
        z = np.asarray(logits, dtype=np.float64)
        e = np.exp(z - z.max(axis=-3, keepdims=True))
        p = apply_code(e / e.sum(axis=-3, keepdims=True), inverse_code(code))
        total = p if total is None else total + p
    return total / len(codes)


def rank_epoch_rng(seed: int, rank: int, epoch: int) -> np.random.RandomState:
    """the generator HipTrainer draws a training epoch's codes from: ranks and epochs get streams of their own"""
    return np.random.RandomState([int(seed) & 0xffffffff, int(rank), int(epoch)])
