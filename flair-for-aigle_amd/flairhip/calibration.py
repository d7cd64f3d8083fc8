"""Calibrated class thresholds: the host side.

The device side is ``ops.calib_hist`` (the score histograms of a validation split) and ``ops.predict_thresholded_u8`` /
``ops.tta_predict_thresholded_u8`` (labels under per-class thresholds); the definitions are in
include/flairhip_calib.h.  Everything here is numpy on the ``[K, 2, 256]`` integers ``hist[k, side, q]`` (side 1: the
pixel's target is class k) and the ``best_thresholds.yaml`` file the reference looks for next to a checkpoint
(utils/s3.py prepare_local_model_folder) and hands on as ``config["model_threshold_filepath"]``.

The sweep scores the one-vs-rest masks ``{q_k >= t}``.  The label rule lets the runner-up take a pixel whose best class
was rejected, so the two coincide only where ``t > 128`` (at most one class holds such a score); what the combined rule
really scores is measured by a second pass over the split (flair_hub.tasks.stages.calibrate_stage).
"""
from __future__ import annotations

import math
import os
from typing import Any, Dict, Optional, Sequence

import numpy as np

FILE_NAME = "best_thresholds.yaml"
OBJECTIVES = ("iou", "f1")


def _hist(hist) -> np.ndarray:
    if hasattr(hist, "detach"):
        hist = hist.detach().cpu().numpy()
    h = np.asarray(hist)
    if h.ndim != 3 or h.shape[1:] != (2, 256) or not np.issubdtype(h.dtype, np.integer):
        raise ValueError(f"score histograms are integers [K, 2, 256], got {h.dtype} {h.shape}")
    return h.astype(np.int64)


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    """float64 num / den, 0 where den is 0"""
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num, den, out=out, where=den != 0)
    return out


def sweep(hist) -> Dict[str, np.ndarray]:
    """Per class and threshold t = 0..255, all [K, 256]: ``tp`` = pos with q >= t, ``fp`` = neg with q >= t, ``fn`` =
    pos with q < t (exact int64), and ``iou`` = tp / (tp + fp + fn), ``precision``, ``recall``, ``f1`` (float64
    divisions of the integers, 0 / 0 = 0)."""
    h = _hist(hist)
    neg, pos = h[:, 0], h[:, 1]
    tp = np.cumsum(pos[:, ::-1], axis=1)[:, ::-1]
    fp = np.cumsum(neg[:, ::-1], axis=1)[:, ::-1]
    fn = pos.sum(axis=1, keepdims=True) - tp
    return {"tp": tp, "fp": fp, "fn": fn, "iou": _ratio(tp, tp + fp + fn), "precision": _ratio(tp, tp + fp),
            "recall": _ratio(tp, tp + fn), "f1": _ratio(2 * tp, 2 * tp + fp + fn)}


def best_thresholds(hist, objective: str = "iou", min_support: int = 1) -> np.ndarray:
    """uint8 [K]: per class the t in 1..255 that maximises the objective, the smallest on a tie; 0 (no constraint) for
    a class with fewer than ``min_support`` target pixels."""
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be one of {OBJECTIVES}, got {objective!r}")
    h = _hist(hist)
    score = sweep(h)[objective][:, 1:]
    best = 1 + np.argmax(score, axis=1)  # the first maximum: the smallest t
    support = h[:, 1].sum(axis=1)
    return np.where(support >= max(int(min_support), 1), best, 0).astype(np.uint8)


def expected_calibration_error(hist) -> np.ndarray:
    """float64 [K]: the one-vs-rest ECE per class over the 256 score bins, sum_q n_q / N * |pos_q / n_q - q / 255|
    (0 for a class without pixels)."""
    h = _hist(hist)
    n = h.sum(axis=1)
    gap = np.abs(_ratio(h[:, 1], n) - np.arange(256, dtype=np.float64) / 255.0)
    return _ratio((n * gap).sum(axis=1), n.sum(axis=1))


def iou_from_confmat(confmat, support=None) -> np.ndarray:
    """float64 [K] per-class IoU of an integer confusion matrix (rows = target), 0 / 0 = 0.  ``support`` [K]: the
    number of target pixels per class where the rows do not hold them all -- a fallback label >= K has no column, and
    its pixels are still misses of their target class."""
    cm = np.asarray(confmat, dtype=np.int64)
    tp = np.diag(cm)
    rows = cm.sum(axis=1) if support is None else np.asarray(support, dtype=np.int64)
    return _ratio(tp, cm.sum(axis=0) + rows - tp)


def _u8_list(values, what: str):
    out = [int(v) for v in values]
    if any(not 0 <= v <= 255 or v != f for v, f in zip(out, values)):
        raise ValueError(f"{what} must be integers in 0..255, got {list(values)}")
    return out


def write_thresholds(path: str, thresholds: Sequence[int], class_names: Optional[Sequence[str]] = None,
                     extra: Optional[Dict[str, Any]] = None, task: str = "default") -> str:
    """Write (or update the mapping of ``task`` in) a threshold file: ``thresholds`` (floats t / 255), ``thresholds_u8``,
    ``class_names`` and whatever ``extra`` holds (objective, fallback, per-class statistics).  -> path"""
    import yaml
    thr = _u8_list(np.asarray(thresholds).tolist(), "thresholds")
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = yaml.safe_load(f) or {}
    entry = {"thresholds": [t / 255.0 for t in thr], "thresholds_u8": thr}
    if class_names is not None:
        entry["class_names"] = [str(n) for n in class_names]
    for k, v in (extra or {}).items():
        entry[k] = v.tolist() if isinstance(v, np.ndarray) else v.item() if isinstance(v, np.generic) else v
    doc[str(task)] = entry
    with open(path, "w") as f:
        yaml.safe_dump(doc, f, sort_keys=False)
    return path


def read_thresholds(path: str, num_classes: int, task: Optional[str] = None) -> Dict[str, Any]:
    """-> {'thresholds_u8': uint8 [K], 'fallback': int or None, 'entry': the task's mapping}.  The file holds one
    mapping per task or is such a mapping itself; ``task`` picks its own mapping, a file with a single mapping serves
    every task, ``task`` None takes the first.  ``thresholds`` are floats
    tau in [0, 1], read as ceil(255 tau - 1e-9) -- the smallest byte whose score is >= tau -- clipped to 0..255;
    ``thresholds_u8`` are accepted in their place (and win where both are there).  A length other than
    ``num_classes`` raises ValueError."""
    import yaml
    with open(path) as f:
        doc = yaml.safe_load(f)
    if not isinstance(doc, dict) or not doc:
        raise ValueError(f"{path}: not a threshold file")
    if "thresholds" in doc or "thresholds_u8" in doc:
        entry = doc
    else:
        if task is not None and task not in doc and len(doc) > 1:
            raise ValueError(f"{path}: no thresholds for task {task!r} (it holds {sorted(doc)})")
        entry = doc[task] if task in doc else next(iter(doc.values()))
        if not isinstance(entry, dict) or not ("thresholds" in entry or "thresholds_u8" in entry):
            raise ValueError(f"{path}: not a threshold file")
    if entry.get("thresholds_u8") is not None:
        thr = _u8_list(entry["thresholds_u8"], f"{path}: thresholds_u8")
    else:
        taus = [float(t) for t in entry["thresholds"]]
        if any(not 0.0 <= t <= 1.0 for t in taus):
            raise ValueError(f"{path}: thresholds must lie in [0, 1], got {taus}")
        thr = [min(max(int(math.ceil(255.0 * t - 1e-9)), 0), 255) for t in taus]
    if len(thr) != int(num_classes):
        raise ValueError(f"{path}: {len(thr)} thresholds for {int(num_classes)} classes")
    fallback = entry.get("fallback")
    return {"thresholds_u8": np.asarray(thr, dtype=np.uint8), "fallback": None if fallback is None else int(fallback),
            "entry": entry}
