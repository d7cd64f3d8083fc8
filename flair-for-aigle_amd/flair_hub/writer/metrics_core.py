"""Scores of a confusion matrix (rows = target, columns = prediction), in percent -- counterpart of the reference's
flair_hub/writer/metrics_core.py.  numpy only.  A class without support has 0 / 0 = NaN in a ratio: the per-class scores
report 0 there, as the reference does; no warning escapes (np.errstate)."""
from __future__ import annotations

from typing import Tuple

import numpy as np


def _percent(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        r = 100 * np.asarray(num) / np.asarray(den)
    r[np.isnan(r)] = 0
    return r


def overall_accuracy(npcm: np.ndarray) -> float:
    """100 * trace / total; NaN for an empty matrix (the reference's value)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return 100 * (np.trace(npcm) / npcm.sum())


def class_IoU(npcm: np.ndarray, n_class: int) -> Tuple[np.ndarray, float]:
    tp = np.diag(npcm)
    ious = _percent(tp, np.sum(npcm, axis=1) + np.sum(npcm, axis=0) - tp)
    return ious, np.mean(ious)


def class_precision(npcm: np.ndarray) -> Tuple[np.ndarray, float]:
    precision = _percent(np.diag(npcm), np.sum(npcm, axis=0))
    return precision, np.mean(precision)


def class_recall(npcm: np.ndarray) -> Tuple[np.ndarray, float]:
    recall = _percent(np.diag(npcm), np.sum(npcm, axis=1))
    return recall, np.mean(recall)


def class_fscore(precision: np.ndarray, recall: np.ndarray) -> Tuple[np.ndarray, float]:
    with np.errstate(divide="ignore", invalid="ignore"):
        fscore = 2 * (precision * recall) / (precision + recall)
    fscore[np.isnan(fscore)] = 0
    return fscore, np.mean(fscore)
