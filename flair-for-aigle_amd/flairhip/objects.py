"""Object matching on the host: from the region tables and the overlap list of two class maps
(``flairhip.ops.region_overlaps``, include/flairhip_objects.h) to matched objects, per-class TP / FP / FN and
precision / recall / F1.  numpy only; the pixel work was done on the device, what is left is as long as the pair list.

A is the prediction and B the reference throughout."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

CLASS_MODES = ("same", "any")


def _np(t, dtype):
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=dtype)


@dataclass
class ObjectMatches:
    """Per region of A: ``a_match`` int64 (index in B or -1), ``a_match_iou`` float64 (the IoU of that match, 0.0
    without one), ``a_best_iou`` float64 (greatest IoU with any candidate, 0.0 without one), ``a_covered`` float64 (sum
    of the shared pixels over its candidates divided by its pixels, in [0, 1]); the same four for B."""
    a_match: np.ndarray
    a_match_iou: np.ndarray
    a_best_iou: np.ndarray
    a_covered: np.ndarray
    b_match: np.ndarray
    b_match_iou: np.ndarray
    b_best_iou: np.ndarray
    b_covered: np.ndarray


def match_objects(ov, iou_threshold: float = 0.5, classes: str = "same") -> ObjectMatches:
    """One-to-one matching of the regions of A and B.  Candidates are the pairs of ``ov`` (with ``classes="same"`` only
    those whose two regions have the same class); IoU = n / (pa + pb - n) in float64 from the exact integers; pairs are
    taken greedily by descending IoU, ties to the smaller (ia, ib), and accepted while both regions are free and
    IoU >= ``iou_threshold``."""
    if classes not in CLASS_MODES:
        raise ValueError(f"match_objects: classes must be one of {CLASS_MODES}, got {classes!r}")
    a_pix, b_pix = _np(ov.a_pixels, np.int64), _np(ov.b_pixels, np.int64)
    ia, ib, n = _np(ov.pair_a, np.int64), _np(ov.pair_b, np.int64), _np(ov.pair_pixels, np.int64)
    Pa, Pb = len(a_pix), len(b_pix)
    if classes == "same" and len(ia):
        same = _np(ov.a_class, np.int64)[ia] == _np(ov.b_class, np.int64)[ib]
        ia, ib, n = ia[same], ib[same], n[same]
    iou = n.astype(np.float64) / (a_pix[ia] + b_pix[ib] - n).astype(np.float64) if len(ia) else np.zeros(0)
    out = ObjectMatches(np.full(Pa, -1, np.int64), np.zeros(Pa), np.zeros(Pa), np.zeros(Pa),
                        np.full(Pb, -1, np.int64), np.zeros(Pb), np.zeros(Pb), np.zeros(Pb))
    if not len(ia):
        return out
    np.maximum.at(out.a_best_iou, ia, iou)
    np.maximum.at(out.b_best_iou, ib, iou)
    out.a_covered = np.bincount(ia, weights=n, minlength=Pa) / np.maximum(a_pix, 1)
    out.b_covered = np.bincount(ib, weights=n, minlength=Pb) / np.maximum(b_pix, 1)
    order = np.lexsort((ib, ia, -iou))  # the last key is the primary one
    order = order[iou[order] >= iou_threshold]
    for k in order.tolist():
        x, y = int(ia[k]), int(ib[k])
        if out.a_match[x] < 0 and out.b_match[y] < 0:
            out.a_match[x], out.b_match[y] = y, x
            out.a_match_iou[x] = out.b_match_iou[y] = iou[k]
    return out


def object_counts(ov, matches: ObjectMatches, num_classes: int):
    """(int64 [K, 3] of TP, FP, FN per class, float64 [K] sums of matched IoU).  TP: a matched region of A of that
    class; FP: an unmatched region of A; FN: an unmatched region of B.  Regions of a class >= K count nowhere.  Both
    results are additive over patches and ranks."""
    K = int(num_classes)
    a_cls, b_cls = _np(ov.a_class, np.int64), _np(ov.b_class, np.int64)
    counts = np.zeros((K, 3), np.int64)
    iou_sums = np.zeros(K, np.float64)
    a_in, b_in = a_cls < K, b_cls < K
    hit = matches.a_match >= 0
    counts[:, 0] = np.bincount(a_cls[a_in & hit], minlength=K)
    counts[:, 1] = np.bincount(a_cls[a_in & ~hit], minlength=K)
    counts[:, 2] = np.bincount(b_cls[b_in & (matches.b_match < 0)], minlength=K)
    iou_sums += np.bincount(a_cls[a_in & hit], weights=matches.a_match_iou[a_in & hit], minlength=K)
    return counts, iou_sums


def _ratio(num, den):
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    out = np.full(num.shape, np.nan)
    np.divide(num, den, out=out, where=den > 0)
    return out


def object_scores(counts, iou_sums) -> dict:
    """Precision TP / (TP + FP), recall TP / (TP + FN), F1 2 TP / (2 TP + FP + FN) and mean matched IoU per class
    (float64 [K] arrays under "precision", "recall", "f1", "mean_matched_iou", with "tp", "fp", "fn") and over the
    summed counts (the same keys under "micro").  A value whose denominator is 0 is nan (``scores_json``: None)."""
    counts = np.asarray(counts, np.int64).reshape(-1, 3)
    iou_sums = np.asarray(iou_sums, np.float64).reshape(-1)

    def scores(tp, fp, fn, s):
        return {"tp": tp, "fp": fp, "fn": fn, "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
                "f1": _ratio(2 * tp, 2 * tp + fp + fn), "mean_matched_iou": _ratio(s, tp)}

    out = scores(counts[:, 0], counts[:, 1], counts[:, 2], iou_sums)
    micro = scores(counts[:, 0].sum(), counts[:, 1].sum(), counts[:, 2].sum(), iou_sums.sum())
    out["micro"] = {k: (int(v) if k in ("tp", "fp", "fn") else float(v)) for k, v in micro.items()}
    return out


def _json_value(v):
    if isinstance(v, (int, np.integer)):
        return int(v)
    v = float(v)
    return None if v != v else v


def scores_json(scores: dict, names=None) -> dict:
    """``object_scores``'s result as plain JSON values: {"classes": {name: {tp, fp, fn, precision, recall, f1,
    mean_matched_iou}}, "micro": {...}}, nan as None.  ``names``: class names by index (default: the indices)."""
    keys = ("tp", "fp", "fn", "precision", "recall", "f1", "mean_matched_iou")
    K = len(scores["tp"])
    names = [str(i) for i in range(K)] if names is None else [str(n) for n in names]
    return {"classes": {names[k]: {key: _json_value(scores[key][k]) for key in keys} for k in range(K)},
            "micro": {key: _json_value(scores["micro"][key]) for key in keys}}
