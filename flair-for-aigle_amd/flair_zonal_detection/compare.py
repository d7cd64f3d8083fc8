"""Run against run, run against truth: the objects of two class rasters on one grid, matched.

``compare_objects(pred, ref)`` polygonises both rasters with the same options and matches their regions one to one
(GPU region overlaps, flairhip.ops.region_overlaps; host matching, flairhip/objects.py): what this run found that the
reference has ("matched"), what only this run has ("new"), what only the reference has ("missing")."""
from __future__ import annotations

import numpy as np

from flairhip import objects
from flair_zonal_detection.inference import raster_to_polygons


def summary_of(sink: dict, compare_iou: float, num_classes=None) -> dict:
    """objects.object_scores of a finished matching (what raster_to_polygons left in its ``_compare_sink``), in the
    JSON form of objects.scores_json, with ``iou_threshold`` and ``compare_classes``; classes 0 .. ``num_classes`` - 1
    (default: up to the greatest class either side holds)"""
    ov = sink["overlaps"]
    if num_classes is None:
        num_classes = 1 + max([-1] + ov.a_class.cpu().tolist() + ov.b_class.cpu().tolist())
    counts, iou_sums = objects.object_counts(ov, sink["matches"], int(num_classes))
    summary = objects.scores_json(objects.object_scores(counts, iou_sums))
    summary.update(iou_threshold=float(compare_iou), compare_classes=sink["classes"])
    return summary


def compare_objects(pred, ref, compare_iou: float = 0.5, compare_classes: str = "same", num_classes=None, **options):
    """``pred`` and ``ref``: class rasters as raster_to_polygons takes them, of one shape, bounds and resolution
    (ValueError otherwise).  ``options``: raster_to_polygons' own keywords (background, min_area, simplification, zone,
    classes, sieve_area, ...), applied to both.

    Returns ``(pred_frame, ref_frame, summary)``.  ``pred_frame`` is raster_to_polygons(pred, compare=ref) -- the
    columns ``match_iou``, ``matched``, ``ref_id``, ``ref_fraction`` -- with a ``status`` of "matched" or "new".
    ``ref_frame`` holds the reference's polygons with ``match_iou``, ``pred_id`` (index of the matched polygon of
    ``pred_frame``, or -1) and a ``status`` of "matched" or "missing".  ``summary`` is objects.object_scores over the
    classes 0 .. ``num_classes`` - 1 (default: up to the greatest class either raster holds) in the JSON form of
    objects.scores_json -- per class and micro-averaged tp / fp / fn, precision, recall, f1, mean_matched_iou, None
    where a denominator is 0 -- with ``iou_threshold`` and ``compare_classes``."""
    for key in ("compare", "confidence"):
        if key in options:
            raise TypeError(f"compare_objects: {key!r} is not an option here")
    sink = {}
    pred_frame = raster_to_polygons(pred, compare=ref, compare_iou=compare_iou, compare_classes=compare_classes,
                                    _compare_sink=sink, **options)
    if "ref" not in sink:
        raise ValueError("compare_objects: ref must be a class raster, not a geometry")
    ref_frame = raster_to_polygons(ref, **options)
    cols = sink["ref"]
    if len(cols["matched"]) != len(ref_frame):
        raise RuntimeError(f"compare_objects: {len(cols['matched'])} reference regions matched, {len(ref_frame)} polygons")
    at = list(ref_frame.columns).index("geometry")
    ref_frame.insert(at, "match_iou", cols["match_iou"])
    ref_frame.insert(at + 1, "pred_id", cols["pred_id"])
    ref_frame.insert(at + 2, "status", np.where(cols["matched"] > 0, "matched", "missing"))
    pred_frame.insert(list(pred_frame.columns).index("geometry"), "status",
                      np.where(pred_frame["matched"].to_numpy() > 0, "matched", "new"))
    return pred_frame, ref_frame, summary_of(sink, compare_iou, num_classes)
