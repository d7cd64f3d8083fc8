"""metrics.json and confmat_<mode>.npy of one task -- counterpart of the reference's flair_hub/writer/metrics_utils.py
(same keys in the same order, same numbers).  numpy only."""
from __future__ import annotations

import json
import logging
import os
from typing import Any, Dict, List

import numpy as np

from flair_hub.writer.metrics_core import class_fscore, class_IoU, class_precision, class_recall, overall_accuracy

logger = logging.getLogger(__name__)


def class_weights_of(config: Dict[str, Any], task: str):
    """(default weight per class, {active modality: weight per class}) from labels_configs[task].value_weights:
    `default`, overridden per class by `default_exceptions`, and per modality by `per_modality_exceptions`"""
    label_config = config["labels_configs"][task]
    num_classes = len(label_config["value_name"])
    vw = label_config.get("value_weights", {}) or {}
    default: List[Any] = [vw.get("default", 1)] * num_classes
    for i, w in (vw.get("default_exceptions") or {}).items():
        default[i] = w
    active = [m for m, on in config["modalities"]["inputs"].items() if on]
    per_mod = vw.get("per_modality_exceptions") or {}
    by_modality = {}
    for m in active:
        by_modality[m] = list(default)
        for i, w in (per_mod.get(m) or {}).items():
            by_modality[m][i] = w
    return default, by_modality


def compute_metrics(confmat: np.ndarray, config: Dict[str, Any], task: str) -> Dict[str, Any]:
    """the contents of metrics.json: classes whose default weight is 0 leave rows and columns, then per-class IoU /
    F-score / precision / recall in percent (NaN -> 0), their means and the overall accuracy"""
    names = config["labels_configs"][task]["value_name"]
    default, by_modality = class_weights_of(config, task)
    used = [i for i, w in enumerate(default) if w != 0]
    cm = np.asarray(confmat)[np.ix_(used, used)]
    ious, miou = class_IoU(cm, len(used))
    precision, avg_precision = class_precision(cm)
    recall, avg_recall = class_recall(cm)
    fscore, avg_fscore = class_fscore(precision, recall)
    return {
        "Avg_metrics_name": ["mIoU", "Overall Accuracy", "F-score", "Precision", "Recall"],
        "Avg_metrics": [float(miou), float(overall_accuracy(cm)), float(avg_fscore), float(avg_precision),
                        float(avg_recall)],
        "classes": [names[i] for i in used],
        "per_class_iou": [float(v) for v in ious],
        "per_class_fscore": [float(v) for v in fscore],
        "per_class_precision": [float(v) for v in precision],
        "per_class_recall": [float(v) for v in recall],
        "per_class_default_weight": [default[i] for i in used],
        "per_class_modality_weights": {m: [w[i] for i in used] for m, w in by_modality.items()},
    }


def compute_and_save_object_metrics(counts: np.ndarray, iou_sums: np.ndarray, config: Dict[str, Any], output_dir: str,
                                    task: str, iou_threshold: float, min_pixels: int, classes=None) -> Dict[str, Any]:
    """<output_dir>/metrics_<paths.out_model_name>/<task>/object_metrics.json, next to metrics.json: per class (by
    value_name) tp / fp / fn, precision, recall, f1 and mean_matched_iou of the predicted objects against the reference
    objects (flairhip/objects.py; ``counts`` int64 [K, 3], ``iou_sums`` float64 [K]), their micro average, the IoU
    threshold, min_pixels and the class filter.  A value whose denominator is 0 is null."""
    from flairhip import objects
    names = config["labels_configs"][task]["value_name"]
    names = [str(names[i]) for i in range(len(names))]
    out = objects.scores_json(objects.object_scores(counts, iou_sums), names)
    out.update(iou_threshold=float(iou_threshold), min_pixels=int(min_pixels),
               class_filter=None if classes is None else [int(c) for c in classes])
    folder = os.path.join(str(output_dir), f"metrics_{config['paths']['out_model_name']}", task)
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "object_metrics.json"), "w") as f:
        json.dump(out, f, indent=2)
    micro = out["micro"]
    logger.info("Task: %s - objects at IoU >= %.2f: %d found, %d invented, %d missed", task, float(iou_threshold),
                micro["tp"], micro["fp"], micro["fn"])
    return out


def compute_and_save_metrics(confmat: np.ndarray, config: Dict[str, Any], output_dir: str, task: str,
                             mode: str = "predict") -> None:
    """<output_dir>/metrics_<paths.out_model_name>/<task>/metrics.json and confmat_<mode>.npy (the full matrix), and the
    same table in the log"""
    metrics = compute_metrics(confmat, config, task)
    folder = os.path.join(str(output_dir), f"metrics_{config['paths']['out_model_name']}", task)
    os.makedirs(folder, exist_ok=True)
    np.save(os.path.join(folder, f"confmat_{mode}.npy"), confmat)
    with open(os.path.join(folder, "metrics.json"), "w") as f:
        json.dump(metrics, f, indent=2)

    mods = list(metrics["per_class_modality_weights"])
    rule = "-" * (90 + 15 * len(mods))
    logger.info("Task: %s - global metrics", task)
    logger.info(rule)
    for name, value in zip(metrics["Avg_metrics_name"], metrics["Avg_metrics"]):
        logger.info("%-20s %.4f", name, value)
    logger.info(rule)
    logger.info("%-6s %-25s %-10s %-10s %-10s %-10s %-15s%s", "Idx", "Class", "IoU", "F-score", "Precision", "Recall",
                "w.TASK", "".join(f" {'w.' + m:<15}" for m in mods))
    for i, name in enumerate(metrics["classes"]):
        logger.info("%-6d %-25s %-10.4f %-10.4f %-10.4f %-10.4f %-15s%s", i, name, metrics["per_class_iou"][i],
                    metrics["per_class_fscore"][i], metrics["per_class_precision"][i], metrics["per_class_recall"][i],
                    metrics["per_class_default_weight"][i],
                    "".join(f" {metrics['per_class_modality_weights'][m][i]:<15}" for m in mods))
    default, _ = class_weights_of(config, task)
    unused = [i for i, w in enumerate(default) if w == 0]
    if unused:
        names = config["labels_configs"][task]["value_name"]
        logger.info("0-weighted classes of the task: %s", ", ".join(f"{i} {names[i]}" for i in unused))
