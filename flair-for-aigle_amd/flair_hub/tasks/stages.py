"""Training and prediction stages -- counterpart of the reference's flair_hub/tasks/stages.py (training_stage :19-58,
predict_stage :62-102): train, reload the best checkpoint, predict with the PredictionWriter -- and the calibration
stage that writes the per-model threshold file the reference's interface carries (main.py --threshold_file_path)."""
from __future__ import annotations

import datetime
import logging
import os
import random
from collections import OrderedDict
from pathlib import Path
from typing import Dict, Optional

import numpy as np
import torch

from flair_hub.models.checkpoint import load_checkpoint
from flair_hub.tasks.module_setup import build_segmentation_module, get_input_img_sizes
from flair_hub.tasks.trainers import HipTrainer, _to_device, predict, train

logger = logging.getLogger(__name__)


def seed_everything(seed: int) -> None:
    """python, numpy and torch generators (what pytorch_lightning.seed_everything sets)"""
    random.seed(seed)
    np.random.seed(seed % (1 << 32))
    torch.manual_seed(seed)


def training_stage(config: Dict, data_module, out_dir) -> OrderedDict:
    """-> the state dict of the best checkpoint (by config['saving']['ckpt_monitor'], val_miou by default)"""
    start = datetime.datetime.now()
    seed_everything(int(config["hyperparams"]["seed"]))
    in_img_sizes = get_input_img_sizes(config, data_module, stage="fit")
    seg_module = build_segmentation_module(config, in_img_sizes, stage="train")
    if config["tasks"].get("train_tasks", {}).get("init_weights_only_from_ckpt", False):
        load_checkpoint(config, seg_module, exit_on_fail=True)
    trainer = train(config, data_module, seg_module, os.path.join(str(out_dir), "checkpoints"))
    if trainer.best_model_path is None:  # not rank 0: the file is rank 0's
        state = OrderedDict((k, v.detach().cpu()) for k, v in seg_module.state_dict().items())
    else:
        state = torch.load(trainer.best_model_path, map_location=torch.device("cpu"))["state_dict"]
    took = datetime.datetime.now() - start
    hw = config.get("hardware", {})
    logger.info("[Training finished in %s HH:MM:SS with %s nodes and %s gpus per node]",
                str(datetime.timedelta(seconds=int(took.total_seconds()))), hw.get("num_nodes", 1),
                hw.get("gpus_per_node", 1))
    logger.info("Model path: %s", os.path.join(str(out_dir), "checkpoints"))
    return state


def predict_stage(config: Dict, data_module, out_dir_predict, trained_state_dict: Optional[OrderedDict] = None) -> None:
    """predict the test split (PRED_* rasters, metrics.json) or, with tasks.metrics_only alone, score the rasters of an
    earlier run"""
    out_dir_predict = Path(out_dir_predict)
    tasks = config["tasks"]
    if tasks.get("metrics_only", False) and not tasks.get("predict", False):
        logger.info("[ ] Running in metrics-only mode: loading predictions from disk . . .")
        predict(config, data_module, None, str(out_dir_predict))
        return
    if tasks.get("predict", False):
        in_img_sizes = get_input_img_sizes(config, data_module, stage="predict")
        seg_module = build_segmentation_module(config, in_img_sizes, stage="predict")
        if tasks.get("train") and trained_state_dict is not None:
            seg_module.load_state_dict(trained_state_dict, strict=False)
        else:
            load_checkpoint(config, seg_module)
        logger.info("[ ] Running inference and metrics calculation . . .")
        predict(config, data_module, seg_module, str(out_dir_predict))
    if not tasks.get("predict") and not tasks.get("metrics_only"):
        logger.info("[ ] Neither 'predict' nor 'metrics_only' is enabled. Finishing.")


@torch.no_grad()
def _walk_validation(trainer, seg_module, data_module, per_batch) -> None:
    """the validation split of this rank, without augmentation: per_batch(task, NHWC logits, uint8 targets) per step"""
    from flairhip.nn import LOGIT_PITCH, to_nhwc
    seg_module.to(trainer.device)
    seg_module.trainer = trainer
    data_module.setup("validate")
    trainer._attach_store(seg_module, data_module)
    loader = trainer._shard(data_module.val_dataloader(), shuffle=False, drop_last=False)
    seg_module.eval()
    for batch in loader:
        logits = {}
        _, _, targets = seg_module.step(seg_module._without_aug(_to_device(batch, trainer.device)), training=False,
                                        logits_out=logits)
        for task, z in logits.items():
            nhwc = getattr(z, "_ffa_nhwc", None)
            if nhwc is None:  # a model outside flairhip.nn, as SegmentationTask._update_class_stats lays it out
                nhwc = to_nhwc(z.detach().float().contiguous(), torch.float32, LOGIT_PITCH)
            per_batch(task, nhwc, targets[task])


def calibrate_stage(config: Dict, data_module, out_dir, trained_state_dict: Optional[OrderedDict] = None,
                    seg_module=None) -> str:
    """Calibrated class thresholds of a trained model on its validation split -> the path of best_thresholds.yaml, next
    to the checkpoints (rank 0 writes it).  Runs on the reloaded best checkpoint after training (``trained_state_dict``)
    or alone on paths.ckpt_model_path, as predict_stage does; ``seg_module``: a task that is already built and loaded.

    Pass 1: the score histograms of every task (ops.calib_hist on the step's own logits) and the confusion counts of
    the plain labels, all on the device, summed over the ranks as integers, read once per task at the end;
    flairhip.calibration.best_thresholds picks the thresholds (tasks.calibrate_objective: iou | f1, default iou;
    tasks.calibrate_min_support, default 1).  Pass 2 (tasks.calibrate_verify, default true): the same split through
    ops.predict_thresholded_u8 with those thresholds (fallback label tasks.calibrate_fallback, default 18) and the
    confusion matrix of its labels.  Per class the file then holds iou_argmax (plain labels), iou_one_vs_rest (the
    sweep's value at the chosen threshold) and iou_thresholded (what the label rule really scores)."""
    from flairhip import calibration, ops
    from flairhip.distributed import all_reduce_sum_
    tasks = config.get("tasks", {})
    objective = tasks.get("calibrate_objective", "iou")
    if objective not in calibration.OBJECTIVES:
        raise ValueError(f"tasks.calibrate_objective must be one of {calibration.OBJECTIVES}, got {objective!r}")
    fallback = tasks.get("calibrate_fallback", 18)
    if isinstance(fallback, bool) or not isinstance(fallback, int) or not 0 <= fallback <= 255:
        raise ValueError(f"tasks.calibrate_fallback must be an integer in 0..255, got {fallback!r}")
    if seg_module is None:
        in_img_sizes = get_input_img_sizes(config, data_module, stage="fit")
        seg_module = build_segmentation_module(config, in_img_sizes, stage="train")
        if trained_state_dict is not None:
            seg_module.load_state_dict(trained_state_dict, strict=False)
        else:
            load_checkpoint(config, seg_module)
    hw = config.get("hardware", {})
    trainer = HipTrainer(accelerator=hw.get("accelerator", "gpu"), devices=hw.get("gpus_per_node", 1),
                         strategy=hw.get("strategy", "auto"), num_nodes=hw.get("num_nodes", 1))
    lcfg = config["labels_configs"]
    classes = {t: len(lcfg[t]["value_name"]) for t in config["labels"]}
    dev = trainer.device
    hists = {t: torch.zeros((k, 2, 256), dtype=torch.int64, device=dev) for t, k in classes.items()}
    plain = {t: torch.zeros((k, k), dtype=torch.int64, device=dev) for t, k in classes.items()}

    def pass1(task, nhwc, targets):
        ops.calib_hist(nhwc, targets, classes[task], hist=hists[task])
        ops.eval_stats(nhwc, targets, classes[task], confmat=plain[task], want_pred=False, want_class_nll=False)

    logger.info("[ ] Calibrating class thresholds on the validation split . . .")
    _walk_validation(trainer, seg_module, data_module, pass1)
    all_reduce_sum_(list(hists.values()) + list(plain.values()))
    found = {}
    for task, k in classes.items():
        state = torch.cat([hists[task].reshape(-1), plain[task].reshape(-1)]).cpu().numpy()  # the task's one host read
        hist, cm = state[:k * 512].reshape(k, 2, 256), state[k * 512:].reshape(k, k)
        thr = calibration.best_thresholds(hist, objective, int(tasks.get("calibrate_min_support", 1)))
        found[task] = (hist, cm, thr)
    thresholded = {}
    if tasks.get("calibrate_verify", True):
        thr_dev = {t: torch.from_numpy(found[t][2]).to(dev) for t in classes}
        second = {t: torch.zeros((k, k), dtype=torch.int64, device=dev) for t, k in classes.items()}

        def pass2(task, nhwc, targets):
            labels = ops.predict_thresholded_u8(nhwc, classes[task], "argmax", thr_dev[task], fallback)
            ops.confusion_matrix_update(second[task], labels.reshape(targets.shape), targets)

        _walk_validation(trainer, seg_module, data_module, pass2)
        all_reduce_sum_(list(second.values()))
        thresholded = {t: second[t].cpu().numpy() for t in classes}
    path = os.path.join(str(out_dir), "checkpoints", calibration.FILE_NAME)
    if trainer.rank != 0:
        return path
    os.makedirs(os.path.dirname(path), exist_ok=True)
    if os.path.exists(path):
        os.remove(path)  # write_thresholds adds a task's mapping to the file it finds
    for task, k in classes.items():
        hist, cm, thr = found[task]
        names = lcfg[task]["value_name"]
        names = [names.get(i, f"class_{i}") if hasattr(names, "get") else names[i] for i in range(k)]
        curves = calibration.sweep(hist)
        extra = {"objective": objective, "fallback": fallback, "support": hist[:, 1].sum(axis=1),
                 "ece": calibration.expected_calibration_error(hist),
                 "iou_argmax": calibration.iou_from_confmat(cm),
                 "iou_one_vs_rest": curves["iou"][np.arange(k), thr]}
        if task in thresholded:
            extra["iou_thresholded"] = calibration.iou_from_confmat(thresholded[task], support=cm.sum(axis=1))
        calibration.write_thresholds(path, thr, names, extra, task=task)
        logger.info("%s: thresholds %s", task, thr.tolist())
    logger.info("Threshold file: %s", path)
    return path
