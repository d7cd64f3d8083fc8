"""Training and prediction stages -- counterpart of the reference's flair_hub/tasks/stages.py (training_stage :19-58,
predict_stage :62-102): train, reload the best checkpoint, predict with the PredictionWriter."""
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
from flair_hub.tasks.trainers import predict, train

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
