"""``python -m flair_hub.main --config DIR_OR_YAML`` -- counterpart of the reference's flair_hub/main.py: read the
configuration, list the dataset, train, reload the best checkpoint and predict.  TensorBoard, progress bars and the
message banner of the reference are not part of this build."""
from __future__ import annotations

import argparse
import logging
import os
import sys
from pathlib import Path

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

from flair_hub.data.utils_data.paths import get_datasets  # noqa: E402
from flair_hub.tasks.module_setup import build_data_module  # noqa: E402
from flair_hub.tasks.stages import calibrate_stage, predict_stage, training_stage  # noqa: E402
from flair_hub.utils.config_io import setup_environment  # noqa: E402

logger = logging.getLogger(__name__)


def main(argv=None) -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--config", help="Path to the .yaml config file or to a directory of them", required=True)
    args = parser.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    config, out_dir = setup_environment(args)
    dict_train, dict_val, dict_test = get_datasets(config)
    dm = build_data_module(config, dict_train=dict_train, dict_val=dict_val, dict_test=dict_test)
    state = None
    if config["tasks"]["train"]:
        state = training_stage(config, dm, out_dir)
    if config["tasks"].get("calibrate", False):  # per-class thresholds from the validation split: best_thresholds.yaml
        calibrate_stage(config, dm, out_dir, state)
    if config["tasks"].get("predict") or config["tasks"].get("metrics_only"):
        out_dir_predict = Path(out_dir, "results_" + config["paths"]["out_model_name"])
        out_dir_predict.mkdir(parents=True, exist_ok=True)
        predict_stage(config, dm, out_dir_predict, state)
    else:
        logger.info("[WARNING] Neither prediction nor metrics_only was enabled. Finishing.")


if __name__ == "__main__":
    main()
