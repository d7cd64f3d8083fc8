"""Test stage -- counterpart of the reference's flair_hub/writer/prediction_writer.py (a Lightning BasePredictionWriter
callback; here HipTrainer.predict calls the same two hooks).

Per batch and task the reference copies the prediction to the host, opens the label file of sample 0 with rasterio,
writes PRED_<label file name> and adds an sklearn confusion matrix of the two host arrays.  Here the label files of
EVERY sample of the batch are read (flair_zonal_detection.geotiff), go to the device in one copy, and one ops.eval_stats
pass over the logits that predict_step left on the module gives the labels and adds the counts to a device matrix: no
second forward, no host arithmetic.  The labels are copied back only when files are to be written, and a single writer
thread encodes the files of batch k while the device works on batch k + 1.
"""
from __future__ import annotations

import csv
import logging
import os
from concurrent.futures import ThreadPoolExecutor
from typing import Any, Dict, List

import numpy as np
import torch
import torch.distributed as dist

from flairhip import ops
from flairhip.distributed import all_reduce_sum_
from flairhip.nn import LOGIT_PITCH, to_nhwc
from flair_hub.writer.metrics_utils import compute_and_save_metrics, compute_and_save_object_metrics
from flair_zonal_detection.geotiff import GeoTiffRaster, GeoTiffWriter

logger = logging.getLogger(__name__)


def read_label_band(path: str, channel: int) -> np.ndarray:
    """band ``channel`` (1-based) of a label raster as uint8 [H, W]; a value outside 0..255 becomes 255, which no task
    has as a class, so the pixel counts nowhere"""
    with GeoTiffRaster(path) as src:
        band = src.read(channel)
    if band.dtype == np.uint8:
        return band
    return np.where((band < 0) | (band > 255), 255, band).astype(np.uint8)


def object_metrics_options(config: Dict[str, Any]):
    """The key tasks.object_metrics: absent or false = off (None); else {iou_threshold: 0.5, min_pixels: 1,
    classes: null} (true or an empty mapping: those defaults).  A bad value raises ValueError."""
    opt = (config.get("tasks") or {}).get("object_metrics")
    if opt is None or opt is False:
        return None
    if opt is True:
        opt = {}
    if not isinstance(opt, dict) or set(opt) - {"iou_threshold", "min_pixels", "classes"}:
        raise ValueError(f"tasks.object_metrics must be false or a mapping of iou_threshold, min_pixels and classes, "
                         f"got {opt!r}")
    thr, minp, classes = opt.get("iou_threshold", 0.5), opt.get("min_pixels", 1), opt.get("classes")
    if isinstance(thr, bool) or not isinstance(thr, (int, float)) or not 0.0 < float(thr) <= 1.0:
        raise ValueError(f"tasks.object_metrics.iou_threshold must be a number in (0, 1], got {thr!r}")
    if isinstance(minp, bool) or not isinstance(minp, int) or minp < 1:
        raise ValueError(f"tasks.object_metrics.min_pixels must be an integer >= 1, got {minp!r}")
    if classes is not None:
        classes = sorted({int(c) for c in classes})
        if not all(0 <= c < 255 for c in classes):
            raise ValueError(f"tasks.object_metrics.classes must be class ids below 255, got {classes}")
    return {"iou_threshold": float(thr), "min_pixels": int(minp), "classes": classes}


def _write_prediction(path: str, labels: np.ndarray, like: str, georeferenced: bool) -> None:
    """single-band uint8 LZW TIFF; ``georeferenced``: on the grid of the label file ``like`` (origin, resolution, CRS)"""
    h, w = labels.shape
    if georeferenced:
        with GeoTiffRaster(like) as ref:
            out = GeoTiffWriter.like(path, ref, 1, width=w, height=h)
    else:
        out = GeoTiffWriter(path, w, h, 1, 0.0, float(h), 1.0, crs=None, georeferenced=False)
    out.data[0] = labels
    out.close()


class PredictionWriter:
    """write_on_batch_end / on_predict_epoch_end / load_predictions_and_compute_metrics of the reference's callback."""

    def __init__(self, config: Dict[str, Any], output_dir: str, write_interval: str = "batch") -> None:
        self.config = config
        self.output_dir = str(output_dir)
        self.write_interval = write_interval
        self.accumulated_confmats: Dict[str, Any] = {task: None for task in config["labels"]}
        # object metrics (tasks.object_metrics, off by default): per task int64 [K, 3] TP / FP / FN, float64 [K] IoU sums
        self.object_options = object_metrics_options(config)
        self.object_counts: Dict[str, Any] = {}
        self.object_iou_sums: Dict[str, Any] = {}
        self._io = None       # one thread: files of batch k are encoded while the device runs batch k + 1
        self._pending: List[Any] = []

    # ---- helpers -----------------------------------------------------------------------------------------------------
    def _classes(self, task: str) -> int:
        return len(self.config["labels_configs"][task]["value_name"])

    def _channel(self, task: str) -> int:
        return int(self.config["labels_configs"][task].get("label_channel_nomenclature", 1))

    def _prediction_dir(self, task: str) -> str:
        return os.path.join(self.output_dir, f"predictions_{self.config['paths']['out_model_name']}", task)

    def _drain(self) -> None:
        pending, self._pending = self._pending, []
        for job in pending:
            job.result()  # a failed write surfaces here

    # ---- object metrics --------------------------------------------------------------------------------------------
    def _object_state(self, task: str):
        if task not in self.object_counts:
            k = self._classes(task)
            self.object_counts[task] = np.zeros((k, 3), np.int64)
            self.object_iou_sums[task] = np.zeros(k, np.float64)
        return self.object_counts[task], self.object_iou_sums[task]

    def _count_objects(self, task: str, pred: torch.Tensor, target: torch.Tensor) -> None:
        """Add the objects of device uint8 [B, H, W] predictions (A) against targets (B) to the task's counts.  On
        copies: a target >= K becomes the background 255 -- with the optional class filter in the same
        ffa_zone_clip_u8 pass -- and the prediction takes 255 where the target was >= K, so ignored ground truth
        creates no false positive; with a class filter the prediction is filtered like the target."""
        from flairhip import objects
        opt, k = self.object_options, self._classes(task)
        keep = [c for c in (range(k) if opt["classes"] is None else opt["classes"]) if c < k]
        tgt = target.contiguous().clone()
        prd = pred.contiguous().clone()
        prd.masked_fill_(tgt >= k, 255)
        ops.zone_clip_(tgt, None, keep_classes=keep, fill=255)
        if opt["classes"] is not None:
            ops.zone_clip_(prd, None, keep_classes=keep, fill=255)
        counts, iou_sums = self._object_state(task)
        for ov in ops.region_overlaps_batch(prd, tgt, 255, 255, opt["min_pixels"], opt["min_pixels"]):
            c, s = objects.object_counts(ov, objects.match_objects(ov, opt["iou_threshold"], "same"), k)
            counts += c
            iou_sums += s

    def _save_object_metrics(self, task: str, counts, iou_sums) -> None:
        opt = self.object_options
        compute_and_save_object_metrics(counts, iou_sums, self.config, self.output_dir, task, opt["iou_threshold"],
                                        opt["min_pixels"], opt["classes"])

    # ---- hooks -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def write_on_batch_end(self, trainer, module, prediction, batch_indices, batch, batch_idx, dataloader_idx) -> None:
        tasks = list(self.config["labels"])
        device = module.device
        logits = getattr(module, "_last_logits", None)
        if logits is None:
            raise RuntimeError("PredictionWriter: the module's predict_step left no logits (_last_logits)")
        # every label band of the batch, all tasks: one pinned buffer, one copy to the device
        paths = {task: [str(p) for p in batch[f"ID_{task}"]] for task in tasks}
        bands = {task: [read_label_band(p, self._channel(task)) for p in paths[task]] for task in tasks}
        total = sum(b.size for bs in bands.values() for b in bs)
        host = torch.empty(total, dtype=torch.uint8).pin_memory()
        view, pos, spans = host.numpy(), 0, {}
        for task in tasks:
            spans[task] = pos
            for b in bands[task]:
                view[pos:pos + b.size] = b.reshape(-1)
                pos += b.size
        targets = host.to(device, non_blocking=True)

        write = bool(self.config["tasks"].get("write_files", False))
        geo = bool(self.config["tasks"].get("georeferencing_output", False))
        for task in tasks:
            k = self._classes(task)
            lg = logits[task]
            nhwc = getattr(lg, "_ffa_nhwc", None)
            if nhwc is None:
                nhwc = to_nhwc(lg.detach().float().contiguous(), torch.float32, LOGIT_PITCH)
            B, H, W = nhwc.shape[:3]
            if len(bands[task]) != B or any(b.shape != (H, W) for b in bands[task]):
                raise ValueError(f"PredictionWriter: {task}: the label files of the batch are "
                                 f"{[b.shape for b in bands[task]]}, the logits {(B, H, W)}")
            if self.accumulated_confmats[task] is None:
                self.accumulated_confmats[task] = torch.zeros(k, k, dtype=torch.int64, device=device)
            tgt = targets[spans[task]:spans[task] + B * H * W].view(B, H, W)
            labels, _, _ = ops.eval_stats(nhwc, tgt, k, confmat=self.accumulated_confmats[task], want_pred=True,
                                          want_class_nll=False)
            if self.object_options is not None:
                self._count_objects(task, labels.view(B, H, W), tgt)
            if not write:
                continue
            out_dir = self._prediction_dir(task)
            os.makedirs(out_dir, exist_ok=True)
            staged = torch.empty(labels.shape, dtype=torch.uint8).pin_memory()
            staged.copy_(labels, non_blocking=True)
            done = torch.cuda.Event()
            done.record()
            if self._io is None:
                self._io = ThreadPoolExecutor(1, thread_name_prefix="prediction-writer")
            self._pending.append(self._io.submit(self._write_batch, staged, done, paths[task], out_dir, geo))
        if len(self._pending) > 8:  # bound what is in flight: the oldest jobs have long finished
            old, self._pending = self._pending[:-4], self._pending[-4:]
            for job in old:
                job.result()

    @staticmethod
    def _write_batch(staged: torch.Tensor, done, label_paths: List[str], out_dir: str, geo: bool) -> None:
        done.synchronize()  # this thread waits for the copy, the stream goes on
        arr = staged.numpy()
        for j, label_path in enumerate(label_paths):
            _write_prediction(os.path.join(out_dir, f"PRED_{os.path.basename(label_path)}"), arr[j], label_path, geo)

    def on_predict_epoch_end(self, trainer, module) -> None:
        self._drain()
        device = module.device
        mats = []
        for task in self.config["labels"]:
            if self.accumulated_confmats[task] is None:  # a rank without batches still takes part in the sum
                k = self._classes(task)
                self.accumulated_confmats[task] = torch.zeros(k, k, dtype=torch.int64, device=device)
            mats.append(self.accumulated_confmats[task])
        objs = []
        if self.object_options is not None:  # one more tensor per task: float64 [K, 4] of TP, FP, FN, IoU sum
            for task in self.config["labels"]:
                counts, iou_sums = self._object_state(task)
                objs.append(torch.from_numpy(np.concatenate([counts.astype(np.float64), iou_sums[:, None]], 1)).to(device))
        all_reduce_sum_(mats + objs)
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        if rank == 0:
            for task, mat in zip(self.config["labels"], mats):
                compute_and_save_metrics(mat.cpu().numpy(), self.config, self.output_dir, task, mode="predict")
            for task, obj in zip(self.config["labels"], objs):
                obj = obj.cpu().numpy()
                self._save_object_metrics(task, np.rint(obj[:, :3]).astype(np.int64), obj[:, 3])
        if self._io is not None:
            self._io.shutdown(wait=True)
            self._io = None

    def load_predictions_and_compute_metrics(self) -> None:
        """The reference's metrics_only path: pair PRED_<name> under predictions_<model>/<task>/ with every label file of
        paths.test_csv (column <task>), count on the device, write the metrics with mode="metrics_only"."""
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        if rank != 0:
            return
        device = torch.device("cuda", torch.cuda.current_device())
        found_any = False
        for task in self.config["labels"]:
            k = self._classes(task)
            with open(self.config["paths"]["test_csv"], newline="") as f:
                gt_paths = [row[task] for row in csv.DictReader(f)]
            confmat = torch.zeros(k, k, dtype=torch.int64, device=device)
            self.object_counts.pop(task, None)  # this path counts from the files alone
            pred_dir = self._prediction_dir(task)
            missing, valid = [], 0
            for gt_path in gt_paths:
                pred_path = os.path.join(pred_dir, f"PRED_{os.path.basename(gt_path)}")
                if not os.path.exists(pred_path):
                    missing.append(pred_path)
                    continue
                gt = read_label_band(gt_path, self._channel(task))
                pred = read_label_band(pred_path, 1)
                if gt.shape != pred.shape:
                    logger.info("[ERROR] %s: label %s, prediction %s", os.path.basename(gt_path), gt.shape, pred.shape)
                    continue
                both = torch.from_numpy(np.stack([pred, gt])).to(device)
                ops.confusion_matrix_update(confmat, both[0], both[1])
                if self.object_options is not None:
                    self._count_objects(task, both[0:1], both[1:2])
                valid += 1
            for p in missing:
                logger.info("missing prediction: %s", p)
            logger.info("%s: %d of %d label files have a prediction", task, valid, len(gt_paths))
            if valid:
                self.accumulated_confmats[task] = confmat
                compute_and_save_metrics(confmat.cpu().numpy(), self.config, self.output_dir, task, mode="metrics_only")
                if self.object_options is not None:
                    self._save_object_metrics(task, *self._object_state(task))
                found_any = True
        if not found_any:
            logger.info("[ERROR] no predictions found at all: metrics are not calculated")
