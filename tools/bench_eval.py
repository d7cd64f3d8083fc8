#!/usr/bin/env python
"""Timing of the evaluation kernel (ffa_eval_stats) at the flagship validation batch, 32 x 512 x 512 pixels, 19 classes
at pitch 32, bf16:

  1. ops.eval_stats with all outputs (labels, confusion matrix, per-class loss sums and counts);
  2. the launches it replaces in a validation batch: ops.softmax_ce without gradient with labels, plus two
     ops.confusion_matrix_update (val_metrics and val_iou) -- the per-class loss has no counterpart there;
  3. the HBM floor: logits + targets read once, labels written once;
  and a validation epoch of the resnet34-unet (4 batches of 8 tiles) with and without the per-class logging.

HIP events around back-to-back launches on the stream, the best of several batches after a warm-up; random inputs.

  python tools/bench_eval.py [--iters 20] [--reps 7] [--no-epoch]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

import torch

from flairhip import ops

HBM_TBS = 8.0  # MI355X data sheet


def best_us(fn, iters, reps, warm_s=0.4):
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < warm_s:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / iters * 1e3)
    return min(out)


def bench_kernel(args):
    dev = torch.device("cuda:0")
    B, H, K, cp = 32, 512, 19, 32
    logits = (4 * torch.randn(B, H, H, cp, device=dev)).to(torch.bfloat16)
    tgt = torch.randint(0, K, (B, H, H), device=dev, dtype=torch.uint8)
    cw = torch.tensor([1.0] * 15 + [0.0] * 4, device=dev)
    cm, cm2 = (torch.zeros(K, K, dtype=torch.int64, device=dev) for _ in range(2))

    def replaced():
        _, _, _, pred = ops.softmax_ce(logits, tgt, cw, K, want_pred=True)
        ops.confusion_matrix_update(cm, pred, tgt)
        ops.confusion_matrix_update(cm2, pred, tgt)

    nbytes = logits.numel() * 2 + 2 * tgt.numel()
    res = {
        "eval_stats_us": best_us(lambda: ops.eval_stats(logits, tgt, K, confmat=cm), args.iters, args.reps),
        "eval_stats_labels_only_us": best_us(lambda: ops.eval_stats(logits, tgt, K, want_class_nll=False), args.iters,
                                             args.reps),
        "replaced_launches_us": best_us(replaced, args.iters, args.reps),
        "softmax_ce_pred_us": best_us(lambda: ops.softmax_ce(logits, tgt, cw, K, want_pred=True), args.iters, args.reps),
        "bytes": nbytes,
        "hbm_floor_us": nbytes / (HBM_TBS * 1e6),
    }
    res["eval_stats_TBs"] = nbytes / res["eval_stats_us"] / 1e6
    return res


def bench_epoch(args):
    from flairhip.configs import unet_resnet34_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from flair_hub.tasks.trainers import HipTrainer
    task_name, mod = "AERIAL_LABEL-COSIA", "AERIAL_RGBI"
    cfg = unet_resnet34_config(in_channels=5, precision="bf16", batch_size=8)
    torch.manual_seed(0)
    task = build_segmentation_module(cfg, {mod: 512}, "train").cuda()
    g = torch.Generator().manual_seed(0)
    batches = [{mod: torch.randn(8, 5, 512, 512, generator=g).cuda(),
                task_name: torch.randint(0, 19, (8, 512, 512), generator=g).to(torch.uint8).cuda()} for _ in range(4)]
    trainer = HipTrainer()

    def epoch_ms():
        best = None
        for i in range(4):  # the first is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.validate(task, dataloaders=batches)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                best = dt if best is None else min(best, dt)
        return best

    with_logging = epoch_ms()
    task._update_class_stats = lambda key, logits, preds, targets: task.val_iou[key].update(preds, targets)
    task._log_per_class = lambda key: None
    return {"val_epoch_ms": with_logging, "val_epoch_without_per_class_ms": epoch_ms(), "val_epoch_tiles": 32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-epoch", action="store_true")
    args = ap.parse_args()
    res = bench_kernel(args)
    if not args.no_epoch:
        res.update(bench_epoch(args))
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
