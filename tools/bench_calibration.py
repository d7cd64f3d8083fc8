#!/usr/bin/env python
"""Timing of the calibration kernels at the flagship validation batch, 32 x 512 x 512 pixels, 19 classes at pitch 32,
bf16, on two inputs: saturated logits (the winner +40, the rest -40: a trained model's shape, every score 0 or 255)
and broad logits (N(0, 2^2): scores all over 1..254).

  1. ffa_calib_hist against ffa_eval_stats (all outputs) on the same tensor in the same process -- the same reads --
     and against the byte floor: logits + targets read once (545 MB) at the float4-copy rate of DESIGN.md section 5b.
  2. ffa_predict_thresholded_u8 modes 0 / 2 against ffa_predict_u8 modes 0 / 2 on the same tensor and margin crop
     (40 of 512): the same bytes, plus K byte compares per pixel.

HIP events around back-to-back launches on the stream; per kernel the median over --reps windows of --iters launches
after a warm-up, the kernels of a comparison alternating window by window.  One JSON line.

  python tools/bench_calibration.py [--iters 10] [--reps 9]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

import torch

from flairhip import ops

COPY_TBS = 6.29  # the measured float4-copy rate
B, H, K, CP, MARGIN = 32, 512, 19, 32, 40


def median_us(fns, iters, reps, warm_s=0.3):
    """{name: median microseconds per launch}; the windows of the functions alternate"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < warm_s:
        for fn in fns.values():
            for _ in range(iters):
                fn()
        torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            torch.cuda.synchronize()
            out[name].append(s.elapsed_time(e) / iters * 1e3)
    return {name: statistics.median(v) for name, v in out.items()}


def inputs(kind, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    tgt = torch.randint(0, K, (B, H, H), device=dev, dtype=torch.uint8, generator=g)
    if kind == "saturated":
        z = torch.full((B, H, H, CP), -40.0, device=dev)
        # the model is right on 80 % of the pixels
        winner = torch.where(torch.rand((B, H, H), device=dev, generator=g) < 0.8, tgt.long(),
                             torch.randint(0, K, (B, H, H), device=dev, generator=g))
        z.scatter_(3, winner[..., None], 40.0)
    else:
        z = 2.0 * torch.randn((B, H, H, CP), device=dev, generator=g)
    return z.to(torch.bfloat16), tgt


def hist_fns(z, tgt):
    hist = torch.zeros((K, 2, 256), dtype=torch.int64, device=z.device)
    cm = torch.zeros((K, K), dtype=torch.int64, device=z.device)
    return {"calib_hist_us": lambda: ops.calib_hist(z, tgt, K, hist=hist),
            "eval_stats_us": lambda: ops.eval_stats(z, tgt, K, confmat=cm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    keep = H - 2 * MARGIN
    crop = (MARGIN, MARGIN, keep, keep)
    thr = torch.tensor([160 if k % 2 == 0 else 40 for k in range(K)], dtype=torch.uint8, device=dev)
    res = {"hist_bytes": B * H * H * (CP * 2 + 1)}
    res["hist_floor_us"] = res["hist_bytes"] / (COPY_TBS * 1e6)
    for kind in ("saturated", "broad"):
        z, tgt = inputs(kind, dev)
        r = median_us(hist_fns(z, tgt), args.iters, args.reps)
        r["calib_hist_over_eval_stats"] = r["calib_hist_us"] / r["eval_stats_us"]
        r["calib_hist_over_floor"] = r["calib_hist_us"] / res["hist_floor_us"]
        fns = {}
        for mode in ("argmax", "argmax_conf"):
            fns[f"predict_u8_{mode}_us"] = lambda mode=mode: ops.predict_u8(z, K, mode, crop=crop)
            fns[f"predict_thresholded_u8_{mode}_us"] = \
                lambda mode=mode: ops.predict_thresholded_u8(z, K, mode, thr, 18, crop=crop)
        r.update(median_us(fns, args.iters, args.reps))
        for mode in ("argmax", "argmax_conf"):
            r[f"thresholded_over_plain_{mode}"] = r[f"predict_thresholded_u8_{mode}_us"] / r[f"predict_u8_{mode}_us"]
        res[kind] = {k: round(v, 3) for k, v in r.items()}
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
