#!/usr/bin/env python
"""PCIe-inclusive training throughput: HipTrainer.fit over HOST-resident batches (pinned), i.e. what a DataLoader hands
over, for the reference's batch schema (f32 imagery + f32 one-hot labels, 25 MB per tile) and for the compact schema
the product also accepts (uint8 imagery + '<MOD>_NORM' + uint8 class indices, 1.6 MB per tile).  bench.py's `value`
has its inputs resident in HBM; this is the number next to it.

  python tools/bench_trainer_pcie.py [--batch 32] [--steps 30] [--schemas compact,reference] [--repeat 1] [--augment]
  python tools/bench_trainer_pcie.py --dataset DIR --cache none|device [--batch 32] [--steps 30] [--repeat 1]

--dataset DIR (written by tools/make_patch_dataset.py): the same step fed by FlairDataModule from GeoTIFF patches on
disk, gathered from the device-resident sample store (--cache device) or decoded and streamed per batch (--cache none).
A dataset written with --sentinel2 adds the U-TAE branch; DIR/config says whether its series are averaged per period
(one T: the captured step replays) and whether hardware.sample_cache_series lets them into the store.

--augment: the same run with modalities.pre_processings.use_augmentation on (per-sample flips / rotations drawn by the
trainer, applied inside the layout and label kernels).  --schemas picks the schemas to run and --repeat N runs each N
times in this process (a fresh model per run): the spread of the number, which a comparison against another commit or
against --augment has to be read next to.  One JSON line per run, then the box's pinned H2D rate.  Every line says how many
of the run's steps were graph replays and how many ran eagerly (HipTrainer.graph_replays / eager_steps); --no-graph runs
the eager trainer for comparison.
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

MOD, TASK = "AERIAL_RGBI", "AERIAL_LABEL-COSIA"


class Cycle:
    """len()-able loader over a few pinned host batches, reused round-robin"""

    def __init__(self, batches, n):
        self.batches, self.n = batches, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for i in range(self.n):
            yield self.batches[i % len(self.batches)]


def run(schema: str, B: int, steps: int, warm: int = 10, augment: bool = False, hip_graph: bool = True):
    from flairhip.configs import unet_resnet34_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from flair_hub.tasks.trainers import HipTrainer
    cfg = unet_resnet34_config(in_channels=5, precision="bf16", batch_size=B, total_steps=steps + warm + 8)
    cfg["modalities"]["pre_processings"]["use_augmentation"] = bool(augment)
    torch.manual_seed(2025)
    task = build_segmentation_module(cfg, {MOD: 512}, "train")
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(3):
        t = torch.randint(0, 19, (B, 512, 512), generator=g)
        if schema == "reference":
            b = {MOD: torch.randn(B, 5, 512, 512, generator=g),
                 TASK: torch.nn.functional.one_hot(t, 19).permute(0, 3, 1, 2).float().contiguous()}
        else:
            b = {MOD: torch.randint(0, 255, (B, 5, 512, 512), generator=g, dtype=torch.uint8),
                 MOD + "_NORM": torch.tensor([[110.0] * 5, [50.0] * 5]), TASK: t.to(torch.uint8)}
        batches.append({k: v.pin_memory() for k, v in b.items()})
    mb = sum(v.numel() * v.element_size() for v in batches[0].values()) / 2 ** 20
    marks = {}
    orig = task.on_train_batch_end

    def hook(loss, batch, i):
        if task.global_step in (warm, warm + steps):
            torch.cuda.synchronize()
            marks[task.global_step] = time.perf_counter()
        return orig(loss, batch, i)

    task.on_train_batch_end = hook
    tr = HipTrainer(max_epochs=1, max_steps=warm + steps, hip_graph=hip_graph)
    tr.fit(task, train_dataloaders=Cycle(batches, warm + steps + 1))
    dt = marks[warm + steps] - marks[warm]
    return {"schema": schema, "augment": bool(augment), "graph_replays": tr.graph_replays, "eager_steps": tr.eager_steps,
            "host_MB_per_batch": round(mb, 1), "ms_per_step": round(dt / steps * 1e3, 3),
            "tiles_per_s": round(B * steps / dt, 1), "h2d_GBps_needed": round(mb / 1024 / (dt / steps), 1)}


def run_dataset(root: str, cache: str, B: int, steps: int, warm: int = 10, hip_graph: bool = True):
    """the training step fed by FlairDataModule from the on-disk dataset tools/make_patch_dataset.py wrote under
    ``root``: cache='device' gathers every batch from the device-resident sample store, cache='none' decodes the
    GeoTIFF patches per batch and streams the raw samples.  Aerial, plus the Sentinel-2 branch when the dataset was
    written with one (``--sentinel2``; DIR/config then says whether the series are averaged per period and whether
    hardware.sample_cache_series lets them into the store); augmentation on, hipGraph step where the batches share
    one T."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_patch_dataset import make_config
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    from flair_hub.tasks.module_setup import build_segmentation_module, get_input_img_sizes
    from flair_hub.tasks.trainers import HipTrainer
    csvs = {k: os.path.join(root, f"{k}.csv") for k in ("train", "val", "test")}
    written = {}
    if os.path.isdir(os.path.join(root, "config")):
        from flair_hub.utils.config_io import read_config
        written = read_config(os.path.join(root, "config"))
    s2 = bool(written.get("modalities", {}).get("inputs", {}).get("SENTINEL2_TS", False))
    average = written.get("modalities", {}).get("pre_processings", {}).get("temporal_average_sentinel2") or None
    series_cache = bool(written.get("hardware", {}).get("sample_cache_series", False))
    cfg = make_config(root, csvs, cache, B, 1, "bf16", dem=False, sentinel2=s2, s2_average=average,
                      cache_series=series_cache)
    cfg["tasks"]["predict"] = False
    tr_paths, va_paths, _ = get_datasets(cfg)
    dm = FlairDataModule(cfg, tr_paths, va_paths, None, num_workers=16, batch_size=B, drop_last=True,
                         use_augmentations=True, cache=cache, device_prepare=True, series_cache=series_cache)
    t0 = time.perf_counter()
    sizes = get_input_img_sizes(cfg, dm, "fit")
    fill_s = time.perf_counter() - t0
    torch.manual_seed(2025)
    task = build_segmentation_module(cfg, sizes, "train")
    marks = {}
    orig = task.on_train_batch_end

    def hook(loss, batch, i):
        if task.global_step in (warm, warm + steps):
            torch.cuda.synchronize()
            marks[task.global_step] = time.perf_counter()
        return orig(loss, batch, i)

    task.on_train_batch_end = hook
    if dm.store is not None:
        task.attach_store(dm.store)  # fit() is handed the loader, not the data module
    per_epoch = max(len(dm.train_dataloader()), 1)
    tr = HipTrainer(max_epochs=-(-(warm + steps) // per_epoch), max_steps=warm + steps, hip_graph=hip_graph)
    tr.fit(task, train_dataloaders=dm.train_dataloader())
    dt = marks[warm + steps] - marks[warm]
    return {"dataset": root, "cache": cache, "resident": dm.store is not None, "sentinel2": s2,
            "s2_average": average, "series_resident": dm.store is not None and bool(dm.store.series),
            "store_MB": round(dm.store.bytes / 2 ** 20, 1) if dm.store is not None else 0, "setup_s": round(fill_s, 2),
            "graph_replays": tr.graph_replays, "eager_steps": tr.eager_steps,
            "ms_per_step": round(dt / steps * 1e3, 3), "tiles_per_s": round(B * steps / dt, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default=None, help="a directory written by tools/make_patch_dataset.py: train from it")
    ap.add_argument("--cache", choices=("none", "device"), default="device", help="with --dataset: the sample cache")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--schemas", default="compact,reference")
    ap.add_argument("--augment", action="store_true", help="use_augmentation on")
    ap.add_argument("--repeat", type=int, default=1, help="runs per schema (the spread of the number)")
    ap.add_argument("--no-graph", action="store_true", help="HipTrainer(hip_graph=False): every step eager")
    args = ap.parse_args()
    if args.dataset:
        for _ in range(args.repeat):
            print(json.dumps(run_dataset(os.path.abspath(args.dataset), args.cache, args.batch, args.steps,
                                         hip_graph=not args.no_graph)), flush=True)
        return
    for schema in args.schemas.split(","):
        for _ in range(args.repeat):
            print(json.dumps(run(schema, args.batch, args.steps, augment=args.augment, hip_graph=not args.no_graph)), flush=True)
    # raw H2D rate of this box for scale
    x = torch.empty(1 << 30, dtype=torch.uint8).pin_memory()
    d = torch.empty_like(x, device="cuda")
    d.copy_(x, non_blocking=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        d.copy_(x, non_blocking=True)
    torch.cuda.synchronize()
    print(json.dumps({"pinned_h2d_GBps": round(5 / (time.perf_counter() - t0), 1)}))


if __name__ == "__main__":
    main()
