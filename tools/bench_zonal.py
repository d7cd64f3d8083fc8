#!/usr/bin/env python
"""Zonal inference throughput on a synthetic in-memory raster.

  python tools/bench_zonal.py [--size 6048] [--batch 8] [--write-confidence] [--zone]

Reports (a) the model forward alone (eval mode: BatchNorm folded into the conv operands, bias / ReLU / decoder
upsample+concat in conv epilogues / prologues) at the loop's batch size and at 32, and (b) the whole
run_inference loop: slicing, windowed reads + normalisation (numpy, host), H2D, forward, fused margin-crop + argmax,
D2H of 1 byte per kept pixel, window placement, writes into the in-memory output raster.  --write-confidence turns the
config key write_confidence on: label + confidence from one kernel pass, 2 bytes per kept pixel, two rasters.
--zone: instead of (b), the loop under a disc-shaped geozone covering about 40 % of the raster, with
skip_tiles_outside_zone off (every tile of the zone's bounding box is inferred) and on, in one process: tiles skipped
and the wall time of the tile loop (inference_and_write) of both.
--cog: instead of all the above, the COG conversion of a one-band class raster of --cog-size (default 5000) squared:
the overview pyramid alone for each method (hip events, best of 3 after a warm-up), the wall time of
postprocess.convert_to_cog, and the plain GeoTiffWriter.close() of the same raster for comparison (the COG holds 4/3 of
the tiles).
--tta flips|d4: the tile loop with the config key tta (V forward passes per batch, probabilities averaged in the tile's
frame), after the kernels of that path alone at the loop's shapes: ffa_tta_accumulate for an even-k and an odd-k view
and ffa_tta_predict_u8 (hip events over queued calls, best of 3 after a warm-up), with the bytes each moves per second.
--thresholds FILE: the tile loop with calibrated class thresholds in effect (the thresholded label kernels in place of
ffa_predict_u8 / ffa_tta_predict_u8); 'flat:T' stands for a file of 19 thresholds T.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

import numpy as np
import torch
import yaml


def bench_cog(size: int) -> None:
    import shutil
    import tempfile
    from flairhip import ops
    from flair_zonal_detection.geotiff import GeoTiffWriter, validate_cog
    from flair_zonal_detection.postprocess import convert_to_cog
    g = np.random.default_rng(0)
    H = W = size
    # label-like content: 8 x 8 blocks of one class, so that LZW has what a prediction raster gives it
    cls = np.repeat(np.repeat(g.integers(0, 19, (1, H // 8 + 1, W // 8 + 1), dtype=np.uint8), 8, 1), 8, 2)[:, :H, :W]
    cls = np.ascontiguousarray(cls)
    dev = torch.from_numpy(cls).cuda()
    L = ops.overview_levels(H, W, 512)
    moved = cls.nbytes + sum(-(-H // 2 ** l) * -(-W // 2 ** l) for l in range(1, L + 1))
    # the C entry point on a preallocated pyramid, queued back to back: the events then bracket kernels, not the
    # host's per-call work (ops.overview_pyramid adds an allocation and the level views, timed separately below)
    from flairhip import lib as _l
    lib, reps = _l.load(), 20
    pyr = torch.empty(int(lib.ffa_overview_pyramid_bytes(1, H, W, L)), dtype=torch.uint8, device=dev.device)
    stream = torch.cuda.current_stream().cuda_stream
    for code, method in enumerate(("nearest", "mode", "average")):
        def call():
            _l.check(lib.ffa_overview_pyramid_u8(dev.data_ptr(), pyr.data_ptr(), 1, H, W, L, code, -1, stream))
        call()  # warm-up
        best = float("inf")
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / reps)
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(reps):
            ops.overview_pyramid(dev, method=method)
        torch.cuda.synchronize()
        wall = (time.time() - t0) / reps
        print(f"overview pyramid {H}x{W}, {L} levels, {method}: {best * 1e3:.1f} us per call (hip events over {reps} "
              f"queued calls, best of 3) = {moved / best / 1e6:.0f} GB/s of {moved / 1e6:.1f} MB read + written; "
              f"ops.overview_pyramid {wall * 1e6:.1f} us per call (host clock, synchronised)")
    d = tempfile.mkdtemp(prefix="bench_cog_")
    try:
        plain, closes = os.path.join(d, "plain.tif"), []
        for _ in range(3):  # the first pass also warms the encoder pool
            w = GeoTiffWriter(plain, W, H, 1, 651000.0, 6865000.0, 0.2, crs="EPSG:2154")
            w.data[...] = cls
            t0 = time.time()
            w.close()
            closes.append(time.time() - t0)
        plain_mb = os.path.getsize(plain) / 1e6
        walls = []
        for _ in range(2):
            src = os.path.join(d, "pred.tif")
            shutil.copy(plain, src)
            t0 = time.time()
            convert_to_cog(src, os.path.join(d, "pred_COG.tif"), overview_resampling="mode")
            walls.append(time.time() - t0)
        errors = validate_cog(os.path.join(d, "pred_COG.tif"))
        print(f"GeoTiffWriter.close() {H}x{W} LZW: {min(closes[1:]):.2f} s ({plain_mb:.1f} MB); convert_to_cog (read + "
              f"GPU pyramid + write_cog, blocksize 512): {min(walls):.2f} s "
              f"({os.path.getsize(os.path.join(d, 'pred_COG.tif')) / 1e6:.1f} MB) = {min(walls) / min(closes[1:]):.2f} x "
              f"the close; validate_cog: {errors or 'valid'}")
    finally:
        shutil.rmtree(d)


HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X, TB/s: the yardstick of the streaming kernels


def bench_tta_kernels(batch: int, precision: str, mode: str, patch: int = 512, margin: int = 40, K: int = 19) -> None:
    """ffa_tta_accumulate (code 0: rows stay rows; code 4: a destination row is a column of the view) and
    ffa_tta_predict_u8 at the tile loop's shapes.  Bytes: the logits window read once, the accumulator written (first
    view) or read and written (later views); predict reads the accumulator and writes its uint8 planes."""
    from flairhip import ops
    dev = torch.device("cuda:0")
    dtype = torch.bfloat16 if precision == "bf16" else torch.float32
    cp, keep = ops.pad_channels(K), patch - 2 * margin
    logits = torch.randn(batch, patch, patch, cp, device=dev).to(dtype)
    acc = ops.tta_buffer(batch, K, keep, keep, dev, cp=cp)
    crop = (margin, margin, keep, keep)
    window_bytes = batch * keep * keep * cp * logits.element_size()
    acc_bytes = acc.numel() * 4
    planes = {"argmax": 1, "class_prob": K, "argmax_conf": 2}[mode]
    reps = 20

    def timed(call):
        call()  # warm-up
        best = float("inf")
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                call()
            b.record()
            torch.cuda.synchronize()
            best = min(best, a.elapsed_time(b) / reps)
        return best  # ms

    rows = [(f"tta_accumulate code {code} (k = {code >> 2}) {'store' if first else 'add'}",
             lambda code=code, first=first: ops.tta_accumulate_(acc, logits, K, code, crop=crop, first=first),
             window_bytes + acc_bytes * (1 if first else 2))
            for code in (0, 4) for first in (True, False)]
    rows.append((f"tta_predict_u8 {mode}", lambda: ops.tta_predict_u8(acc, mode, 8),
                 acc_bytes + batch * keep * keep * planes))
    for name, call, moved in rows:
        ms = timed(call)
        tbs = moved / ms / 1e9
        print(f"{name}: {ms * 1e3:.1f} us per call (batch {batch}, {keep} x {keep} of {patch} x {patch}, pitch {cp}, "
              f"{precision}; hip events over {reps} queued calls, best of 3) = {tbs:.2f} TB/s of {moved / 1e6:.1f} MB "
              f"= {100 * tbs / HBM_COPY_TBS:.0f} % of the {HBM_COPY_TBS} TB/s copy rate")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=6048, help="raster height = width in pixels")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--output-type", default="argmax", choices=["argmax", "class_prob"])
    ap.add_argument("--profile", action="store_true", help="cProfile of the tile loop (host hot spots)")
    ap.add_argument("--tif", action="store_true", help="also run from / to GeoTIFF files (built-in reader / writer)")
    ap.add_argument("--arch", default="resnet34-unet",
                    help="models.monotemp_model.arch, e.g. swin_base_patch4_window12_384-upernet (the fork's zonal config)")
    ap.add_argument("--channels", type=int, default=5)
    ap.add_argument("--forward-only", action="store_true", help="skip the tile loop (kernel profiles of the network)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--write-confidence", action="store_true",
                    help="run the tile loop with write_confidence: true (argmax output only)")
    ap.add_argument("--tta", default=None, choices=["flips", "d4"],
                    help="run the tile loop with the config key tta, after timing the kernels of that path alone")
    ap.add_argument("--thresholds", default=None, metavar="FILE",
                    help="run the tile loop with calibrated class thresholds (config key model_threshold_filepath; "
                         "'flat:T' writes a file of 19 thresholds T first)")
    ap.add_argument("--zone", action="store_true",
                    help="time the tile loop under a geozone with skip_tiles_outside_zone off and on")
    ap.add_argument("--cog", action="store_true",
                    help="time the overview pyramid and convert_to_cog against GeoTiffWriter.close(), nothing else")
    ap.add_argument("--cog-size", type=int, default=5000, help="with --cog: raster height = width in pixels")
    args = ap.parse_args()
    if args.cog:
        bench_cog(args.cog_size)
        return
    from flairhip.configs import unet_resnet34_config
    from flair_hub.models.flair_model import FLAIR_HUB_Model
    from flair_zonal_detection.inference import run_inference
    from flair_zonal_detection.raster import ArrayRaster

    dev = torch.device("cuda:0")
    MOD, TASK = "AERIAL_RGBI", "AERIAL_LABEL-COSIA"
    # (a) forward alone
    C = args.channels
    cfg = unet_resnet34_config(in_channels=C, precision=args.precision)
    cfg["models"]["monotemp_model"]["arch"] = args.arch
    model = FLAIR_HUB_Model(cfg, {MOD: 512}).to(dev).eval()
    for B in ((args.batch,) if args.forward_only else (args.batch, 32)):
        x = torch.randn(B, C, 512, 512, device=dev)
        with torch.no_grad():
            for _ in range(3):
                model({MOD: x})
            torch.cuda.synchronize()
            t0 = time.time()
            n = args.iters
            for _ in range(n):
                model({MOD: x})
            torch.cuda.synchronize()
        dt = (time.time() - t0) / n
        print(f"forward only, batch {B:2d}: {dt * 1e3:7.2f} ms/batch = {B / dt:8.1f} tiles/s")

    if args.forward_only:
        return
    # (b) the zonal loop
    g = np.random.default_rng(0)
    H = W = args.size
    img = g.integers(0, 255, (C, H, W), dtype=np.uint8)
    ras = ArrayRaster(img, 651000.0, 6865000.0, 0.2)
    zc = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "zonal_config.yaml")))
    zc.update({"output_path": "/tmp", "output_name": "bench_zonal", "img_pixels_detection": 512, "margin": 40,
               "output_px_meters": 0.2, "output_type": args.output_type, "batch_size": args.batch, "num_worker": 0,
               "hardware": {"precision": args.precision}, "model_weights": "/tmp/bench_zonal_weights.ckpt",
               "monotemp_arch": args.arch})
    if args.write_confidence:
        zc["write_confidence"] = True
    if args.thresholds:
        path = args.thresholds
        if path.startswith("flat:"):
            from flairhip.calibration import write_thresholds
            path = write_thresholds("/tmp/bench_zonal_thresholds.yaml", [int(path[5:])] * 19, task=TASK)
        zc["model_threshold_filepath"] = path
    if args.tta:
        bench_tta_kernels(args.batch, args.precision,
                          "argmax_conf" if args.write_confidence else args.output_type)
        zc["tta"] = args.tta
    torch.save({"state_dict": {"model." + k: v.cpu() for k, v in model.state_dict().items()}}, zc["model_weights"])
    zc["modalities"][MOD].update({"input_img_path": ras, "channels": list(range(1, C + 1)),
                                  "normalization": {"type": "custom", "means": [110.0] * C, "stds": [50.0] * C}})
    zc["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    if args.zone:
        import copy
        from flair_zonal_detection import inference as zi
        ang = np.linspace(0.0, 2.0 * np.pi, 720, endpoint=False)
        rad = np.sqrt(0.4 / np.pi) * H * 0.2  # disc of 40 % of the raster, in metres
        cx, cy = 651000.0 + W * 0.1, 6865000.0 - H * 0.1
        zone = {"type": "Polygon", "coordinates": [np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1).tolist()]}
        loops = []
        inner = zi.inference_and_write

        def timed(model_, loader_, tiles_, *a, **k):
            torch.cuda.synchronize()
            t0 = time.time()
            inner(model_, loader_, tiles_, *a, **k)
            torch.cuda.synchronize()
            loops.append((len(tiles_), time.time() - t0))
        zi.inference_and_write = timed
        run_inference(copy.deepcopy(zc), geozone=zone)  # warm-up: kernels, workspaces, graph capture
        for skip in (False, True, False, True):
            c = copy.deepcopy(zc)
            c["skip_tiles_outside_zone"] = skip
            run_inference(c, geozone=zone)
        zi.inference_and_write = inner
        (n_off, _), (n_on, _) = loops[1], loops[2]
        off, on = min(loops[1][1], loops[3][1]), min(loops[2][1], loops[4][1])
        print(f"zone of 40 % on {H}x{W} px: skip off {n_off} tiles, tile loop {off:.2f} s; skip on {n_on} tiles "
              f"({n_off - n_on} of {n_off} skipped), tile loop {on:.2f} s (best of 2 each)")
        return
    t0 = time.time()
    out = run_inference(zc)
    torch.cuda.synchronize()
    dt = time.time() - t0
    ntiles = ((H + 80 + 431) // 432) ** 2
    what = f"run_inference with tta {args.tta}" if args.tta else "run_inference"
    if args.thresholds:
        what += f" with thresholds {args.thresholds}"
    print(f"{what} on {H}x{W} px ({ntiles} tiles of 512, batch {args.batch}): {dt:.2f} s = {ntiles / dt:.1f} tiles/s, "
          f"{H * W / dt / 1e6:.1f} Mpx/s; output {out[TASK].data.shape}")

    # the same run split into its stages (second pass: kernels and workspaces are warm)
    from torch.utils.data import DataLoader
    from flair_zonal_detection import inference as zi
    from flair_zonal_detection.model_utils import build_inference_model, compute_patch_sizes
    from flair_zonal_detection.slicing import generate_patches_from_reference
    t = [time.time()]
    cfg2 = zi.prep_config(zc)
    tiles = generate_patches_from_reference(cfg2, ras, None)
    t.append(time.time())
    sizes = compute_patch_sizes(cfg2)
    mdl = build_inference_model(cfg2, sizes).to(cfg2["device"])
    t.append(time.time())
    ds = zi.prep_dataset(cfg2, tiles, sizes)
    from flair_zonal_detection.dataset import TileBatcher
    loader = TileBatcher(ds, args.batch) if TileBatcher.supports(ds) else DataLoader(ds, batch_size=args.batch,
                                                                                     pin_memory=True)
    outputs, _ = zi.init_outputs(cfg2, ras)
    t.append(time.time())
    if args.profile:
        import cProfile
        import pstats
        pr = cProfile.Profile()
        pr.enable()
    zi.inference_and_write(mdl, loader, tiles, cfg2, outputs, ras)
    torch.cuda.synchronize()
    t.append(time.time())
    if args.profile:
        pr.disable()
        pstats.Stats(pr).sort_stats("cumulative").print_stats(28)
    names = ["config + slicing", "model build + checkpoint", "dataset + output rasters", "tile loop"]
    print("  stages: " + ", ".join(f"{n} {b - a:.2f} s" for n, a, b in zip(names, t, t[1:])) +
          f"  -> tile loop alone {len(tiles) / (t[4] - t[3]):.0f} tiles/s")

    if args.tif:  # the same mosaic as an LZW GeoTIFF on disk, predictions written as GeoTIFF
        import copy
        import tempfile
        from flair_zonal_detection.geotiff import GeoTiffWriter
        d = tempfile.mkdtemp(prefix="bench_zonal_")
        src = os.path.join(d, "mosaic.tif")
        # label-like smooth content so that LZW has something to do (noise would not compress at all)
        smooth = np.repeat(np.repeat(g.integers(0, 255, (5, H // 8 + 1, W // 8 + 1), dtype=np.uint8), 8, 1), 8, 2)[:, :H, :W]
        for comp in ("lzw", None):
            t0 = time.time()
            with GeoTiffWriter.like(src, ras, 5, compress=comp) as w:
                w.data[...] = smooth
            t1 = time.time()
            zt = copy.deepcopy(zc)
            zt["modalities"][MOD]["input_img_path"] = src
            zt["output_path"] = d
            out = run_inference(zt)
            torch.cuda.synchronize()
            dt = time.time() - t1
            print(f"GeoTIFF in ({comp or 'uncompressed'}, {os.path.getsize(src) / 1e6:.0f} MB, written in {t1 - t0:.1f} s) "
                  f"-> GeoTIFF out ({os.path.getsize(out[TASK].path) / 1e6:.1f} MB): {dt:.2f} s = {ntiles / dt:.1f} tiles/s")
        import shutil
        shutil.rmtree(d)


if __name__ == "__main__":
    main()
