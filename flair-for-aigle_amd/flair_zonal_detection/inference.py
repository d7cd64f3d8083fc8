"""Zonal tiled inference -- counterpart of the reference's flair_zonal_detection/inference.py
(prep_config :54-73, initialize_geometry_and_resolutions :76-132, prep_dataset :136-154, init_outputs
:157-208, inference_and_write :254-355, run_inference :644-674).

The tile loop keeps the reference's semantics -- per tile: drop the margin, convert to uint8, place the
window at int(round((left - L) / res)), int(round((T - top) / res)), clip to the raster, skip empty windows,
last writer wins -- and moves the per-pixel work onto the GPU:

    reference (per tile)                             here (per batch)
    D2H of f32 logits, 19.9 MB                       margin crop + argmax / class_prob fused in one HIP kernel
    numpy argmax over 19 x 432 x 432                 over the whole batch (ffa_predict_u8), D2H of uint8:
    scipy nearest zoom (optional)                    0.19 MB per tile; window maths by ffa_write_window
    rasterio window write                            (bit-exact with inference.py:318-335), then the same write

Polygonisation of the written raster (raster_to_polygons, reference :359-413) runs on the GPU as well
(csrc/polygonize.hip: labelling, boundary edges, ring assembly) with a host topology-preserving simplifier
(csrc/polygon_simplify.cpp) and a GDAL-free GeoPackage writer (gpkg.py).  Clipping to the geozone and the class filter
of the fork's postprocess_results happen on the pixel grid before polygonisation (``raster_to_polygons(zone=, classes=)``,
csrc/zone_mask.hip, zone.py), and with the config key ``skip_tiles_outside_zone`` the tile loop leaves out the tiles
that hold no zone pixel.  A zone in another CRS than the raster's (``geozone_crs`` / ``zone_crs``) and polygons wanted in
another one (``target_crs``) are reprojected on the GPU (csrc/crs_transform.hip, crs.py).  With the config key
``cog_conversion`` the written rasters become cloud-optimised GeoTIFFs (postpro_outputs, reference :633-641): the overview
pyramid comes from the GPU (csrc/overview.hip), the file layout from geotiff.write_cog.

Per-polygon confidence (the column the fork's driver fills with random numbers, scripts/
run_fast_aigle_segmentation.py:162-163, and its unused second path :566-630 means to compute): with the config key
``write_confidence`` the tile loop writes a second uint8 raster, rint(255 * max softmax) of every pixel, from the same
kernel pass as the label, and ``raster_to_polygons(..., confidence=...)`` adds the columns ``confidence`` (mean over
the polygon's pixels, from exact integer sums taken on the GPU) and ``pixels``.  ``logits_to_labels_and_confidence``
and ``vectorize_segmentation_parallel`` carry the fork's names for that path.

Test-time augmentation (config key ``tta``: none, flips or d4): every tile is predicted under 4 or 8 flips / rotations
of the square -- the transforms the network was trained with (flairhip/augment.py) -- and the softmax probabilities of
the views are averaged in the tile's own frame (csrc/tta.hip) before the uint8 conversion; the outputs keep their
shapes, so everything after the conversion is shared with the plain loop.
"""
from __future__ import annotations

import glob
import logging
import os
import time
from typing import Dict, Optional, Tuple

import numpy as np
import torch
from torch.utils.data import DataLoader

from flairhip import ops
from flairhip.augment import tta_views
from flair_zonal_detection.config import (config_recap_1, config_recap_2, load_config, validate_cog_conversion,
                                          validate_cog_overview_resampling, validate_config, validate_geozone_crs,
                                          threshold_file, validate_skip_tiles_outside_zone, validate_threshold_fallback,
                                          validate_change, validate_tta, validate_write_confidence,
                                          validate_zone_stats)
from flair_zonal_detection.dataset import MultiModalSlicedDataset, TileBatcher, pad_series_collate
from flair_zonal_detection.model_utils import build_inference_model, compute_patch_sizes
from flair_zonal_detection.postprocess import convert, convert_to_cog  # noqa: F401  (re-exported like the reference)
from flair_zonal_detection.raster import ArrayRaster, make_window, open_raster
from flair_zonal_detection.slicing import generate_patches_from_reference

logger = logging.getLogger(__name__)


def overwrite_config(config: dict, model_ckpt_path: str, model_threshold_filepath: str, result_folder: str,
                     log_folder: str) -> Dict:
    config["model_weights"] = model_ckpt_path
    config["model_threshold_filepath"] = model_threshold_filepath
    config["output_path"] = result_folder
    config["log_folder"] = log_folder
    return config


def prep_config(config_path: str, model_ckpt_path: Optional[str] = None, model_threshold_filepath: Optional[str] = None,
                result_folder: Optional[str] = None, log_folder: Optional[str] = None,
                images_folder: Optional[str] = None) -> Dict:
    """Load + validate the YAML, resolve geometry, pick the device.  Accepts the fork's six-argument call
    (scripts/run_fast_aigle_segmentation.py:75) and upstream FLAIR-HUB's one-argument call."""
    config = load_config(config_path) if isinstance(config_path, str) else config_path
    if images_folder is not None:
        # the fork's caller feeds BD ORTHO JPEG-2000 tiles (scripts/run_fast_aigle_segmentation.py:88): opened by
        # rasterio (GDAL) when installed, else by jp2.Jp2Raster (OpenJPEG through Pillow); with neither only GeoTIFF
        # rasters can be opened (geotiff.py), so say so HERE instead of globbing *.jp2 and failing at the first read
        from flair_zonal_detection import jp2
        try:
            import rasterio  # type: ignore  # noqa: F401
            can_jp2 = True
        except ImportError:
            can_jp2 = jp2.openjpeg_available()
        patterns = ("*.jp2", "*.tif", "*.tiff") if can_jp2 else ("*.tif", "*.tiff")
        if not can_jp2 and glob.glob(os.path.join(images_folder, "*.jp2")):
            logger.warning("%s holds JPEG-2000 rasters, which need rasterio / GDAL or a Pillow with OpenJPEG (neither "
                           "installed): only GeoTIFF inputs are considered", images_folder)
        rasters = sorted(p for pat in patterns for p in glob.glob(os.path.join(images_folder, pat)))
        if not rasters:
            raise FileNotFoundError(f"no raster ({', '.join(patterns)}) in {images_folder}"
                                    + ("" if can_jp2 else
                                       "; JPEG-2000 inputs need rasterio or a Pillow with OpenJPEG, which are not installed"))
        config["modalities"]["AERIAL_RGBI"]["input_img_path"] = rasters[0]
    if model_ckpt_path is not None:
        config = overwrite_config(config, model_ckpt_path, model_threshold_filepath, result_folder, log_folder)
    validate_config(config)
    config_recap_1(config)
    config = initialize_geometry_and_resolutions(config)
    config_recap_2(config)
    use_gpu = config.get("use_gpu", True)
    if not (use_gpu and torch.cuda.is_available()):
        raise RuntimeError("the libflairhip tile loop needs an MI355X (use_gpu must be true and a GPU present); "
                           "there is no CPU path in the product")
    config["device"] = torch.device("cuda")
    config["output_type"] = config.get("output_type", "argmax")
    return config


def initialize_geometry_and_resolutions(config: Dict) -> Dict:
    """reference_resolution (finest active modality, rounded to 5 decimals), per-modality resolutions, image
    bounds / shape, tile and margin size in metres; bounds of all active modalities must agree within 1e-2."""
    modalities = config["modalities"]
    active = [m for m, on in modalities["inputs"].items() if on]
    resolutions, bounds = {}, []
    for mod in active:
        path = modalities[mod]["input_img_path"]
        src = open_raster(path)
        try:
            resolutions[mod] = round(src.res[0], 5)
            bounds.append((mod, src.bounds))
            if "image_shape_px" not in config:
                config["image_shape_px"] = {"height": src.height, "width": src.width}
        finally:
            if isinstance(path, (str, bytes)):
                src.close()
    ref_mod, ref_bounds = bounds[0]
    for mod, b in bounds[1:]:
        if not np.allclose(tuple(b), tuple(ref_bounds), atol=1e-2):
            raise ValueError(f"Bounds mismatch between '{ref_mod}' and '{mod}':\n  {ref_mod}: {ref_bounds}\n  {mod}: {b}")
    ref_mod, reference_resolution = min(resolutions.items(), key=lambda kv: kv[1])
    config["reference_modality"] = ref_mod
    config["reference_resolution"] = reference_resolution
    config["modality_resolutions"] = resolutions
    config["image_bounds"] = {"left": ref_bounds.left, "bottom": ref_bounds.bottom, "right": ref_bounds.right,
                              "top": ref_bounds.top}
    config["tile_size_m"] = round(config["img_pixels_detection"] * reference_resolution, 2)
    config["margin_size_m"] = round(config["margin"] * reference_resolution, 2)
    return config


def prep_dataset(config: Dict, tiles_gdf, patch_sizes: Dict[str, int]) -> MultiModalSlicedDataset:
    active = [m for m, on in config["modalities"]["inputs"].items() if on]
    config["labels"] = [t["name"] for t in config["tasks"] if t["active"]]
    config["labels_configs"] = {t["name"]: {"value_name": t["class_names"]} for t in config["tasks"] if t["active"]}
    return MultiModalSlicedDataset(dataframe=tiles_gdf, modality_cfgs={m: config["modalities"][m] for m in active},
                                   patch_size_dict=patch_sizes, ref_date_str=config.get("multitemp_model_ref_date", "05-15"),
                                   modalities_config=config,
                                   device_normalize=bool(config.get("device_normalize", True)))


CONFIDENCE_SUFFIX = "_confidence"  # outputs / paths key of a task's confidence raster: f"{task}_confidence"


def init_outputs(config: Dict, ref_img, i=None) -> Tuple[Dict[str, object], Dict[str, str]]:
    """One uint8 output raster per active task (1 band for argmax, K for class_prob), on the reference raster's
    grid or on an output_px_meters grid when that differs from the reference resolution.  With write_confidence a
    second one-band raster per task, ``<output_name>_<task>_confidence_i.tif``, under the key f"{task}_confidence"."""
    output_type = config["output_type"]
    ref_res = config["reference_resolution"]
    out_res = config.get("output_px_meters", ref_res)
    ib = config["image_bounds"]
    needs_rescale = abs(ref_res - out_res) > 1e-6
    outputs, paths = {}, {}
    for task in config["tasks"]:
        if not task["active"]:
            continue
        k = len(task["class_names"])
        suffix = "argmax" if output_type == "argmax" else "class-prob"
        rasters = [(task["name"], k if output_type == "class_prob" else 1, suffix)]
        if validate_write_confidence(config):
            rasters.append((task["name"] + CONFIDENCE_SUFFIX, 1, "confidence"))
        if needs_rescale:
            h = int(round((ib["top"] - ib["bottom"]) / out_res))
            w = int(round((ib["right"] - ib["left"]) / out_res))
        else:
            h, w = ref_img.height, ref_img.width
        for key, count, suffix in rasters:
            path = os.path.join(config["output_path"], f"{config['output_name']}_{task['name']}_{suffix}_i.tif")
            if config.get("shard") is not None:  # one part file per rank; geotiff.merge_shard_files joins them
                path = path[:-4] + ".r{}of{}.tif".format(*config["shard"])
            if isinstance(ref_img, ArrayRaster):
                outputs[key] = ArrayRaster(np.zeros((count, h, w), np.uint8), ib["left"], ib["top"], out_res,
                                           ref_img.crs)
            else:
                try:
                    import rasterio  # type: ignore
                except ImportError:
                    rasterio = None
                # a sharded run joins per-rank part files + "written" masks (geotiff.merge_shard_files): that protocol
                # belongs to the built-in writer, so it is used for the parts even where rasterio is installed
                if rasterio is None or config.get("shard") is not None:  # tiled, LZW, written on close()
                    from flair_zonal_detection.geotiff import GeoTiffWriter
                    os.makedirs(config["output_path"], exist_ok=True)
                    outputs[key] = GeoTiffWriter.like(path, ref_img, count, np.uint8, width=w, height=h,
                                                      left=ib["left"], top=ib["top"],
                                                      res=out_res if needs_rescale else ref_img.res)
                else:
                    from rasterio.transform import from_origin  # type: ignore
                    profile = ref_img.profile.copy()
                    profile.update({"count": count, "dtype": "uint8", "compress": "lzw"})
                    if needs_rescale:
                        profile.update({"driver": "GTiff", "height": h, "width": w,
                                        "transform": from_origin(ib["left"], ib["top"], out_res, out_res)})
                    outputs[key] = rasterio.open(path, "w", **profile)
            paths[key] = path
    return outputs, paths


def _zoom_index(n: int, scale: float):
    """Source index of every output position of ``scipy.ndimage.zoom(x, scale, order=0)`` along an axis of length
    n, or -1 where scipy writes its constant 0 (reference inference.py:212-226 calls zoom with the default
    mode='constant', grid_mode=False).  scipy maps output i to the input coordinate cc = i * (n - 1) / (out - 1),
    out = round(n * scale), in float64, takes floor(cc + 0.5) for order 0 and treats cc > n - 1 -- which float
    rounding produces for the LAST position of some (n, scale) pairs, e.g. n = 226, scale 0.5 -- as outside the
    array.  Checked against scipy on 1.8 M positions (tests/test_oracle_goldens.py)."""
    import math
    out = int(round(n * scale))
    step = (n - 1) / (out - 1) if out > 1 else 1.0
    idx = []
    for i in range(out):
        cc = i * step
        idx.append(-1 if (cc < 0.0 or cc > n - 1) else int(math.floor(cc + 0.5)))
    return idx


def _nearest_zoom(pred: torch.Tensor, scale: float) -> torch.Tensor:
    """scipy.ndimage.zoom(order=0) on the last two axes, position for position (resample_prediction, reference
    inference.py:212-226)."""
    h, w = pred.shape[-2:]
    ys = torch.tensor(_zoom_index(h, scale), dtype=torch.long, device=pred.device)
    xs = torch.tensor(_zoom_index(w, scale), dtype=torch.long, device=pred.device)
    out = pred[..., ys.clamp(min=0), :][..., xs.clamp(min=0)]
    if bool((ys < 0).any()) or bool((xs < 0).any()):
        out = out.clone()
        out[..., ys < 0, :] = 0
        out[..., xs < 0] = 0
    return out


@torch.no_grad()
def inference_and_write(model: torch.nn.Module, dataloader: DataLoader, tiles_gdf, config: Dict,
                        output_files: Dict[str, object], ref_img) -> None:
    device = config["device"]
    margin = config["margin"]
    tile_size = config["img_pixels_detection"]
    output_type = config["output_type"]
    if output_type not in ("argmax", "class_prob"):
        raise ValueError(f"Unknown output type: {output_type}")
    # label + confidence: one kernel pass, one [B, 2, h, w] tensor per task through zoom, D2H and window placement, so
    # the two planes of a pixel always come from the same tile
    with_conf = validate_write_confidence(config)
    predict_mode = "argmax_conf" if with_conf else output_type
    ref_res = config["reference_resolution"]
    out_res = config.get("output_px_meters", ref_res)
    needs_rescale = abs(ref_res - out_res) > 1e-6
    scale = ref_res / out_res if needs_rescale else 1.0
    img_bounds = tuple(ref_img.bounds)  # (left, bottom, right, top)
    keep = tile_size - 2 * margin

    # raw raster tiles (dataset with device_normalize): the per-channel (mean, std) ride along once per modality
    norms = {}
    ds = getattr(dataloader, "dataset", None)
    if getattr(ds, "device_normalize", False):
        for mod in ds.modalities:
            if ds.delivers_raw(mod):
                norms[mod + "_NORM"] = torch.tensor(np.stack(ds.norm_vectors(mod)), dtype=torch.float32, device=device)

    # tile columns as plain arrays: a pandas row lookup costs ~0.5 ms, twice per tile
    lefts, tops, ids = (np.asarray(tiles_gdf[c]) for c in ("left", "top", "id"))
    graphed = None  # hipGraph of forward + conversion for full batches (the eval forward is ~120 launches)
    use_graph = bool(config.get("hip_graph", True)) and str(device).startswith("cuda")

    # calibrated class thresholds (config["model_threshold_filepath"], flairhip.calibration): read and uploaded once per
    # task, at the first forward (the eager warm-up of a graphed run); the labels -- and the confidence plane -- then
    # come from the thresholded entries, same shapes and dtypes.  Without a file the calls are the plain ones.
    thr_path = threshold_file(config)
    fallback = validate_threshold_fallback(config)
    thr_dev: Dict[str, torch.Tensor] = {}

    def thresholds(task_name, classes):
        thr = thr_dev.get(task_name)
        if thr is None:
            from flairhip.calibration import read_thresholds
            thr = thr_dev[task_name] = torch.from_numpy(read_thresholds(thr_path, classes, task=task_name)
                                                        ["thresholds_u8"]).to(device)
        return thr

    def forward_eager(inputs):
        logits_tasks, _ = model(inputs)
        preds = {}
        for task_name, logits in logits_tasks.items():
            if thr_path is not None:
                preds[task_name] = ops.predict_thresholded_u8(
                    logits._ffa_nhwc, logits._ffa_classes, predict_mode, thresholds(task_name, logits._ffa_classes),
                    fallback, crop=(margin, margin, keep, keep))
                continue
            preds[task_name] = ops.predict_u8(logits._ffa_nhwc, logits._ffa_classes, predict_mode,
                                              crop=(margin, margin, keep, keep))
        return preds

    # test-time augmentation (config key tta): one forward per view, the model's layout kernels apply the view's code to
    # every modality (batch["AUG"]); each view's probabilities go back to the tile's frame and into an f32 accumulator
    # (ffa_tta_accumulate), and the uint8 outputs come from the mean (ffa_tta_predict_u8): same shapes and dtypes as
    # above, so everything downstream is shared.  The whole loop is one graph replay for a full batch.
    views = tta_views(validate_tta(config))
    view_codes: Dict[Tuple[int, int], torch.Tensor] = {}  # (code, batch size) -> constant device uint8 [B]

    def forward_tta(inputs):
        batch_size = next(v.shape[0] for k_, v in inputs.items() if not k_.endswith("_NORM"))
        accs = {}
        for v, code in enumerate(views):
            codes_v = view_codes.get((code, batch_size))
            if codes_v is None:
                codes_v = view_codes[(code, batch_size)] = torch.full((batch_size,), code, dtype=torch.uint8,
                                                                      device=device)
            logits_tasks, _ = model({**inputs, "AUG": codes_v})
            for task_name, logits in logits_tasks.items():
                nhwc, classes = logits._ffa_nhwc, logits._ffa_classes
                if v == 0:
                    accs[task_name] = ops.tta_buffer(nhwc.shape[0], classes, keep, keep, nhwc.device, cp=nhwc.shape[3])
                ops.tta_accumulate_(accs[task_name], nhwc, classes, code, crop=(margin, margin, keep, keep),
                                    first=v == 0)
        if thr_path is not None:
            return {task_name: ops.tta_predict_thresholded_u8(acc, predict_mode, len(views),
                                                              thresholds(task_name, acc._ffa_classes), fallback)
                    for task_name, acc in accs.items()}
        return {task_name: ops.tta_predict_u8(acc, predict_mode, len(views)) for task_name, acc in accs.items()}

    forward = forward_tta if len(views) > 1 else forward_eager

    def write_batch(indices, host_preds):
        """host side of one batch: window placement + raster writes (reference inference.py:297-352)"""
        for task_name, (buf, done) in host_preds.items():
            done.synchronize()
            pred = buf[:len(indices)].numpy()  # uint8: [B,h,w], [B,K,h,w] or [B,2,h,w] (label, confidence)
            for i in range(len(indices)):
                ti = int(indices[i])
                p = pred[i]
                win = ops.write_window(lefts[ti], tops[ti], img_bounds, out_res, p.shape[-2], p.shape[-1])
                if win.skip:
                    logger.info("skipping tile %s: window out of bounds", ids[ti])
                    continue
                p = p[..., :win.height, :win.width]
                window = make_window(win.col_off, win.row_off, win.width, win.height)
                if with_conf:
                    output_files[task_name].write(p[0], 1, window=window)
                    output_files[task_name + CONFIDENCE_SUFFIX].write(p[1], 1, window=window)
                elif output_type == "argmax":
                    output_files[task_name].write(p, 1, window=window)
                else:
                    for c in range(p.shape[0]):
                        output_files[task_name].write(p[c], c + 1, window=window)

    # Two-stage software pipeline: the device works on batch k (H2D, forward, conversion, D2H into a pinned buffer,
    # all stream-ordered and asynchronous) while the host writes the windows of batch k-1 and reads the tiles of
    # batch k+1.  Pinned D2H buffers alternate; the loader's input buffers do too (TileBatcher).
    full = getattr(dataloader, "bs", None) or getattr(dataloader, "batch_size", None)
    host_bufs: Dict[str, list] = {}
    pending = None
    for k, batch in enumerate(dataloader):
        inputs = {k_: v.to(device, non_blocking=True) for k_, v in batch.items()
                  if k_ != "index" and torch.is_tensor(v)}
        for k_, v in norms.items():
            if inputs.get(k_[:-5]) is not None:
                inputs[k_] = v
        indices = batch["index"].cpu().numpy().flatten()
        if use_graph and full and len(indices) == full:
            if graphed is None:
                from flairhip.graph import GraphedCall
                graphed = GraphedCall(forward, inputs)
            preds = graphed(inputs)
        else:
            preds = forward(inputs)
        host_preds = {}
        for task_name, pred in preds.items():
            if needs_rescale:
                pred = _nearest_zoom(pred, scale)
            bufs = host_bufs.get(task_name)
            if bufs is None or bufs[0].shape[1:] != pred.shape[1:] or bufs[0].shape[0] < pred.shape[0]:
                shape = (max(int(full or 0), pred.shape[0]),) + tuple(pred.shape[1:])
                bufs = host_bufs[task_name] = [torch.empty(shape, dtype=pred.dtype).pin_memory() for _ in range(2)]
            buf = bufs[k & 1]
            buf[:pred.shape[0]].copy_(pred, non_blocking=True)  # before the next replay overwrites the graph's output
            done = torch.cuda.Event()
            done.record()
            host_preds[task_name] = (buf, done)
        if pending is not None:
            write_batch(*pending)
        pending = (indices, host_preds)
    if pending is not None:
        write_batch(*pending)
    for dst in output_files.values():
        dst.close()


def shard_tiles(tiles, rank: int, world: int):
    """Tiles of one rank of a sharded run: a CONTIGUOUS slice of the grid order (outer loop x, inner y).  No
    collective is needed -- tiles are independent units -- and contiguity keeps the reference's "last writer wins"
    for the clamped last row / column inside a shard; across shards merge_shard_outputs restores it by rank order."""
    if not (0 <= rank < world):
        raise ValueError(f"shard rank {rank} outside world size {world}")
    n = len(tiles)
    return tiles.iloc[rank * n // world:(rank + 1) * n // world].reset_index(drop=True)


def merge_shard_outputs(outputs_by_rank):
    """One set of output rasters from the per-rank rasters of a sharded in-memory run (ArrayRaster with
    track_writes): pixels a later rank wrote replace those of earlier ranks, i.e. grid order = write order."""
    merged = {}
    for task, first in outputs_by_rank[0].items():
        out = ArrayRaster(first.data.copy(), first.left, first.top, first._res, first.crs)
        for part in outputs_by_rank[1:]:
            r = part[task]
            if r.written is None:
                raise ValueError("merge_shard_outputs needs rasters that tracked their writes")
            out.data[:, r.written] = r.data[:, r.written]
        merged[task] = out
    return merged


def tile_zone_windows(tiles, left: float, top: float, xres: float, yres: float) -> np.ndarray:
    """int64 [n, 4] pixel rectangles (r0, c0, r1, c1) of the tiles' kept bounds on the grid anchored at (left, top):
    snapped outward and grown by one pixel on every side (not clamped: ops.zone_window_counts clamps)."""
    tl, tb, tr, tt = (np.asarray(tiles[k], dtype=np.float64) for k in ("left", "bottom", "right", "top"))
    win = np.empty((len(tl), 4), dtype=np.int64)
    win[:, 0] = np.floor((top - tt) / yres) - 1
    win[:, 1] = np.floor((tl - left) / xres) - 1
    win[:, 2] = np.ceil((top - tb) / yres) + 1
    win[:, 3] = np.ceil((tr - left) / xres) + 1
    return win


def drop_tiles_outside_zone(tiles, ref_img, geozone):
    """The tiles whose kept area can hold a zone pixel (config key skip_tiles_outside_zone).  The zone is rasterised on
    the reference raster's grid (pixel centre inside the contour) and counted per tile over the kept bounds snapped
    outward and grown by a pixel, so a dropped tile cannot have written a zone pixel whatever output rescaling or
    the clamping of the last row / column does: inside the zone the rasters equal those of the full run."""
    from flair_zonal_detection.zone import zone_mask
    b = ref_img.bounds
    left, top = float(b.left), float(b.top)
    xres, yres = (float(v) for v in ref_img.res)
    H, W = int(ref_img.shape[0]), int(ref_img.shape[1])
    mask = zone_mask(geozone, left, top, xres, yres, H, W)
    counts = ops.zone_window_counts(mask, tile_zone_windows(tiles, left, top, xres, yres)).cpu().numpy()
    keep = counts > 0
    logger.info("%d of %d tiles outside the zone skipped", int((~keep).sum()), len(keep))
    return tiles[keep].reset_index(drop=True)


def postpro_outputs(temp_paths: Dict[str, str], config: Dict) -> Dict[str, str]:
    """The reference's postpro_outputs (inference.py:633-641): with ``cog_conversion`` every written raster ``p`` of
    ``temp_paths`` ({output key: path}) is converted to the cloud-optimised ``p.replace(".tif", "_COG.tif")`` and
    removed.  Returns {output key: the path the raster now has}.  Overviews by ``cog_overview_resampling``: nearest
    (default) or average for every raster; with mode the class rasters take the mode, the confidence and
    class-probability rasters the average."""
    paths = dict(temp_paths)
    if not validate_cog_conversion(config):
        return paths
    method = validate_cog_overview_resampling(config)
    for key, temp_path in temp_paths.items():
        classes = config.get("output_type", "argmax") == "argmax" and not str(key).endswith(CONFIDENCE_SUFFIX)
        cog_path = temp_path.replace(".tif", "_COG.tif")  # the reference's naming; convert_to_cog refuses a name it leaves as it is
        t0 = time.time()
        convert_to_cog(temp_path, cog_path, overview_resampling="average" if method == "mode" and not classes else method)
        logger.info("converted to COG in %.1f s: %s", time.time() - t0, cog_path)
        paths[key] = cog_path
    return paths


ZONE_STATS_SUFFIX = "_zone_stats.csv"  # <name>.tif -> <name>_zone_stats.csv


def write_zone_stats(outputs: Dict[str, object], config: Dict, zones, id_field=None, zone_crs=None) -> Dict[str, str]:
    """The config key ``zone_stats``: for every class raster the run wrote to a file ``<name>.tif``, the table of
    zonal_stats.zonal_class_stats over the zone layer ``zones`` as ``<name>_zone_stats.csv``; with write_confidence
    the table has the confidence columns.  Class-probability and in-memory outputs are left alone.  Returns
    {output key: path of the table}."""
    from flair_zonal_detection.geotiff import GeoTiffWriter
    from flair_zonal_detection.zonal_stats import write_zone_stats_csv, zonal_class_stats
    if config.get("output_type", "argmax") != "argmax":
        logger.info("zone_stats: needs class rasters (output_type: argmax), not %s", config.get("output_type"))
        return {}
    names = {t["name"]: t.get("class_names") for t in config.get("tasks", [])}
    written = {}
    for key, out in outputs.items():
        if str(key).endswith(CONFIDENCE_SUFFIX):
            continue
        out_path = getattr(out, "path", None) or getattr(out, "name", None)
        if (isinstance(out, ArrayRaster) and not isinstance(out, GeoTiffWriter)) or not out_path:
            logger.info("zone_stats: the in-memory output %s is not tabulated (zonal_class_stats takes it directly)", key)
            continue
        t0 = time.time()
        table = zonal_class_stats(out, zones, id_field=id_field, confidence=outputs.get(str(key) + CONFIDENCE_SUFFIX),
                                  zone_crs=zone_crs, class_names=names.get(key) or None)
        path = os.path.splitext(str(out_path))[0] + ZONE_STATS_SUFFIX
        written[key] = write_zone_stats_csv(table, path)
        logger.info("zone statistics of %d zones in %.1f s: %s", table.n_zones, time.time() - t0, path)
    return written


ZONE_CHANGE_SUFFIX = "_zone_change.csv"            # <name>.tif -> <name>_zone_change.csv (one line per zone)
ZONE_TRANSITIONS_SUFFIX = "_zone_transitions.csv"  # ... and <name>_zone_transitions.csv (one per zone, from, to)


def change_source(change_from, key, class_keys):
    """the ``before`` raster of the output ``key``: the {task: path} entry, or the bare path when the run has one class
    raster (ValueError with more: a bare path cannot say which); None when the dict does not list the task"""
    if isinstance(change_from, dict):
        return change_from.get(key)
    if len(class_keys) > 1:
        raise ValueError(f"change_from is one path but the run wrote {len(class_keys)} class rasters "
                         f"({', '.join(map(str, class_keys))}): give {{task: path}}")
    return change_from


def write_change_stats(outputs: Dict[str, object], config: Dict, change_from, zones=None, id_field=None,
                       zone_crs=None) -> Dict[str, Tuple[str, str]]:
    """The config key ``change_from``: for every class raster the run wrote to a file ``<name>.tif`` (``outputs``
    values: closed writers or paths), the tables of change.zonal_change_stats against the earlier run's raster as
    ``<name>_zone_change.csv`` and ``<name>_zone_transitions.csv`` -- over the zone layer ``zones``, or with None over
    the whole raster as one zone; with write_confidence the tables have the confidence columns.  Class-probability and
    in-memory outputs are left alone.  Returns {output key: (wide path, long path)}."""
    from flair_zonal_detection.change import write_change_csv, write_transitions_csv, zonal_change_stats
    from flair_zonal_detection.geotiff import GeoTiffWriter
    if config.get("output_type", "argmax") != "argmax":
        logger.info("change_from: needs class rasters (output_type: argmax), not %s", config.get("output_type"))
        return {}
    names = {t["name"]: t.get("class_names") for t in config.get("tasks", [])}
    files = {}
    for key, out in outputs.items():
        if str(key).endswith(CONFIDENCE_SUFFIX):
            continue
        out_path = out if isinstance(out, (str, os.PathLike)) else getattr(out, "path", None) or getattr(out, "name", None)
        if (isinstance(out, ArrayRaster) and not isinstance(out, GeoTiffWriter)) or not out_path:
            logger.info("change_from: the in-memory output %s is not tabulated (zonal_change_stats takes it directly)", key)
            continue
        files[key] = (out, str(out_path))
    written = {}
    for key, (out, out_path) in files.items():
        before = change_source(change_from, key, list(files))
        if before is None:
            logger.info("change_from: no earlier raster listed for %s", key)
            continue
        t0 = time.time()
        table = zonal_change_stats(before, out, zones, id_field=id_field,
                                   confidence=outputs.get(str(key) + CONFIDENCE_SUFFIX), zone_crs=zone_crs,
                                   class_names=names.get(key) or None)
        stem = os.path.splitext(out_path)[0]
        written[key] = (write_change_csv(table, stem + ZONE_CHANGE_SUFFIX),
                        write_transitions_csv(table, stem + ZONE_TRANSITIONS_SUFFIX))
        logger.info("class transitions of %d zones in %.1f s: %s, %s", table.n_zones, time.time() - t0, *written[key])
    return written


def run_inference(config_path, ref_raster=None, geozone=None, shard: Optional[Tuple[int, int]] = None,
                  before_loop=None, geozone_crs=None) -> Dict[str, object]:
    """End-to-end zonal run with upstream FLAIR-HUB's one-argument semantics (the fork's own run_inference is
    stale: inference.py:650-665 calls its helpers with the wrong arity).  Returns the output rasters.
    ``geozone`` (any form zone.zone_rings reads, in the raster's CRS) restricts the tile grid to its bounding box;
    with the config key ``skip_tiles_outside_zone: true`` the tiles holding no pixel of the zone are dropped as well
    (drop_tiles_outside_zone).  ``geozone_crs`` (or the config key of that name; None = the raster's CRS, as before)
    names the CRS the zone is given in -- anything crs.parse accepts, or "auto" for GeoJSON -- and the zone is then
    reprojected to the raster's CRS once, before slicing (zone.zone_in_raster_crs, the reference's
    ``gdf_geozone.to_crs(config.input_crs)``).  ``shard=(rank, world)`` (or config['shard']) restricts the run to that rank's slice of the tile grid: one process
    per GPU, no communication; in-memory outputs then track their writes for merge_shard_outputs.  ``before_loop``
    (optional) is called with the freshly initialised outputs before the first tile is processed."""
    t0 = time.time()
    config = prep_config(config_path)
    ref_path = config["modalities"][config["reference_modality"]]["input_img_path"]
    ref_img = ref_raster if ref_raster is not None else open_raster(ref_path)
    if geozone is not None:
        from flair_zonal_detection.zone import zone_in_raster_crs
        geozone_crs = geozone_crs if geozone_crs is not None else validate_geozone_crs(config)
        geozone = zone_in_raster_crs(geozone, geozone_crs, getattr(ref_img, "crs", None))
    tiles = generate_patches_from_reference(config, ref_img, geozone)
    if validate_skip_tiles_outside_zone(config) and geozone is not None and len(tiles):
        tiles = drop_tiles_outside_zone(tiles, ref_img, geozone)
    shard = shard if shard is not None else config.get("shard")
    if shard is not None:
        config["shard"] = (int(shard[0]), int(shard[1]))
        tiles = shard_tiles(tiles, int(shard[0]), int(shard[1]))
    patch_sizes = compute_patch_sizes(config)
    model = build_inference_model(config, patch_sizes).to(config["device"])
    dataset = prep_dataset(config, tiles, patch_sizes)
    if TileBatcher.supports(dataset) and not config.get("num_worker", 0):
        loader = TileBatcher(dataset, config.get("batch_size", 8))  # uint8 tiles straight into pinned batch buffers
    else:
        series = any(m.endswith("_TS") for m in dataset.modalities)
        loader = DataLoader(dataset, batch_size=config.get("batch_size", 8), num_workers=config.get("num_worker", 0),
                            pin_memory=True, collate_fn=pad_series_collate if series else None)
        if series and dataset.mask_reader is not None:
            config["hip_graph"] = False  # per-tile cloud filtering: the number of dates changes from batch to batch
    outputs, _ = init_outputs(config, ref_img)
    if before_loop is not None:
        before_loop(outputs)
    if shard is not None:
        for o in outputs.values():
            if isinstance(o, ArrayRaster):
                o.track_writes()
    inference_and_write(model, loader, tiles, config, outputs, ref_img)
    logger.info("zonal inference of %d tiles took %.1f s", len(tiles), time.time() - t0)
    zone_layer, zone_id, zone_layer_crs = validate_zone_stats(config)
    if zone_layer is not None:  # before the COG conversion removes the plain rasters
        if shard is not None:
            logger.info("zone_stats: the part files of a sharded run are not tabulated")
        else:
            write_zone_stats(outputs, config, zone_layer, zone_id, zone_layer_crs)
    change_from, _ = validate_change(config)
    if change_from is not None:  # likewise before the COG conversion
        if shard is not None:
            logger.info("change_from: the part files of a sharded run are not tabulated (rank 0 does it after the merge)")
        else:
            write_change_stats(outputs, config, change_from, zone_layer, zone_id, zone_layer_crs)
    if validate_cog_conversion(config):
        from flair_zonal_detection.geotiff import GeoTiffWriter
        files = {k: o.path for k, o in outputs.items() if isinstance(o, GeoTiffWriter)}
        if shard is not None:
            logger.info("cog_conversion: the part files of a sharded run are not converted; the conversion follows "
                        "merge_shard_files")
        elif files:
            for key, path in postpro_outputs(files, config).items():
                outputs[key].path = path  # raster_to_polygons(outputs) reads the file that now exists
        else:
            logger.info("cog_conversion: in-memory outputs are left as they are")
    return outputs


def _polygon_source(tiff_path):
    """The raster raster_to_polygons reads: the reference passes the output_files dict of init_outputs / run_inference
    and opens its 'AERIAL_LABEL-COSIA' entry (inference.py:389); a lone entry, a path or a raster object also do."""
    return _open_polygon_raster(_class_entry(tiff_path)[1])


def _class_entry(src):
    """(key, value) of the class raster in an outputs dict (confidence rasters are not candidates); (None, src) for
    anything that is not a dict"""
    if not isinstance(src, dict):
        return None, src
    if "AERIAL_LABEL-COSIA" in src:
        return "AERIAL_LABEL-COSIA", src["AERIAL_LABEL-COSIA"]
    classes = {k: v for k, v in src.items() if not str(k).endswith(CONFIDENCE_SUFFIX)}
    if len(classes) == 1:
        return next(iter(classes.items()))
    raise KeyError(f"raster_to_polygons: no 'AERIAL_LABEL-COSIA' entry among {sorted(src)}")


def _open_polygon_raster(src):
    if isinstance(src, (str, bytes, os.PathLike)):
        return open_raster(src)
    from flair_zonal_detection.geotiff import GeoTiffWriter
    if isinstance(src, GeoTiffWriter) or getattr(src, "mode", "r") != "r":  # an output raster: read the written file
        path = getattr(src, "path", None) or getattr(src, "name", None)
        if not getattr(src, "closed", False):
            raise ValueError(f"raster_to_polygons: {path} is still open for writing; close it first")
        return open_raster(path)
    return src


def min_pixels_for_area(min_area: float, pixel_area: float) -> int:
    """Smallest pixel count k with k * pixel_area >= min_area in float64: the components the reference keeps
    (it drops a polygon when poly.area < min_area)."""
    if not min_area > 0:
        return 1
    k = max(1, int(np.ceil(min_area / pixel_area)))
    while k > 1 and (k - 1) * pixel_area >= min_area:
        k -= 1
    while k * pixel_area < min_area:
        k += 1
    return k


def sieve_pixels_for_area(sieve_area, pixel_area: float) -> int:
    """The sieve's pixel threshold for ``sieve_area`` (map units squared): components of fewer pixels are small.
    0 (off) for an area of 0; a negative or non-finite area raises ValueError."""
    area = float(sieve_area)
    if not 0.0 <= area < float("inf"):
        raise ValueError(f"sieve_area must be a number >= 0, got {sieve_area!r}")
    return min_pixels_for_area(area, pixel_area) if area > 0 else 0


def _bounds4(raster):
    b = raster.bounds
    return tuple(float(v) for v in ((b.left, b.bottom, b.right, b.top) if hasattr(b, "left") else tuple(b)[:4]))


def _confidence_source(tiff_path, confidence):
    """The raster behind raster_to_polygons' ``confidence`` argument: True = the f"{task}_confidence" entry of the
    outputs dict passed as ``tiff_path``; else a raster / path / writer like ``tiff_path`` itself."""
    if confidence is True:
        if not isinstance(tiff_path, dict):
            raise ValueError("raster_to_polygons: confidence=True needs the outputs dict of a write_confidence run")
        key = _class_entry(tiff_path)[0] + CONFIDENCE_SUFFIX
        if key not in tiff_path:
            raise KeyError(f"raster_to_polygons: no {key!r} entry among {sorted(tiff_path)} (write_confidence off?)")
        confidence = tiff_path[key]
    elif isinstance(confidence, dict):
        raise ValueError("raster_to_polygons: confidence must be True, a raster or a path, not a dict")
    return _open_polygon_raster(confidence)


def _polygon_table(data: np.ndarray, conf: Optional[np.ndarray], left: float, top: float, xres: float, yres: float,
                   crs, bg: Optional[int], min_pixels: int, simplification: float, n_jobs: Optional[int],
                   zone=None, classes=None, zone_crs=None, target_crs=None, sieve_pixels: int = 0,
                   workspace: str = "auto", compare=None, compare_iou: float = 0.5, compare_classes: str = "same",
                   compare_sink: Optional[dict] = None):
    """Shared tail of raster_to_polygons / rasters_to_polygons / vectorize_segmentation_parallel: on the device copy
    of the raster the
    sieve (ops.sieve_, only when ``sieve_pixels`` > 1), then zone clip and class filter (one ffa_zone_clip_u8 pass,
    only when asked for), GPU polygonisation (+ zonal sums of the
    uint8 confidence plane), map coordinates, host simplification, reprojection of the kept vertices to
    ``target_crs`` (one ffa_crs_transform_f64 pass, only when asked for), frame.  ``data`` / ``conf`` are host arrays,
    or device tensors this call may change (the mosaic of rasters_to_polygons).  ``workspace``: "bound"
    (ops.polygonize), "counted" (ops.polygonize_counted) or "auto" = bound where 4 * H * W < 2^31, else counted.
    ``compare``: None, or what _compare_source returned -- a reference class band (host array) or ("zone", geometry);
    the four object-matching columns of _compare_columns then follow the others (``compare_sink``: a dict that
    receives the reference's side of the matching, for compare.compare_objects)."""
    from flair_zonal_detection.polygons import FlatPolygons, PolygonFrame
    if workspace not in ("auto", "bound", "counted"):
        raise ValueError(f"raster_to_polygons: workspace must be 'auto', 'bound' or 'counted', got {workspace!r}")
    if workspace == "auto":
        workspace = "bound" if 4 * int(data.shape[0]) * int(data.shape[1]) < 1 << 31 else "counted"
    polygonize = ops.polygonize if workspace == "bound" else ops.polygonize_counted
    dev = torch.device("cuda")
    if torch.is_tensor(data):
        cls_dev, values = data, conf
    else:
        values = None if conf is None else torch.from_numpy(np.ascontiguousarray(conf)).to(dev)
        cls_dev = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    if sieve_pixels > 1:
        stats = ops.sieve_(cls_dev, int(sieve_pixels), background=bg)
        logger.info("sieve: %d regions (%d pixels) below %d pixels merged into a neighbour in %d rounds, %d remain",
                    stats["relabelled_components"], stats["relabelled_pixels"], int(sieve_pixels), stats["rounds"],
                    stats["remaining_small"])
    if zone is not None or classes is not None:
        keep = None if classes is None else sorted({int(c) for c in classes})
        if keep is not None and not all(0 <= c <= 255 for c in keep):
            raise ValueError(f"raster_to_polygons: class ids must be uint8 values, got {keep}")
        if bg is None:
            # every value is a class, so there is no background to reuse: 255 stands in, unless the raster needs it
            bg = 255
            if (keep is None or 255 in keep) and bool((data == 255).any()):
                raise ValueError("raster_to_polygons: with ignore_background=False the zone / class filter uses 255 as "
                                 "the fill value, but the raster holds 255 in a kept class")
        mask = None
        if zone is not None:
            from flair_zonal_detection.zone import zone_mask
            mask = zone_mask(zone, left, top, xres, yres, data.shape[0], data.shape[1], zone_crs=zone_crs,
                             raster_crs=crs)
        ops.zone_clip_(cls_dev, mask, keep_classes=keep, fill=bg)
    else:
        mask = keep = None
    compare_columns = None
    if compare is not None:
        compare_columns = _compare_columns(cls_dev, compare, bg, min_pixels, mask, keep, (left, top, xres, yres), crs,
                                           zone_crs, compare_iou, compare_classes, compare_sink)
    res = [t.cpu().numpy() for t in polygonize(cls_dev, bg, min_pixels,
                                               **({} if values is None else {"values": values}))]
    pc, pix, pro, rvo, verts = res[:5]
    xy = np.empty(verts.shape, dtype=np.float64)
    xy[:, 0] = left + verts[:, 0] * xres
    xy[:, 1] = top - verts[:, 1] * yres
    if simplification and simplification > 0 and len(pc):
        threads = max(1, min(16, int(n_jobs) if n_jobs else (os.cpu_count() or 1)))
        keep = ops.polygon_simplify(xy, rvo, pro, float(simplification), threads)
        kept_before = np.concatenate([[0], np.cumsum(keep)])
        rvo = kept_before[rvo].astype(np.int32)
        xy = xy[keep]
    if target_crs is not None:
        from flair_zonal_detection import crs as crs_table
        if not isinstance(crs, crs_table.CrsParams) and crs_table.epsg_code(crs) is None:
            raise ValueError(f"raster_to_polygons: target_crs needs a raster with a recognisable CRS, got {crs!r}")
        dst = crs_table.parse(target_crs)
        if not crs_table.same(crs, dst):
            xy = ops.reproject_points(np.ascontiguousarray(xy), crs, dst)
            crs = str(dst)
    flat = FlatPolygons(pc.astype(np.int32), pro.astype(np.int32), rvo.astype(np.int32), xy)
    columns = {}
    if conf is not None:
        pixels = pix.astype(np.int64)
        # exact integer sum / (255 * pixel count), one float64 division per polygon: a number in [0, 1]
        columns = {"confidence": res[5].astype(np.int64) / (255.0 * pixels), "pixels": pixels}
    if compare_columns is not None:
        if len(compare_columns["matched"]) != len(pc):
            raise RuntimeError(f"raster_to_polygons: {len(compare_columns['matched'])} regions matched, {len(pc)} "
                               "polygons emitted")
        columns = {**columns, **compare_columns}
    try:
        import geopandas as gpd  # type: ignore
        from shapely.geometry import Polygon as ShapelyPolygon  # type: ignore
    except ImportError:
        return PolygonFrame.from_flat(flat, crs, **({"columns": columns} if columns else {}))
    geoms = [ShapelyPolygon(r[0], r[1:]) for r in (flat.rings(q) for q in range(len(flat)))]
    return gpd.GeoDataFrame({"class_id": flat.class_id.astype(np.int64), **columns, "geometry": geoms}, crs=crs)


def _compare_is_zone(compare) -> bool:
    """whether raster_to_polygons' ``compare`` is a geometry (anything zone.zone_rings reads) and not a class raster"""
    if hasattr(compare, "__geo_interface__"):
        return True
    if isinstance(compare, dict):
        return "type" in compare  # GeoJSON; an outputs dict has task names for keys
    if isinstance(compare, (str, os.PathLike)):
        return str(os.fspath(compare)).lower().endswith((".geojson", ".json"))
    return isinstance(compare, (list, tuple))


def _compare_source(compare, shape, bounds, res, name: str):
    """What _polygon_table takes as ``compare``: ("zone", geometry), or the one uint8 band of the reference class
    raster ``compare`` (path, raster object, outputs dict or closed writer), which must have the prediction's
    ``shape``, ``bounds`` (left, bottom, right, top; to within 1e-6 of a pixel) and ``res``, else ValueError starting
    with ``name``."""
    if _compare_is_zone(compare):
        return ("zone", compare)
    csrc = _polygon_source(compare)
    if csrc.count != 1:
        raise ValueError(f"{name}: the compare raster must have one band, got {csrc.count}")
    ref = np.asarray(csrc.read(1))
    if ref.dtype != np.uint8:
        raise ValueError(f"{name}: uint8 compare raster expected, got {ref.dtype}")
    if ref.shape != tuple(shape):
        raise ValueError(f"{name}: compare raster is {ref.shape}, the class raster {tuple(shape)}")
    cres, cbounds = tuple(float(v) for v in csrc.res), _bounds4(csrc)
    tol = 1e-6 * max(float(v) for v in res)
    if cres != tuple(float(v) for v in res) or any(abs(a - b) > tol for a, b in zip(cbounds, bounds)):
        raise ValueError(f"{name}: the compare raster's bounds / resolution differ from the class raster's "
                         f"({cbounds}, {cres} vs {tuple(bounds)}, {tuple(res)})")
    return ref


def _compare_regions(cls_dev, compare, bg, min_pixels, mask, keep, grid, crs, zone_crs, compare_classes):
    """(ops.RegionOverlaps of the class plane against the reference, compare_classes in force).  The reference raster
    gets the zone clip and class filter the class plane got; a geometry becomes one "known" class (1 inside, 0 =
    background outside), clipped to the zone, and is compared with ``classes="any"``."""
    dev = cls_dev.device
    if isinstance(compare, tuple):
        from flair_zonal_detection.zone import zone_mask
        left, top, xres, yres = grid
        ref = zone_mask(compare[1], left, top, xres, yres, cls_dev.shape[0], cls_dev.shape[1], zone_crs=zone_crs,
                        raster_crs=crs).clone()
        if mask is not None:
            ref.mul_(mask)
        return ops.region_overlaps(cls_dev, ref, bg, 0, min_pixels, min_pixels), "any"
    ref = torch.from_numpy(np.ascontiguousarray(compare)).to(dev)
    if mask is not None or keep is not None:
        ops.zone_clip_(ref, mask, keep_classes=keep, fill=bg)
    return ops.region_overlaps(cls_dev, ref, bg, bg, min_pixels, min_pixels), compare_classes


def _class_order(cls: np.ndarray):
    """(order, rank): the stable sort by class that puts a region table into polygon order, and its inverse"""
    order = np.argsort(cls, kind="stable")
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return order, rank


def _compare_frames_data(ov, compare_iou, compare_classes):
    """object matching of a RegionOverlaps with both sides in polygon order: (columns of the prediction's polygons,
    columns of the reference's regions, the host matching)"""
    from flairhip import objects
    m = objects.match_objects(ov, float(compare_iou), compare_classes)
    order_a, rank_a = _class_order(ov.a_class.cpu().numpy())
    order_b, rank_b = _class_order(ov.b_class.cpu().numpy())
    hit_a, hit_b = m.a_match >= 0, m.b_match >= 0
    ref_id = np.where(hit_a, rank_b[np.where(hit_a, m.a_match, 0)] if len(rank_b) else -1, -1).astype(np.int64)
    pred_id = np.where(hit_b, rank_a[np.where(hit_b, m.b_match, 0)] if len(rank_a) else -1, -1).astype(np.int64)
    pred = {"match_iou": m.a_match_iou[order_a], "matched": hit_a[order_a].astype(np.int64), "ref_id": ref_id[order_a],
            "ref_fraction": m.a_covered[order_a]}
    ref = {"match_iou": m.b_match_iou[order_b], "matched": hit_b[order_b].astype(np.int64), "pred_id": pred_id[order_b]}
    return pred, ref, m


def _compare_columns(cls_dev, compare, bg, min_pixels, mask, keep, grid, crs, zone_crs, compare_iou, compare_classes,
                     sink=None):
    """the four columns raster_to_polygons(compare=...) adds, in polygon order"""
    ov, mode = _compare_regions(cls_dev, compare, bg, min_pixels, mask, keep, grid, crs, zone_crs, compare_classes)
    pred, ref, m = _compare_frames_data(ov, compare_iou, mode)
    if sink is not None:
        sink.update(ref=ref, overlaps=ov, matches=m, classes=mode)
    return pred


def _class_band(src, name: str, shape=None):
    """The one uint8 band of a class raster (``shape``: the (h, w) its bounds and resolution give, when known);
    ValueError messages start with ``name``."""
    if src.count != 1:
        raise ValueError(f"{name}: a one-band class raster (argmax output) expected, got {src.count} bands")
    data = np.asarray(src.read(1))
    if data.dtype != np.uint8:
        raise ValueError(f"{name}: uint8 class raster expected, got {data.dtype}")
    if shape is not None and data.shape != tuple(shape):
        raise ValueError(f"{name}: {data.shape} pixels, but its bounds and resolution give {tuple(shape)}")
    return data


def _confidence_band(csrc, src, data, name: str):
    """The one uint8 band of the confidence raster ``csrc`` of the class raster ``src`` with band ``data``: same
    shape, bounds and resolution, else ValueError starting with ``name``."""
    if csrc.count != 1:
        raise ValueError(f"{name}: the confidence raster must have one band, got {csrc.count}")
    conf = np.asarray(csrc.read(1))
    if conf.dtype != np.uint8:
        raise ValueError(f"{name}: uint8 confidence raster expected, got {conf.dtype}")
    if conf.shape != data.shape:
        raise ValueError(f"{name}: confidence raster is {conf.shape}, the class raster {data.shape}")
    res, cres = tuple(float(v) for v in src.res), tuple(float(v) for v in csrc.res)
    if cres != res or _bounds4(csrc) != _bounds4(src):
        raise ValueError(f"{name}: the confidence raster's bounds / resolution differ from the class raster's "
                         f"({_bounds4(csrc)}, {cres} vs {_bounds4(src)}, {res})")
    return conf


def _background(ignore_background: bool, background_value):
    """the polygoniser's background: ``background_value`` when it is to be ignored and a uint8 pixel can hold it,
    else None = every value is a class"""
    bg = int(background_value) if ignore_background else None
    return bg if bg is not None and 0 <= bg <= 255 else None


def raster_to_polygons(tiff_path, ignore_background: bool = True, background_value: int = 18, min_area: float = 1.0,
                       simplification: float = 0.1, n_jobs: Optional[int] = None, confidence=None, zone=None,
                       classes=None, zone_crs=None, target_crs=None, sieve_area: float = 0.0,
                       workspace: str = "auto", compare=None, compare_iou: float = 0.5, compare_classes: str = "same",
                       _compare_sink: Optional[dict] = None):
    """Vector polygons of a class raster -- the reference's raster_to_polygons (inference.py:377-413) with its
    signature and call form ``raster_to_polygons(output_files, n_jobs=4)``.

    One polygon per 4-connected component of equal value (what rasterio.features.shapes(mask, mask=mask,
    connectivity=4) yields per class); every value except ``background_value`` (when ``ignore_background``) is a
    class -- 0 in never-written areas included, a reference quirk kept on purpose.  A polygon is dropped when its
    unsimplified area, pixel count * |xres * yres| in float64, is below ``min_area``; the reference computes that area
    with GEOS's shoelace on absolute coordinates, which can differ only for areas equal to min_area to within about
    1e-9 relative.  Map coordinates are left + col * xres, top - row * yres in float64 (north-up rasters only).  With
    ``simplification`` > 0 each polygon is simplified like shapely's simplify(tol, preserve_topology=True)
    (csrc/polygon_simplify.cpp; not vertex-for-vertex identical to GEOS).  ``n_jobs`` bounds the simplifier's host
    threads (at most 16).  Labelling and ring assembly run on the GPU (ops.polygonize).

    Returns a GeoDataFrame(class_id, geometry, crs) when geopandas and shapely are importable, else a
    polygons.PolygonFrame with the same columns, ``crs`` and ``to_file(path, driver="GPKG")``.  Polygons come in
    (class, first pixel) order, which the reference's process pool does not fix.  Multi-band rasters (class_prob
    outputs) raise ValueError -- the reference would silently polygonise band 1.

    ``confidence``: None (the columns above), a confidence raster (path, raster object or closed writer; one band,
    uint8, the class raster's shape, bounds and resolution, else ValueError) or True = the f"{task}_confidence" entry
    of the outputs dict a ``write_confidence`` run returned.  Two columns then follow ``class_id``: ``confidence``
    (float64) = sum of the raster's values over the polygon's pixels / (255.0 * pixels), the mean over the polygon of
    the winning class's softmax probability as the uint8 raster holds it, and ``pixels`` (int64), the unsimplified
    pixel count that mean was taken over.  The sums are exact integers taken on the GPU
    (ffa_polygonize_zonal_sum_u8), so equal rasters give equal columns; geometry, order and class_id do not depend on
    ``confidence``.

    ``zone``: a geozone in the raster's CRS (any form zone.zone_rings reads: GeoJSON dict or file, objects with
    ``__geo_interface__``, bounds, sequences of those).  It is rasterised on the class raster's own grid -- a pixel
    belongs to the zone when its centre is inside the contour, as rasterio.mask.mask means it -- and pixels outside
    take the background value before polygonisation: the fork's ``intersection(contour_union)`` to within half a
    pixel, with integer vertices and valid rings kept.  ``classes``: an iterable of class ids; only those are
    polygonised (the fork's ``class_id == 6`` filter).  Both are one pass on the GPU copy of the raster
    (ffa_zone_clip_u8); the confidence sums need no change since background pixels contribute nowhere.  With
    ``ignore_background=False`` there is no background value to reuse: 255 is the fill, and a raster that holds 255
    in a kept class raises ValueError.  With ``zone=None, classes=None`` nothing changes.

    ``zone_crs``: the CRS the zone is given in (anything crs.parse accepts, or "auto" for GeoJSON: the legacy ``crs``
    member, else EPSG:4326); the zone is reprojected to the raster's CRS before it is rasterised.  None: the zone is in
    the raster's CRS.  ``target_crs``: the CRS of the result (the driver's ``clean_results_gdf.to_crs(target_crs)``).
    The order is the driver's: polygonise, ``min_area`` and simplification in the raster's CRS, then the kept vertices
    through one pass of the GPU transform (ops.reproject_points; edges stay straight, as to_crs leaves them) and the
    frame's ``crs`` is the target.  class_id, confidence, pixels, polygon order and ring structure do not depend on
    ``target_crs``.  Either argument with a raster whose CRS is unknown raises ValueError; None changes nothing.

    ``sieve_area`` (map units squared, default 0 = off): regions -- 4-connected components of equal class -- whose
    area, pixel count * |xres * yres|, is below it are merged into their largest neighbour on the device copy of the
    class plane (ops.sieve_; gdal_sieve's job) BEFORE the zone clip, the class filter and polygonisation.  ``min_area``
    drops a small polygon and leaves its footprint as a hole of the polygon around it; the sieve makes a noise pixel of
    class 3 inside a class-6 roof class 6, so it leaves no hole once ``classes=[6]`` is applied.  The area converts
    to pixels as ``min_area`` does (min_pixels_for_area); ``ignore_background`` / ``background_value`` mean what they
    mean for the polygoniser: background pixels never change and are never merged into.  The confidence raster is not
    touched: a relabelled pixel contributes its own stored confidence to the polygon it joined.  The input raster is
    not modified.  0 takes the code path without the sieve, with no new call.

    ``workspace``: how the polygoniser's device workspace is sized.  "bound" is ops.polygonize: 184 bytes per pixel
    whatever the raster holds, rasters of 4 * H * W < 2^31 (about 536 Mpx) only.  "counted" is
    ops.polygonize_counted: 16 bytes per pixel, then about 42 bytes per boundary edge once the edges are counted, one
    host synchronisation more, rasters of H * W < 2^30 -- a 25 000 x 25 000 BD ORTHO dalle included.  Both give the
    same polygons, byte for byte.  "auto" (the default) is "bound" wherever it can run, else "counted", so no call
    that worked before changes.  ``sieve_area`` > 0 on a raster beyond 4 * H * W < 2^31 still raises from ops.sieve_,
    whose limit is its own, as a ``zone`` does from the zone mask's.

    ``compare``: None, or a reference to match the polygons against as objects (flairhip/objects.py).  A class raster
    (path, raster object or closed writer; one band, uint8, the class raster's shape, bounds and resolution, else
    ValueError): the ground truth, or last run's prediction.  It gets the same zone clip and class filter, the same
    background and ``min_area``; its regions are numbered in (class, first pixel) order like the polygons.  Or a
    geometry (anything zone.zone_rings reads, in ``zone_crs`` like the zone): a layer of known objects, rasterised
    with zone.zone_mask into one "known" class -- each feature filled even-odd over its rings (ffa_zone_mask_u8) and
    the features united, so overlapping and touching features merge into one region -- and ``compare_classes`` is
    then "any".  The regions of both are overlapped on the GPU (ops.region_overlaps, after the sieve, the zone clip
    and the class filter) and matched one to one, greedily by descending IoU, a pair counting when its IoU >=
    ``compare_iou`` and, with ``compare_classes="same"`` (not "any"), its classes agree.  Four columns follow the
    others: ``match_iou`` (float64, 0.0 without a match), ``matched`` (int64, 0 or 1), ``ref_id`` (int64, index of the
    matched reference region, or -1) and ``ref_fraction`` (float64, the share of the polygon's pixels that reference
    regions cover -- of the same class with "same").  Geometry, order, class_id, confidence and pixels do not depend
    on ``compare``; None makes no new call.
    """
    if compare_classes not in ("same", "any"):
        raise ValueError(f"raster_to_polygons: compare_classes must be 'same' or 'any', got {compare_classes!r}")
    src = _polygon_source(tiff_path)
    data = _class_band(src, "raster_to_polygons")
    xres, yres = (float(v) for v in src.res)
    left, _, _, top = _bounds4(src)
    conf = None
    if confidence is not None and confidence is not False:
        conf = _confidence_band(_confidence_source(tiff_path, confidence), src, data, "raster_to_polygons")
    min_pixels = min_pixels_for_area(float(min_area), abs(xres * yres))
    bg = _background(ignore_background, background_value)
    if compare is not None:
        compare = _compare_source(compare, data.shape, _bounds4(src), (xres, yres), "raster_to_polygons")
    return _polygon_table(data, conf, left, top, xres, yres, getattr(src, "crs", None), bg, min_pixels, simplification,
                          n_jobs, zone=zone, classes=classes, zone_crs=zone_crs, target_crs=target_crs,
                          sieve_pixels=sieve_pixels_for_area(sieve_area, abs(xres * yres)), workspace=workspace,
                          compare=compare, compare_iou=compare_iou, compare_classes=compare_classes,
                          compare_sink=_compare_sink)


def mosaic_grid(bounds_list, res, names=None):
    """The common pixel grid of rasters with bounds (left, bottom, right, top) and one resolution ``res`` = (xres,
    yres): ``(H, W, left, top, [(row0, col0, h, w), ...])``, the union's size and origin and each raster's window in
    it, in input order.  Host arithmetic only.  Every origin must differ from the first raster's by whole pixels to
    within 1e-6 of a pixel, every extent must be a whole number of pixels, no two windows may share a pixel and the
    union must hold fewer than 2^30 pixels; else ValueError naming the source (``names[i]``, default "source i").
    The origin returned is the ``left`` of the first leftmost raster and the ``top`` of the first topmost one as
    they stand, not a sum that could round: a mosaic's map coordinates are bit for bit those of one raster with that
    origin."""
    xres, yres = (float(v) for v in res)
    if not (xres > 0 and yres > 0):
        raise ValueError(f"mosaic_grid: resolution {res!r} must be positive")
    bounds_list = [tuple(float(v) for v in b) for b in bounds_list]
    if not bounds_list:
        raise ValueError("mosaic_grid: no sources")
    names = [f"source {i}" for i in range(len(bounds_list))] if names is None else [str(n) for n in names]
    left0, _, _, top0 = bounds_list[0]

    def whole(v, what, name):
        k = round(v)
        if abs(v - k) > 1e-6:
            raise ValueError(f"mosaic_grid: {name}: {what} is {v!r} pixels, not a whole number (within 1e-6)")
        return int(k)

    wins = []
    for name, (l, b, r, t) in zip(names, bounds_list):
        c0 = whole((l - left0) / xres, "the origin's x offset from the first source", name)
        r0 = whole((top0 - t) / yres, "the origin's y offset from the first source", name)
        w = whole((r - l) / xres, "the width", name)
        h = whole((t - b) / yres, "the height", name)
        if h < 1 or w < 1:
            raise ValueError(f"mosaic_grid: {name}: empty extent {h} x {w}")
        wins.append((r0, c0, h, w))
    rmin, cmin = min(w[0] for w in wins), min(w[1] for w in wins)
    H = max(w[0] + w[2] for w in wins) - rmin
    W = max(w[1] + w[3] for w in wins) - cmin
    if H * W >= 1 << 30:
        raise ValueError(f"mosaic_grid: the mosaic of {len(wins)} sources is {H} x {W} pixels, beyond the limit "
                         f"H * W < 2^30 (its last source: {names[-1]})")
    wins = [(r0 - rmin, c0 - cmin, h, w) for r0, c0, h, w in wins]
    order = sorted(range(len(wins)), key=lambda i: wins[i])
    for n, i in enumerate(order):  # sorted by first row: only windows that start before this one ends can meet it
        r0, c0, h, w = wins[i]
        for j in order[n + 1:]:
            s0, d0, g, v = wins[j]
            if s0 >= r0 + h:
                break
            if d0 < c0 + w and c0 < d0 + v:
                raise ValueError(f"mosaic_grid: {names[j]} and {names[i]} share pixels (windows {wins[j]} and "
                                 f"{wins[i]} as (row0, col0, h, w))")
    left = next(b[0] for b, w in zip(bounds_list, wins) if w[1] == 0)
    top = next(b[3] for b, w in zip(bounds_list, wins) if w[0] == 0)
    return H, W, left, top, wins


def _same_crs(a, b) -> bool:
    if a is None or b is None:
        return a is None and b is None
    from flair_zonal_detection import crs as crs_table
    ca, cb = crs_table.epsg_code(a), crs_table.epsg_code(b)
    return ca == cb if ca is not None and cb is not None else str(a) == str(b)


def rasters_to_polygons(sources, confidence=None, ignore_background: bool = True, background_value: int = 18,
                        min_area: float = 1.0, simplification: float = 0.1, n_jobs: Optional[int] = None, zone=None,
                        classes=None, zone_crs=None, target_crs=None, sieve_area: float = 0.0,
                        workspace: str = "auto", compare=None, compare_iou: float = 0.5, compare_classes: str = "same"):
    """``raster_to_polygons`` of several rasters of one grid as ONE raster: an object lying across two dalles comes
    out as one polygon with its whole pixel count and one confidence, where polygonising each raster on its own and
    concatenating the frames (the driver's loop) cuts it at the seam and lets ``min_area`` drop the halves.

    ``sources``: a sequence of anything raster_to_polygons accepts (outputs dicts, paths, raster objects), in any
    order.  ``confidence``: None, True (each outputs dict's own confidence entry) or a sequence of confidence rasters
    of the same length.  The other keywords mean what they mean for raster_to_polygons.  All sources must be one-band
    uint8 rasters of one resolution and CRS whose origins differ by whole pixels (within 1e-6 of a pixel), and no two
    may share a pixel; the mosaic must hold fewer than 2^30 pixels: each violation is a ValueError naming the source.
    Pixels of the union's bounding box that no source covers take ``background_value``, which needs
    ``ignore_background=True`` (ValueError otherwise), and confidence 0, which no polygon sees.

    The mosaic is assembled on the device -- a uint8 plane filled with the background, each source uploaded once and
    copied into its window -- and goes through raster_to_polygons' own tail with the mosaic's origin: the result
    equals raster_to_polygons of a single raster holding the same pixels.  ``compare``: as for raster_to_polygons; a
    reference raster must cover the mosaic's grid (its shape, bounds and resolution)."""
    if compare_classes not in ("same", "any"):
        raise ValueError(f"rasters_to_polygons: compare_classes must be 'same' or 'any', got {compare_classes!r}")
    sources = list(sources)
    if not sources:
        raise ValueError("rasters_to_polygons: no sources")
    if confidence is None or confidence is False:
        conf_args = [None] * len(sources)
    elif confidence is True:
        conf_args = [True] * len(sources)
    else:
        conf_args = list(confidence)
        if len(conf_args) != len(sources):
            raise ValueError(f"rasters_to_polygons: {len(conf_args)} confidence rasters for {len(sources)} sources")
        missing = [i for i, c in enumerate(conf_args) if c is None]
        if missing and len(missing) != len(conf_args):
            raise ValueError(f"rasters_to_polygons: source {missing[0]} has no confidence raster, others have one")
    rasters, names = [], []
    for i, s in enumerate(sources):
        src = _polygon_source(s)
        name = f"source {i} ({getattr(src, 'path', None) or getattr(src, 'name', None) or type(src).__name__})"
        if src.count != 1:
            raise ValueError(f"rasters_to_polygons: {name}: a one-band class raster expected, got {src.count} bands")
        if rasters and tuple(float(v) for v in src.res) != tuple(float(v) for v in rasters[0].res):
            raise ValueError(f"rasters_to_polygons: {name}: resolution {tuple(src.res)} differs from the first "
                             f"source's {tuple(rasters[0].res)}")
        if rasters and not _same_crs(getattr(src, "crs", None), getattr(rasters[0], "crs", None)):
            raise ValueError(f"rasters_to_polygons: {name}: CRS {getattr(src, 'crs', None)!r} differs from the first "
                             f"source's {getattr(rasters[0], 'crs', None)!r}")
        rasters.append(src)
        names.append(name)
    xres, yres = (float(v) for v in rasters[0].res)
    H, W, left, top, wins = mosaic_grid([_bounds4(r) for r in rasters], (xres, yres), names)
    bg = _background(ignore_background, background_value)
    covered = sum(h * w for _, _, h, w in wins)
    if covered != H * W and bg is None:
        raise ValueError(f"rasters_to_polygons: the {len(rasters)} sources leave {H * W - covered} pixels of their "
                         f"{H} x {W} bounding box uncovered (first gap next to {names[0]}); filling a gap needs "
                         "ignore_background=True and a uint8 background_value")
    dev = torch.device("cuda")
    plane = torch.full((H, W), bg if bg is not None else 0, dtype=torch.uint8, device=dev)
    cplane = torch.zeros((H, W), dtype=torch.uint8, device=dev) if conf_args[0] is not None else None
    for s, src, name, carg, (r0, c0, h, w) in zip(sources, rasters, names, conf_args, wins):
        data = _class_band(src, f"rasters_to_polygons: {name}", (h, w))
        plane[r0:r0 + h, c0:c0 + w] = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
        if cplane is None:
            continue
        if carg is None:
            raise ValueError(f"rasters_to_polygons: {name}: no confidence raster, the other sources have one")
        conf = _confidence_band(_confidence_source(s, carg), src, data, f"rasters_to_polygons: {name}")
        cplane[r0:r0 + h, c0:c0 + w] = torch.from_numpy(np.ascontiguousarray(conf)).to(dev)
    min_pixels = min_pixels_for_area(float(min_area), abs(xres * yres))
    if compare is not None:
        compare = _compare_source(compare, (H, W), (left, top - H * yres, left + W * xres, top), (xres, yres),
                                  "rasters_to_polygons")
    return _polygon_table(plane, cplane, left, top, xres, yres, getattr(rasters[0], "crs", None), bg, min_pixels,
                          simplification, n_jobs, zone=zone, classes=classes, zone_crs=zone_crs, target_crs=target_crs,
                          sieve_pixels=sieve_pixels_for_area(sieve_area, abs(xres * yres)), workspace=workspace,
                          compare=compare, compare_iou=compare_iou, compare_classes=compare_classes)


def logits_to_labels_and_confidence(probs):
    """The reference's helper of the same name (inference.py:566-572): per-class scores [K, H, W] (numpy or torch,
    any real dtype) -> (uint8 labels = argmax over K, first maximum; confidence = max over K in the input's dtype).
    Thin and off the hot path: the tile loop gets both planes from ffa_predict_u8 mode 2 instead."""
    if torch.is_tensor(probs):
        probs = probs.detach().cpu().numpy()
    probs = np.asarray(probs)
    if probs.ndim != 3 or probs.shape[0] < 1:
        raise ValueError(f"logits_to_labels_and_confidence: a [K, H, W] array expected, got shape {probs.shape}")
    if probs.shape[0] > 256:
        raise ValueError(f"logits_to_labels_and_confidence: {probs.shape[0]} classes do not fit uint8 labels")
    return probs.argmax(axis=0).astype(np.uint8), probs.max(axis=0)


def _affine6(transform):
    """(a, b, c, d, e, f) of an affine object with .a .. .f or of a 6-tuple: x = a col + b row + c, y = d col + e row + f"""
    if all(hasattr(transform, n) for n in "abcdef"):
        t = tuple(float(getattr(transform, n)) for n in "abcdef")
    else:
        try:
            t = tuple(float(v) for v in transform)
        except TypeError:
            raise ValueError("vectorize_segmentation_parallel: transform must be an affine object or a 6-tuple") from None
        if len(t) != 6:
            raise ValueError(f"vectorize_segmentation_parallel: a 6-tuple (a, b, c, d, e, f) expected, got {len(t)} values")
    a, b, c, d, e, f = t
    if b != 0.0 or d != 0.0 or not a > 0.0 or not e < 0.0:
        raise ValueError(f"vectorize_segmentation_parallel: north-up transforms only (b = d = 0, a > 0, e < 0), got {t}")
    return t


def quantize_confidence(confidence) -> np.ndarray:
    """uint8 confidence plane: uint8 input as it is (value / 255 is the probability), float input in [0, 1] as
    rint(255 c) -- the quantisation the tile loop's confidence raster has."""
    if torch.is_tensor(confidence):
        confidence = confidence.detach().cpu().numpy()
    confidence = np.asarray(confidence)
    if confidence.dtype == np.uint8:
        return confidence
    if confidence.dtype.kind != "f":
        raise ValueError(f"confidence must be uint8 or float in [0, 1], got {confidence.dtype}")
    if not np.all((confidence >= 0.0) & (confidence <= 1.0)):  # NaN fails both comparisons
        raise ValueError("float confidence must lie in [0, 1]")
    return np.rint(255.0 * confidence.astype(np.float64)).astype(np.uint8)


def vectorize_segmentation_parallel(labels, confidence, transform, n_jobs: int = 4, simplification_tolerance: float = 1.0,
                                    min_area: float = 4.0, crs="EPSG:5490"):
    """The reference's vectorize_segmentation_parallel (inference.py:606-630) with its argument names and defaults:
    polygons of a label map [H, W] (uint8; class 0 is the background, :617-618) with the columns ``class_id``,
    ``confidence``, ``pixels`` and ``geometry`` (frame type as raster_to_polygons).

    ``confidence`` is uint8 (value / 255) or float in [0, 1]; float input is quantised with rint(255 c) first, so the
    result equals that of the uint8 raster the tile loop writes.  ``transform`` is an affine object with .a .. .f or
    the 6-tuple (a, b, c, d, e, f), north-up only.  ``n_jobs`` bounds the simplifier's host threads; the polygons of
    all classes come from one GPU pass, not from a process per class.

    One deliberate departure: the reference takes ``confidence[mask].mean()`` over ALL pixels of a class and gives
    every polygon of that class the same number (:590-598); here each polygon gets the mean over its own pixels.

    The signature is the reference's and stays so: clipping to a geozone, the class filter and the sieve are
    arguments of raster_to_polygons (``zone=``, ``classes=``, ``sieve_area=``)."""
    if torch.is_tensor(labels):
        labels = labels.detach().cpu().numpy()
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.dtype != np.uint8:
        raise ValueError(f"vectorize_segmentation_parallel: uint8 [H, W] labels expected, got {labels.dtype} "
                         f"{labels.shape}")
    conf = quantize_confidence(confidence)
    if conf.shape != labels.shape:
        raise ValueError(f"vectorize_segmentation_parallel: confidence is {conf.shape}, labels {labels.shape}")
    a, _, c, _, e, f = _affine6(transform)
    xres, yres = a, -e
    min_pixels = min_pixels_for_area(float(min_area), abs(xres * yres))
    return _polygon_table(labels, conf, c, f, xres, yres, crs, 0, min_pixels, simplification_tolerance, n_jobs)
