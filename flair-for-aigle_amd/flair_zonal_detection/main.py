"""Command-line entry of the zonal tile loop -- counterpart of the reference's flair_zonal_detection/main.py:8-14
(``python -m flair_zonal_detection.main --config <yaml>`` -> run_inference(config)).

Multi-GPU: the path shards by tiles with no collective.  Launched as one process per GPU,

    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m flair_zonal_detection.main --config zonal.yaml

every rank takes RANK / WORLD_SIZE / LOCAL_RANK from the environment, runs its contiguous slice of the tile grid on
its own GPU and writes ``<output>.r<rank>of<world>.tif`` (+ a one-band "written" mask); rank 0 then waits for the
part files of all ranks and joins them in rank order into the output the single-process run would have written
(``geotiff.merge_shard_files``: the reference's last-writer-wins for the clamped last row / column is preserved).
No process group is created: the only synchronisation is the appearance of the part files (each is renamed into
place when complete).
"""
from __future__ import annotations

import argparse
import logging
import os
import sys
import time
from typing import Dict, Optional

sys.path.append(os.path.abspath(os.path.join(os.path.dirname(__file__), "../")))

logger = logging.getLogger(__name__)


def _remove_stale_parts(outputs) -> None:
    """called by run_inference once the outputs exist, before the tile loop: drop this rank's leftovers"""
    from flair_zonal_detection.geotiff import WRITTEN_SUFFIX
    for o in outputs.values():
        path = getattr(o, "path", None)
        if path:
            for f in (path, path + WRITTEN_SUFFIX):
                if os.path.exists(f):
                    os.remove(f)


def _wait_for(paths, timeout_s: float, newer_than: float = 0.0) -> None:
    t0 = time.time()
    while True:
        missing = [p for p in paths if not (os.path.exists(p) and os.path.getmtime(p) >= newer_than)]
        if not missing:
            return
        if time.time() - t0 > timeout_s:
            raise TimeoutError(f"part files of other ranks did not appear within {timeout_s:.0f} s: {missing[:4]}")
        time.sleep(0.2)


def run_sharded(config, rank: int, world: int, timeout_s: float = 3600.0, keep_parts: bool = False, geozone=None,
                geozone_crs=None) -> Optional[Dict[str, str]]:
    """This rank's share of a zonal run over ``world`` processes (one per GPU).  Rank 0 returns {task: merged path}
    once every rank's part file exists; the other ranks return None as soon as their own part is written.
    ``geozone`` and ``geozone_crs`` are passed on to run_inference (every rank slices and filters the same tile
    grid)."""
    import torch
    from flair_zonal_detection.geotiff import WRITTEN_SUFFIX, GeoTiffWriter, merge_shard_files
    from flair_zonal_detection.inference import run_inference
    if torch.cuda.is_available():
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", rank)) % torch.cuda.device_count())
    # The only synchronisation between ranks is the appearance of part files, so files an earlier (crashed, or
    # --keep-parts) run left under the same names must not be mistaken for this run's: every rank removes its own
    # part + mask before it starts, and rank 0 only accepts parts at least as new as its own start.
    t_start = time.time()
    outputs = run_inference(config, geozone=geozone, shard=(rank, world), before_loop=_remove_stale_parts,
                            geozone_crs=geozone_crs)
    for task, o in outputs.items():
        if not isinstance(o, GeoTiffWriter):
            raise TypeError("a sharded multi-process run needs file outputs (GeoTIFF paths), not in-memory rasters")
    if rank != 0:
        return None
    merged = {}
    for task, o in outputs.items():
        mine = o.path  # <base>.r0of<world>.tif
        base = mine[:-len(f".r0of{world}.tif")]
        parts = [f"{base}.r{r}of{world}.tif" for r in range(world)]
        # the mask is written after its part file; ranks start together (torchrun), so a mask older than this
        # rank's start (minus a generous clock / start-up skew) is a leftover that its owner has not replaced yet
        _wait_for([p + WRITTEN_SUFFIX for p in parts], timeout_s, newer_than=t_start - 600.0)
        merged[task] = merge_shard_files(parts, base + ".tif")
        if not keep_parts:
            for p in parts:
                for f in (p, p + WRITTEN_SUFFIX):
                    os.remove(f)
        logger.info("merged %d part files into %s", world, merged[task])
    return merged


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Run zonal detection inference.")
    parser.add_argument("--config", type=str, required=True, help="Path to the detection config file")
    parser.add_argument("--keep-parts", action="store_true", help="sharded runs: keep the per-rank part files")
    parser.add_argument("--polygons", type=str, default=None, metavar="PATH.gpkg",
                        help="also polygonise the written class raster (raster_to_polygons with the reference's "
                             "defaults) and write the polygons as a GeoPackage, with the columns confidence and pixels "
                             "when the config sets write_confidence; sharded runs: rank 0, after the merge")
    parser.add_argument("--sieve-area", type=float, default=None, metavar="M2",
                        help="with --polygons: before polygonisation, merge regions of the class raster below this "
                             "area (map units squared) into their largest neighbour, so that speckle leaves neither "
                             "polygons nor holes.  Default: the config key sieve_area, else 0 (off)")
    parser.add_argument("--cog", action="store_true",
                        help="convert the written rasters to cloud-optimised GeoTIFFs (<name>_COG.tif: overview "
                             "pyramid, IFDs ahead of the data), as the config key cog_conversion: true does; overviews "
                             "by the config key cog_overview_resampling (nearest, mode or average)")
    parser.add_argument("--tta", type=str, default=None, choices=("none", "flips", "d4"),
                        help="test-time augmentation: predict every tile under the flips (4 views) or all flips and "
                             "rotations of the square (d4, 8 views) and average the class probabilities.  Default: the "
                             "config key tta, else none")
    parser.add_argument("--zone", type=str, default=None, metavar="PATH.geojson",
                        help="geozone contour (GeoJSON, in the raster's CRS unless --zone-crs says otherwise): only its "
                             "bounding box is sliced (and, with skip_tiles_outside_zone in the config, only the tiles "
                             "that hold a zone pixel are inferred); with --polygons the polygons are clipped to the "
                             "contour")
    parser.add_argument("--classes", type=str, default=None, metavar="ID[,ID...]",
                        help="with --polygons: polygonise these class ids only, e.g. 6,7")
    parser.add_argument("--zone-crs", type=str, default=None, metavar="EPSG:NNNN|auto",
                        help="CRS the --zone file is given in; it is reprojected to the raster's CRS first.  auto: the "
                             "GeoJSON's legacy crs member, else EPSG:4326 (RFC 7946).  Default: the config key "
                             "geozone_crs, else the raster's CRS (no reprojection)")
    parser.add_argument("--target-crs", type=str, default=None, metavar="EPSG:NNNN",
                        help="with --polygons: write the polygons in this CRS (e.g. EPSG:4326) instead of the raster's")
    parser.add_argument("--thresholds", type=str, default=None, metavar="FILE",
                        help="calibrated class thresholds (best_thresholds.yaml, written by flair_hub's calibrate "
                             "stage): a class takes a pixel only where its score reaches its threshold, the best "
                             "passing class wins, and a pixel no class passes at gets the fallback label.  Default: the "
                             "config key model_threshold_filepath, else none")
    parser.add_argument("--threshold-fallback", type=int, default=None, metavar="N",
                        help="the label (0..255) of a pixel at which no class reaches its threshold.  Default: the "
                             "config key threshold_fallback, else 18")
    parser.add_argument("--compare", type=str, default=None, metavar="PATH",
                        help="with --polygons: match the polygons as objects against a reference -- a class raster on "
                             "the prediction's grid (ground truth, or last run's output) or a GeoJSON layer of known "
                             "objects.  The GeoPackage gains the columns match_iou, matched, ref_id and ref_fraction, "
                             "and per-class object precision / recall / F1 go to <polygons stem>_objects.json.  "
                             "Default: the config key compare_raster, else none")
    parser.add_argument("--compare-iou", type=float, default=None, metavar="X",
                        help="the IoU from which a polygon and a reference object match.  Default: the config key "
                             "compare_iou, else 0.5")
    parser.add_argument("--compare-classes", type=str, default=None, choices=("same", "any"),
                        help="whether only objects of the same class may match.  Default: the config key "
                             "compare_classes, else same")
    parser.add_argument("--zone-stats", type=str, default=None, metavar="PATH.geojson",
                        help="a layer of zones (GeoJSON Features: parcels, communes, a grid): after the tile loop each "
                             "written class raster <name>.tif gets <name>_zone_stats.csv, the pixels and area of every "
                             "class in every zone, with the mean confidence when the config sets write_confidence.  "
                             "Default: the config key zone_stats, else none")
    parser.add_argument("--zone-stats-id", type=str, default=None, metavar="FIELD",
                        help="the Feature property that names a zone in the table.  Default: the config key "
                             "zone_stats_id, else the zone's index")
    parser.add_argument("--zone-stats-crs", type=str, default=None, metavar="EPSG:NNNN|auto",
                        help="CRS the --zone-stats layer is given in.  Default: the config key zone_stats_crs, else the "
                             "raster's CRS")
    parser.add_argument("--change-from", type=str, default=None, metavar="PATH",
                        help="the class raster of an earlier run on the same grid: after the tile loop each written "
                             "class raster <name>.tif gets <name>_zone_change.csv (per zone: changed pixels and area, "
                             "gain, loss and net per class) and <name>_zone_transitions.csv (per zone, from-class and "
                             "to-class), over the --zone-stats zones or the whole raster as one zone.  Default: the "
                             "config key change_from, else none")
    parser.add_argument("--change-polygons", type=str, default=None, metavar="OUT.gpkg",
                        help="with a change_from: write the regions that changed class as a GeoPackage (class_id = the "
                             "index of the transition, with from_class and to_class; -1 = any), honouring --zone, "
                             "--zone-crs, --target-crs and --sieve-area")
    parser.add_argument("--change-transitions", type=str, default=None, metavar="SPEC[,SPEC...]",
                        help="with a change_from: the transitions --change-polygons draws, FROM:TO with * for any "
                             "class, e.g. *:6,4:0; the earlier spec wins where two overlap.  Default: the config key "
                             "change_transitions, else *:k for every class k")
    return parser


def _write_object_summary(path: str, gdf, compare, compare_iou: float, sink: dict) -> str:
    """<polygons stem>_objects.json: the object scores of the run against the reference (compare.summary_of)"""
    import json
    from flair_zonal_detection.compare import summary_of
    summary = summary_of(sink, compare_iou)
    summary.update(compare=str(compare), polygons=int(len(gdf)))
    out = os.path.splitext(path)[0] + "_objects.json"
    with open(out, "w") as f:
        json.dump(summary, f, indent=2)
    return out


def _change_products(args, config, outputs, tables: bool) -> None:
    """what a run with a change_from writes outside run_inference: the change tables of a sharded run (``tables``;
    rank 0, over the merged rasters) and the --change-polygons GeoPackage"""
    from flair_zonal_detection.config import load_config, validate_change, validate_geozone_crs, validate_sieve_area
    from flair_zonal_detection.config import validate_zone_stats
    cfg = config if isinstance(config, dict) else load_config(config)
    change_from, transitions = validate_change(cfg)
    if change_from is None:
        return
    from flair_zonal_detection.inference import CONFIDENCE_SUFFIX, change_source, write_change_stats
    if tables:
        write_change_stats(outputs, cfg, change_from, *validate_zone_stats(cfg))
    if not args.change_polygons:
        return
    from flair_zonal_detection.change import change_polygons, transition_specs, write_change_polygons
    class_keys = [k for k in outputs if not str(k).endswith(CONFIDENCE_SUFFIX)]
    if len(class_keys) != 1:
        raise ValueError(f"--change-polygons draws one class raster, the run wrote {len(class_keys)}")
    key = class_keys[0]
    before = change_source(change_from, key, class_keys)
    if before is None:
        raise ValueError(f"--change-polygons: change_from lists no earlier raster for {key}")
    names = {t["name"]: t.get("class_names") for t in cfg.get("tasks", [])}.get(key) or None
    zone_crs = args.zone_crs
    if zone_crs is None and args.zone is not None:
        zone_crs = validate_geozone_crs(cfg)
    sieve_area = args.sieve_area if args.sieve_area is not None else validate_sieve_area(cfg)
    pair = {key: outputs[key]}
    with_conf = key + CONFIDENCE_SUFFIX in outputs
    if with_conf:
        pair[key + CONFIDENCE_SUFFIX] = outputs[key + CONFIDENCE_SUFFIX]
    extra = {k: v for k, v in (("zone", args.zone), ("zone_crs", zone_crs), ("target_crs", args.target_crs),
                               ("sieve_area", sieve_area or None)) if v is not None}
    specs = transition_specs(transitions, class_names=names)
    frame = change_polygons(before, pair, transitions=specs, class_names=names,
                            **({"confidence": True} if with_conf else {}), **extra)
    write_change_polygons(frame, args.change_polygons, specs)
    logger.info("wrote %d change polygons against %s to %s", len(frame), before, args.change_polygons)


def main(argv=None) -> None:
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.zone_crs is not None and args.zone is None:
        parser.error("--zone-crs needs --zone")
    if args.target_crs is not None and args.polygons is None:
        parser.error("--target-crs needs --polygons")
    if args.sieve_area is not None and args.polygons is None:
        parser.error("--sieve-area needs --polygons")
    for opt, value in (("--compare", args.compare), ("--compare-iou", args.compare_iou),
                       ("--compare-classes", args.compare_classes)):
        if value is not None and args.polygons is None:
            parser.error(f"{opt} needs --polygons")
    transitions = None
    if args.change_transitions is not None:
        from flair_zonal_detection.change import parse_transition
        transitions = [t.strip() for t in args.change_transitions.split(",") if t.strip()]
        try:
            for spec in transitions:
                parse_transition(spec)
        except ValueError as exc:
            parser.error(f"--change-transitions: {exc}")
    if (args.change_polygons is not None or transitions is not None) and args.change_from is None:
        from flair_zonal_detection.config import load_config
        if (load_config(args.config) or {}).get("change_from") is None:
            opt = "--change-polygons" if args.change_polygons is not None else "--change-transitions"
            parser.error(f"{opt} needs --change-from (or the config key change_from)")
    if args.compare_iou is not None and not 0.0 < args.compare_iou <= 1.0:
        parser.error(f"--compare-iou expects a number in (0, 1], got {args.compare_iou}")
    if args.sieve_area is not None and not 0.0 <= args.sieve_area < float("inf"):
        parser.error(f"--sieve-area expects a number >= 0, got {args.sieve_area}")
    for opt, value in (("--zone-crs", args.zone_crs), ("--target-crs", args.target_crs),
                       ("--zone-stats-crs", args.zone_stats_crs)):
        if value is not None and not (opt != "--target-crs" and value.strip().lower() == "auto"):
            from flair_zonal_detection import crs
            try:
                crs.parse(value)
            except ValueError as exc:
                parser.error(f"{opt}: {exc}")
    try:
        classes = None if args.classes is None else [int(c) for c in args.classes.split(",") if c.strip()]
    except ValueError:
        parser.error(f"--classes expects comma-separated integers, got {args.classes!r}")
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    config = args.config
    if args.threshold_fallback is not None and not 0 <= args.threshold_fallback <= 255:
        parser.error(f"--threshold-fallback expects an integer in 0..255, got {args.threshold_fallback}")
    zone_stats_args = (("zone_stats", args.zone_stats), ("zone_stats_id", args.zone_stats_id),
                       ("zone_stats_crs", args.zone_stats_crs))
    change_args = (("change_from", args.change_from), ("change_transitions", transitions))
    if (args.cog or args.tta is not None or args.thresholds is not None or args.threshold_fallback is not None
            or any(v is not None for _, v in zone_stats_args + change_args)):
        from flair_zonal_detection.config import load_config  # the keys, for this run only
        config = load_config(args.config)
        for key, value in zone_stats_args + change_args:
            if value is not None:
                config[key] = value
        if args.thresholds is not None:
            config["model_threshold_filepath"] = args.thresholds
        if args.threshold_fallback is not None:
            config["threshold_fallback"] = args.threshold_fallback
        if args.cog:
            config["cog_conversion"] = True
        if args.tta is not None:
            config["tta"] = args.tta
    if world > 1:
        outputs = run_sharded(config, int(os.environ.get("RANK", "0")), world, keep_parts=args.keep_parts,
                              geozone=args.zone, geozone_crs=args.zone_crs)
    else:
        from flair_zonal_detection.inference import run_inference
        outputs = run_inference(config, geozone=args.zone, geozone_crs=args.zone_crs)
    if outputs is not None and (world > 1 or args.change_polygons):
        _change_products(args, config, outputs, tables=world > 1)
    if args.polygons and outputs is not None:
        from flair_zonal_detection.inference import raster_to_polygons
        # a write_confidence run also returns f"{task}_confidence" rasters: the polygons then carry their mean
        with_conf = any(str(k).endswith("_confidence") for k in outputs)
        zone_crs = args.zone_crs
        if zone_crs is None and args.zone is not None:
            from flair_zonal_detection.config import load_config, validate_geozone_crs
            zone_crs = validate_geozone_crs(load_config(args.config))
        sieve_area = args.sieve_area
        if sieve_area is None:
            from flair_zonal_detection.config import load_config, validate_sieve_area
            sieve_area = validate_sieve_area(load_config(args.config))
        extra = {k: v for k, v in (("zone", args.zone), ("classes", classes), ("zone_crs", zone_crs),
                                   ("target_crs", args.target_crs), ("sieve_area", sieve_area or None)) if v is not None}
        from flair_zonal_detection.config import load_config, validate_compare
        compare, compare_iou, compare_classes = validate_compare(load_config(args.config))
        compare = args.compare if args.compare is not None else compare
        compare_iou = args.compare_iou if args.compare_iou is not None else compare_iou
        compare_classes = args.compare_classes if args.compare_classes is not None else compare_classes
        sink = {}
        if compare is not None:
            extra.update(compare=compare, compare_iou=compare_iou, compare_classes=compare_classes, _compare_sink=sink)
        gdf = raster_to_polygons(outputs, **({"confidence": True} if with_conf else {}), **extra)
        gdf.to_file(args.polygons, driver="GPKG")
        logger.info("wrote %d polygons to %s", len(gdf), args.polygons)
        if compare is not None:
            out = _write_object_summary(args.polygons, gdf, compare, compare_iou, sink)
            logger.info("wrote the object scores against %s to %s", compare, out)


if __name__ == "__main__":
    main()
