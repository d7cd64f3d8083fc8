"""Zonal-inference configuration -- counterpart of the reference's flair_zonal_detection/config.py
(load_config :6, validate_config :14-29, recaps :33-92).  Same required keys and the same error types."""
from __future__ import annotations

import logging
import os

import yaml

logger = logging.getLogger(__name__)

REQUIRED_KEYS = ["output_path", "output_name", "model_weights", "img_pixels_detection", "margin", "modalities",
                 "tasks", "output_px_meters"]


def load_config(path: str) -> dict:
    with open(path, "r") as f:
        return yaml.safe_load(f)


def validate_write_confidence(config: dict) -> bool:
    """The optional key write_confidence (default false): a second one-band uint8 raster per task that holds
    rint(255 * max softmax) of every written pixel.  Only legal with output_type argmax."""
    write_confidence = config.get("write_confidence", False)
    if not isinstance(write_confidence, bool):
        raise ValueError(f"write_confidence must be true or false, got {write_confidence!r}")
    if write_confidence and config.get("output_type", "argmax") != "argmax":
        raise ValueError("write_confidence needs output_type: argmax (a class_prob raster already holds every "
                         f"probability), got {config.get('output_type')!r}")
    return write_confidence


TTA_MODES = ("none", "flips", "d4")  # the keys of flairhip.augment.TTA_VIEWS


def validate_tta(config: dict) -> str:
    """The optional key tta (default none): test-time augmentation of the tile loop.  'flips': every tile is predicted
    as it is and under the three flips, 'd4': under all 8 flips / rotations of the square; the softmax probabilities
    of the views are averaged in the tile's frame before the uint8 conversion.  Anything else raises ValueError."""
    tta = config.get("tta", "none")
    if tta is None:
        return "none"
    if not isinstance(tta, str) or tta.strip().lower() not in TTA_MODES:
        raise ValueError(f"tta must be one of {', '.join(TTA_MODES)}, got {tta!r}")
    return tta.strip().lower()


def validate_skip_tiles_outside_zone(config: dict) -> bool:
    """The optional key skip_tiles_outside_zone (default false): with a geozone, run_inference drops the tiles whose
    kept area (grown by a pixel) holds no pixel centre inside the zone contour before the tile loop."""
    skip = config.get("skip_tiles_outside_zone", False)
    if not isinstance(skip, bool):
        raise ValueError(f"skip_tiles_outside_zone must be true or false, got {skip!r}")
    return skip


def validate_geozone_crs(config: dict):
    """The optional key geozone_crs (default none: the geozone is in the raster's CRS): the CRS the geozone is given
    in -- 'EPSG:4326', an EPSG code, or 'auto' (GeoJSON: the legacy crs member, else EPSG:4326).  run_inference
    reprojects the zone to the raster's CRS before slicing.  An unsupported CRS raises ValueError here."""
    geozone_crs = config.get("geozone_crs")
    if geozone_crs is None:
        return None
    if isinstance(geozone_crs, str) and geozone_crs.strip().lower() == "auto":
        return "auto"
    from flair_zonal_detection import crs
    if isinstance(geozone_crs, bool) or not isinstance(geozone_crs, (str, int)):
        raise ValueError(f"geozone_crs must be 'auto', 'EPSG:NNNN' or an EPSG code, got {geozone_crs!r}")
    crs.parse(geozone_crs)
    return geozone_crs


def validate_sieve_area(config: dict) -> float:
    """The optional key sieve_area (default 0: off), in map units squared: before polygonisation, regions of the class
    raster below that area are merged into their largest neighbour (raster_to_polygons(sieve_area=...)).  A number
    >= 0 (or a string that reads as one), else ValueError."""
    sieve_area = config.get("sieve_area", 0.0)
    if sieve_area is None:
        return 0.0
    if isinstance(sieve_area, bool) or not isinstance(sieve_area, (int, float, str)):
        raise ValueError(f"sieve_area must be a number >= 0, got {sieve_area!r}")
    try:
        value = float(sieve_area)
    except ValueError:
        raise ValueError(f"sieve_area must be a number >= 0, got {sieve_area!r}") from None
    if not (value >= 0.0 and value != float("inf")):
        raise ValueError(f"sieve_area must be a number >= 0, got {sieve_area!r}")
    return value


def validate_compare(config: dict):
    """The optional keys of object matching against a reference (raster_to_polygons(compare=...)): compare_raster
    (default none: off; a path to a class raster on the prediction's grid, or to a GeoJSON layer of known objects),
    compare_iou (default 0.5, a number in (0, 1]) and compare_classes ("same", the default, or "any").  Returns the
    three; a bad value raises ValueError."""
    path = config.get("compare_raster")
    if path is not None and not isinstance(path, (str, os.PathLike)):
        raise ValueError(f"compare_raster must be a path, got {path!r}")
    iou = config.get("compare_iou", 0.5)
    if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not 0.0 < float(iou) <= 1.0:
        raise ValueError(f"compare_iou must be a number in (0, 1], got {iou!r}")
    mode = config.get("compare_classes", "same")
    if mode not in ("same", "any"):
        raise ValueError(f"compare_classes must be 'same' or 'any', got {mode!r}")
    return (None if path is None else os.fspath(path)), float(iou), mode


def validate_zone_stats(config: dict):
    """The optional keys of zonal statistics, all off by default: zone_stats (a path to a GeoJSON layer of zones; after
    the tile loop every written class raster ``<name>.tif`` gets ``<name>_zone_stats.csv``, the table of
    zonal_stats.zonal_class_stats), zone_stats_id (the Feature property that names a zone; default: its index) and
    zone_stats_crs (the CRS the layer is given in, or 'auto'; default: the raster's).  Returns the three; a bad value
    raises ValueError."""
    path = config.get("zone_stats")
    if path is not None and not isinstance(path, (str, os.PathLike)):
        raise ValueError(f"zone_stats must be a path to a GeoJSON file, got {path!r}")
    field = config.get("zone_stats_id")
    if field is not None and not isinstance(field, str):
        raise ValueError(f"zone_stats_id must be a property name, got {field!r}")
    crs_name = config.get("zone_stats_crs")
    if crs_name is not None and not (isinstance(crs_name, str) and crs_name.strip().lower() == "auto"):
        from flair_zonal_detection import crs
        if isinstance(crs_name, bool) or not isinstance(crs_name, (str, int)):
            raise ValueError(f"zone_stats_crs must be 'auto', 'EPSG:NNNN' or an EPSG code, got {crs_name!r}")
        crs.parse(crs_name)
    return (None if path is None else os.fspath(path)), field, crs_name


def validate_change(config: dict):
    """The optional keys of land-cover change, all off by default: change_from (the class raster of an earlier run on
    the same grid: a path, or {task name: path}; after the tile loop every written class raster ``<name>.tif`` gets
    ``<name>_zone_change.csv`` and ``<name>_zone_transitions.csv``, the tables of change.zonal_change_stats over the
    zones of the zone_stats layer, or over the whole raster as one zone) and change_transitions (a list of transition
    specs such as '*:6' or '4:0' for change.change_polygons; default: 'became k' for every class).  Returns the two;
    a bad value raises ValueError."""
    source = config.get("change_from")
    if isinstance(source, dict):
        for task, path in source.items():
            if not isinstance(task, str) or not isinstance(path, (str, os.PathLike)):
                raise ValueError(f"change_from must map task names to paths, got {task!r}: {path!r}")
        source = {task: os.fspath(path) for task, path in source.items()}
    elif source is not None:
        if not isinstance(source, (str, os.PathLike)):
            raise ValueError(f"change_from must be a path to a class raster or {{task: path}}, got {source!r}")
        source = os.fspath(source)
    specs = config.get("change_transitions")
    if specs is not None:
        from flair_zonal_detection.change import parse_transition
        if isinstance(specs, str) or not isinstance(specs, (list, tuple)):
            raise ValueError(f"change_transitions must be a list of specs such as '*:6', got {specs!r}")
        for spec in specs:
            if not isinstance(spec, str):
                raise ValueError(f"change_transitions must be a list of spec strings, got {spec!r}")
            parse_transition(spec)
        specs = list(specs)
        if source is None:
            raise ValueError("change_transitions needs change_from")
    return source, specs


COG_OVERVIEW_RESAMPLING = ("nearest", "mode", "average")


def validate_cog_conversion(config: dict) -> bool:
    """The key cog_conversion (default false) of every FLAIR-HUB zonal configuration: after the tile loop each written
    raster ``<name>.tif`` is converted to the cloud-optimised ``<name>_COG.tif`` (overview pyramid, IFDs ahead of the
    data) and removed."""
    cog = config.get("cog_conversion", False)
    if cog is None:
        return False
    if not isinstance(cog, bool):
        raise ValueError(f"cog_conversion must be true or false, got {cog!r}")
    return cog


def validate_cog_overview_resampling(config: dict) -> str:
    """The optional key cog_overview_resampling (default nearest, the reference's choice): how an overview pixel is
    made from the 2 x 2 block under it.  'mode': class rasters take the most frequent class, confidence and
    class-probability rasters the average; 'average': the rounded mean for every raster."""
    method = config.get("cog_overview_resampling", "nearest")
    if method is None:
        return "nearest"
    if not isinstance(method, str) or method.strip().lower() not in COG_OVERVIEW_RESAMPLING:
        raise ValueError(f"cog_overview_resampling must be one of {', '.join(COG_OVERVIEW_RESAMPLING)}, got {method!r}")
    return method.strip().lower()


def validate_threshold_fallback(config: dict) -> int:
    """The optional key threshold_fallback (default 18, raster_to_polygons' default background_value, so that rejected
    pixels never become polygons): the label of a pixel at which no class reaches its calibrated threshold.  An int in
    0..255, else ValueError."""
    fallback = config.get("threshold_fallback", 18)
    if isinstance(fallback, bool) or not isinstance(fallback, int) or not 0 <= fallback <= 255:
        raise ValueError(f"threshold_fallback must be an integer in 0..255, got {fallback!r}")
    return fallback


def threshold_file(config: dict):
    """The calibrated class thresholds in effect: the path in config["model_threshold_filepath"] (what prep_config
    stores; flair_hub's calibrate stage writes the file, flairhip.calibration reads it), or None.  A path that does not
    exist is warned about and ignored, as the reference's prepare_local_model_folder does with a model folder without
    best_thresholds.yaml; so is a file next to output_type: class_prob, where there is no label to threshold."""
    path = config.get("model_threshold_filepath")
    if not path:
        return None
    if not os.path.isfile(str(path)):
        logger.warning("threshold file %s does not exist: running without calibrated thresholds", path)
        return None
    if config.get("output_type", "argmax") != "argmax":
        logger.warning("threshold file %s is not applied: thresholds apply to label output (output_type: argmax), not "
                       "to %s", path, config.get("output_type"))
        return None
    return str(path)


def validate_config(config: dict) -> None:
    for key in REQUIRED_KEYS:
        if key not in config:
            raise ValueError(f"Missing required config key: {key}")
    validate_threshold_fallback(config)
    validate_write_confidence(config)
    validate_tta(config)
    validate_skip_tiles_outside_zone(config)
    validate_geozone_crs(config)
    validate_sieve_area(config)
    validate_compare(config)
    validate_zone_stats(config)
    validate_change(config)
    validate_cog_conversion(config)
    validate_cog_overview_resampling(config)
    if not os.path.isfile(config["model_weights"]):
        raise FileNotFoundError(f"Model weights not found at: {config['model_weights']}")
    os.makedirs(config["output_path"], exist_ok=True)


def config_recap_1(config: dict) -> None:
    mods = ", ".join(m for m, on in config["modalities"]["inputs"].items() if on)
    tasks = ", ".join(t["name"] for t in config["tasks"] if t["active"])
    logger.info("FLAIR-HUB zone detection | output %s/%s.tif | modalities %s | tasks %s | output type %s | "
                "checkpoint %s | batch %s", config["output_path"], config["output_name"], mods, tasks,
                config.get("output_type", "argmax"), config["model_weights"], config.get("batch_size"))


def config_recap_2(config: dict) -> None:
    res = config["reference_resolution"]
    shape = config.get("image_shape_px", {})
    if shape:
        logger.info("image %s x %s px (%.2f m x %.2f m)", shape["height"], shape["width"], shape["height"] * res,
                    shape["width"] * res)
    logger.info("reference resolution %s m/px, output %s m/px, patch %s px (%.2f m), margin %s px (%.2f m)", res,
                config["output_px_meters"], config["img_pixels_detection"], config["img_pixels_detection"] * res,
                config["margin"], config["margin"] * res)
