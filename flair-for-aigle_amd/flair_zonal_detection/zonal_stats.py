"""Zonal statistics of a class raster: for a layer of zones (cadastral parcels, communes, a grid), how much of each
class lies in each zone, and with what confidence.

The zones are rasterised on the class raster's own grid by the rule of the geozone clip (a pixel belongs to a zone when
its centre is inside, even-odd over the zone's rings; include/flairhip_zonestats.h) and tabulated on the GPU
(ops.zone_class_stats, csrc/zone_stats.hip): exact integer pixel counts and confidence sums per (zone, class).  Zones are
independent and may overlap: a pixel counts in every zone that holds it.  Everything in the table below derives from
those integers on the host.
"""
from __future__ import annotations

import csv
import json
import logging
from typing import List, Optional

import numpy as np

logger = logging.getLogger(__name__)

DEFAULT_CLASSES = 19  # the COSIA label set, 0..18 (the default background_value of raster_to_polygons is its last)


class ZoneStatsTable(dict):
    """{column name: numpy array of one value per zone}, in column order, with ``n_classes``, ``class_names``
    ({class id: name} or None) and ``crs`` (the raster's) as attributes."""
    n_classes: int = 0
    class_names = None
    crs = None

    @property
    def columns(self) -> List[str]:
        return list(self)

    @property
    def n_zones(self) -> int:
        return len(next(iter(self.values()))) if self else 0


def stats_table(zone_ids, counts, conf_sums=None, pixel_area: float = 1.0, class_names=None, crs=None) -> ZoneStatsTable:
    """The table of ``zonal_class_stats`` from integer counts [Z, K + 1] (column K = the classes >= K) and, optionally,
    confidence sums of the same shape.  Columns, one value per zone:

      zone            the zone's identifier, as given
      pixels          pixels of the zone, every class ("other" included)
      area            pixels * pixel_area
      pixels_<k>, area_<k>    for k = 0 .. K - 1
      other           pixels whose class is >= K
      majority        the class k < K with most pixels, the smaller one on a tie; -1 when no pixel has a class < K
      confidence      sum of the confidence bytes / (255 * pixels); NaN for an empty zone       } only with
      confidence_<k>  the same over the pixels of class k; NaN where the zone has none           } conf_sums
    """
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 2 or counts.shape[1] < 2:
        raise ValueError(f"stats_table: counts must be [Z, K + 1] with K >= 1, got shape {counts.shape}")
    Z, K = counts.shape[0], counts.shape[1] - 1
    zone_ids = np.asarray(zone_ids)
    if zone_ids.shape != (Z,):
        raise ValueError(f"stats_table: {Z} zone identifiers expected, got shape {zone_ids.shape}")
    area = abs(float(pixel_area))
    t = ZoneStatsTable()
    t.n_classes, t.crs = K, crs
    t.class_names = None if class_names is None else _class_names(class_names)
    pixels = counts.sum(axis=1)
    t["zone"] = zone_ids
    t["pixels"] = pixels
    t["area"] = pixels * area
    for k in range(K):
        t[f"pixels_{k}"] = counts[:, k].copy()
        t[f"area_{k}"] = counts[:, k] * area
    t["other"] = counts[:, K].copy()
    classes = counts[:, :K]
    t["majority"] = np.where(classes.sum(axis=1) > 0, classes.argmax(axis=1), -1).astype(np.int64)  # argmax: the first maximum
    if conf_sums is not None:
        sums = np.asarray(conf_sums, dtype=np.int64)
        if sums.shape != counts.shape:
            raise ValueError(f"stats_table: conf_sums is {sums.shape}, counts {counts.shape}")
        with np.errstate(divide="ignore", invalid="ignore"):
            t["confidence"] = np.where(pixels > 0, sums.sum(axis=1) / (255.0 * pixels), np.nan)
            for k in range(K):
                t[f"confidence_{k}"] = np.where(counts[:, k] > 0, sums[:, k] / (255.0 * counts[:, k]), np.nan)
    return t


def _class_names(class_names) -> dict:
    if isinstance(class_names, dict):
        return {int(k): str(v) for k, v in class_names.items()}
    return {k: str(v) for k, v in enumerate(class_names)}


def _features_in_raster_crs(zones, features, zone_crs, raster_crs):
    """the rings of ``features`` as the raster's CRS sees them: all rings of all zones through one
    zone.zone_in_raster_crs call (one reprojection pass), split back zone by zone"""
    from flair_zonal_detection.zone import detect_zone_crs, zone_in_raster_crs, zone_rings
    if zone_crs is None:
        return features
    if isinstance(zone_crs, str) and zone_crs.strip().lower() == "auto":
        zone_crs = detect_zone_crs(zones)
    rings = [r for _, zone in features for r in zone]
    if not rings:
        return features
    layer = {"type": "MultiPolygon", "coordinates": [[r] for r in rings]}
    moved = zone_in_raster_crs(layer, zone_crs, raster_crs)
    if moved is layer:  # the same CRS: nothing was launched
        return features
    new = [poly[0] for poly in zone_rings(moved)]
    if len(new) != len(rings):
        raise ValueError("zonal_class_stats: the reprojection changed the number of rings")
    out, k = [], 0
    for props, zone in features:
        out.append((props, new[k:k + len(zone)]))
        k += len(zone)
    return out


def _zones_in_pixels(zones, id_field, zone_crs, raster_crs, left, top, xres, yres, name: str):
    """(identifiers [Z], zones in pixel coordinates: a list of ring lists) of a zone layer as zone.zone_features reads
    it, reprojected to the raster's CRS first when ``zone_crs`` says so; ValueError messages start with ``name``"""
    from flair_zonal_detection.zone import zone_features
    features = _features_in_raster_crs(zones, zone_features(zones), zone_crs, raster_crs)
    if id_field is None:
        ids = np.arange(len(features), dtype=np.int64)
    else:
        missing = [i for i, (props, _) in enumerate(features) if id_field not in props]
        if missing:
            raise ValueError(f"{name}: zone {missing[0]} has no property {id_field!r}")
        ids = np.asarray([props[id_field] for props, _ in features])
    zones_pix = []
    for _, rings in features:  # rings_to_pixels' two lines, ring by ring
        zones_pix.append([np.stack([(r[:, 0] - left) / xres, (top - r[:, 1]) / yres], axis=1) for r in rings])
    return ids, zones_pix


def zonal_class_stats(raster, zones, id_field: Optional[str] = None, confidence=None, zone_crs=None, class_names=None,
                      n_classes: Optional[int] = None) -> ZoneStatsTable:
    """Per-zone class areas of a class raster, and their confidence.

    ``raster``: a path, a raster object or the outputs dict of run_inference, as raster_to_polygons accepts (a one-band
    uint8 class raster).  ``zones``: a zone layer as zone.zone_features reads it -- a GeoJSON FeatureCollection (dict or
    .geojson / .json path) whose Polygon / MultiPolygon Features are the zones, bare geometries, bounds tuples or a
    sequence of those.  ``id_field``: the Feature property that names a zone in the ``zone`` column (every zone must
    have it); None: the zone's index.  ``confidence``: None, a confidence raster (path, raster object or closed writer on
    the class raster's grid) or True = the f"{task}_confidence" entry of the outputs dict, the convention of
    raster_to_polygons; the table then has the confidence columns.  ``zone_crs``: the CRS the zones are given in (a CRS
    or "auto"), reprojected to the raster's first (zone.zone_in_raster_crs); None: the raster's CRS.  ``n_classes``:
    K, the classes 0 .. K - 1 get columns and every other value counts as ``other``; default: the number of
    ``class_names`` ({id: name} or a list; max id + 1 for a dict), else 19.

    Returns a ZoneStatsTable (stats_table lists the columns); areas are in the raster's map units squared."""
    import torch
    from flairhip import ops
    from flair_zonal_detection.inference import (_bounds4, _class_band, _confidence_band, _confidence_source,
                                                 _polygon_source)
    name = "zonal_class_stats"
    src = _polygon_source(raster)
    data = _class_band(src, name)
    xres, yres = (float(v) for v in src.res)
    left, _, _, top = _bounds4(src)
    if not (xres > 0 and yres > 0):
        raise ValueError(f"{name}: positive pixel sizes expected, got {(xres, yres)}")
    conf = None
    if confidence is not None and confidence is not False:
        conf = _confidence_band(_confidence_source(raster, confidence), src, data, name)
    names = None if class_names is None else _class_names(class_names)
    if n_classes is None:
        n_classes = max(names) + 1 if names else DEFAULT_CLASSES
    if not 1 <= int(n_classes) <= 256:
        raise ValueError(f"{name}: n_classes {n_classes} outside 1..256")
    crs = getattr(src, "crs", None)
    ids, zones_pix = _zones_in_pixels(zones, id_field, zone_crs, crs, left, top, xres, yres, name)
    dev = torch.device("cuda", torch.cuda.current_device())
    counts, sums = ops.zone_class_stats(torch.from_numpy(np.ascontiguousarray(data)).to(dev), zones_pix, int(n_classes),
                                        conf=None if conf is None else torch.from_numpy(np.ascontiguousarray(conf)).to(dev))
    return stats_table(ids, counts.cpu().numpy(), None if sums is None else sums.cpu().numpy(), xres * yres, names, crs)


def _cell(v):
    """one table value as CSV / JSON text material: Python int, float (repr round-trips float64) or str"""
    if isinstance(v, (np.integer, int)) and not isinstance(v, bool):
        return int(v)
    if isinstance(v, (np.floating, float)):
        return float(v)
    return str(v)


def write_zone_stats_csv(table, path: str) -> str:
    """One header line with the column names, one line per zone.  Floats are written with repr (they read back as
    the same float64), NaN as ``nan``."""
    cols = list(table)
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for row in zip(*(table[c] for c in cols)):
            w.writerow([repr(c) if isinstance(c, float) else c for c in map(_cell, row)])
    return path


def write_zone_stats_json(table, path: str) -> str:
    """{"n_classes", "class_names", "crs", "columns", "zones": [{column: value}, ...]}; NaN is written as null."""
    cols = list(table)
    zones = []
    for row in zip(*(table[c] for c in cols)):
        cells = [_cell(v) for v in row]
        zones.append({c: (None if isinstance(v, float) and v != v else v) for c, v in zip(cols, cells)})
    names = getattr(table, "class_names", None)
    doc = {"n_classes": int(getattr(table, "n_classes", 0)),
           "class_names": None if names is None else {str(k): v for k, v in names.items()},
           "crs": None if getattr(table, "crs", None) is None else str(table.crs), "columns": cols, "zones": zones}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(doc, f, indent=1, allow_nan=False)
    return path
