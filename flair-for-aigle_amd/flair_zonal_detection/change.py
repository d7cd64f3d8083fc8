"""Land-cover change between two class rasters on one grid: what changed, how much, from which class to which, and in
which zone.

Two products, both from exact integers taken on the GPU:

  * per-zone transition matrices (ops.zone_transition_stats, csrc/zone_stats.hip): counts[z, a, b] = the pixels of zone
    z that were class a in ``before`` and are class b in ``after``, with the sums of the *after* run's confidence bytes
    over the same pixels.  Zones and membership are those of zonal_stats.zonal_class_stats (a pixel belongs to a zone
    when its centre is inside; zones may overlap).  ``change_table`` derives the per-zone columns and the long
    (zone, from, to) form from those integers on the host.
  * change polygons: the two rasters are recoded into one raster of transition codes through a table
    (``transition_lut``, ops.change_codes, csrc/change.hip) which the existing polygoniser takes with 255 = "no listed
    transition" as its background, so clipping, sieve, confidence and reprojection are raster_to_polygons' own.

Limits: both rasters uint8 on one grid (same shape, bounds and resolution; nothing is resampled), K <= 32 classes.
"""
from __future__ import annotations

import csv
import logging
from typing import List, Optional, Tuple

import numpy as np

from flair_zonal_detection.zonal_stats import DEFAULT_CLASSES, ZoneStatsTable, _cell, _class_names

logger = logging.getLogger(__name__)

MAX_CLASSES = 32  # ops.CHANGE_MAX_CLASSES: the transition tables of the GPU tabulation hold (K + 1)^2 entries per wave
MAX_TRANSITIONS = 255  # codes 0..254; 255 = no listed transition
NO_TRANSITION = 255
ANY = "*"


def _check_classes(n_classes, name: str) -> int:
    if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f"{name}: n_classes {n_classes!r} outside 1..{MAX_CLASSES}")
    return int(n_classes)


def parse_transition(spec, n_classes: Optional[int] = None) -> Tuple[object, object]:
    """(from, to) of one transition spec: a string "from:to" or a pair, either side ``"*"`` (any class) or a class id;
    with ``n_classes`` the ids must be below it.  A malformed spec raises ValueError."""
    if isinstance(spec, str):
        parts = spec.split(":")
        if len(parts) != 2:
            raise ValueError(f"transition {spec!r}: 'FROM:TO' expected, e.g. '*:6', '6:*' or '4:0'")
    elif isinstance(spec, (tuple, list)) and len(spec) == 2:
        parts = list(spec)
    else:
        raise ValueError(f"transition {spec!r}: a string 'FROM:TO' or a pair (from, to) expected")
    sides = []
    for side in parts:
        if isinstance(side, str):
            side = side.strip()
            if side == ANY:
                sides.append(ANY)
                continue
            if not side.isdigit():
                raise ValueError(f"transition {spec!r}: {side!r} is neither '*' nor a class id")
            side = int(side)
        if isinstance(side, bool) or not isinstance(side, (int, np.integer)) or side < 0:
            raise ValueError(f"transition {spec!r}: {side!r} is neither '*' nor a class id")
        if n_classes is not None and side >= n_classes:
            raise ValueError(f"transition {spec!r}: class {int(side)} is not below n_classes = {n_classes}")
        sides.append(int(side))
    return sides[0], sides[1]


def spec_string(spec) -> str:
    return f"{spec[0]}:{spec[1]}"


def transition_lut(transitions, n_classes: int):
    """(lut uint8 [K + 1, K + 1], specs): the table ops.change_codes takes and the parsed (from, to) pairs.

    ``transitions``: a list of specs (parse_transition), or None = ``*:k`` for every k < K, so that code k means
    "became k".  Spec i gets code i; where two specs cover one (from, to) pair the earlier one wins; 255 means no listed
    transition.  A wildcard stands for the classes 0 .. K - 1 other than the one on the other side: it never covers
    from == to (an unchanged pixel), and never row or column K ("other", the values >= K such as the zone clip's 255:
    a pixel one run did not classify has no transition).  A spec with two class ids means that pair, equal ids
    included.  More than 255 specs, a class >= K or a malformed spec raise ValueError."""
    K = _check_classes(n_classes, "transition_lut")
    if transitions is None:
        specs = [(ANY, k) for k in range(K)]
    else:
        if isinstance(transitions, str):
            raise ValueError(f"transition_lut: a list of specs expected, got the string {transitions!r}")
        specs = [parse_transition(s, K) for s in transitions]
    if len(specs) > MAX_TRANSITIONS:
        raise ValueError(f"transition_lut: {len(specs)} transitions, at most {MAX_TRANSITIONS} fit a uint8 code")
    lut = np.full((K + 1, K + 1), NO_TRANSITION, dtype=np.uint8)
    for code in range(len(specs) - 1, -1, -1):  # backwards: the earlier spec is written last and wins
        a, b = specs[code]
        wild = a == ANY or b == ANY
        for i in (range(K) if a == ANY else (a,)):
            for j in (range(K) if b == ANY else (b,)):
                if not (wild and i == j):
                    lut[i, j] = code
    return lut, specs


def change_table(zone_ids, counts, conf_sums=None, pixel_area: float = 1.0, class_names=None, crs=None) -> ZoneStatsTable:
    """The table of ``zonal_change_stats`` from integer transition counts [Z, K + 1, K + 1] (row and column K = the
    values >= K, "other") and, optionally, confidence sums of the same shape.  Columns, one value per zone:

      zone               the zone's identifier, as given
      pixels, area       pixels of the zone, every entry; pixels * pixel_area
      changed            the sum of the off-diagonal entries ("other" included), changed_area = changed * pixel_area
      changed_fraction   changed / pixels, a float64 quotient of exact integers; NaN for an empty zone
      stable             the sum of the diagonal
      gain_<k>, loss_<k>, net_<k>   for k < K: column sum minus diagonal, row sum minus diagonal, gain - loss
      confidence_changed sum of the confidence bytes over the off-diagonal entries / (255 * changed); NaN where nothing
                         changed (only with conf_sums)

    and the attribute ``transitions``, the long form: a dict of arrays zone, from, to, pixels, area (and confidence =
    sum / (255 * pixels) with conf_sums), one entry per non-zero count in (zone, from, to) order, "other" written -1."""
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 3 or counts.shape[1] != counts.shape[2] or counts.shape[1] < 2:
        raise ValueError(f"change_table: counts must be [Z, K + 1, K + 1] with K >= 1, got shape {counts.shape}")
    Z, K = counts.shape[0], counts.shape[1] - 1
    zone_ids = np.asarray(zone_ids)
    if zone_ids.shape != (Z,):
        raise ValueError(f"change_table: {Z} zone identifiers expected, got shape {zone_ids.shape}")
    sums = None
    if conf_sums is not None:
        sums = np.asarray(conf_sums, dtype=np.int64)
        if sums.shape != counts.shape:
            raise ValueError(f"change_table: conf_sums is {sums.shape}, counts {counts.shape}")
    area = abs(float(pixel_area))
    t = ZoneStatsTable()
    t.n_classes, t.crs = K, crs
    t.class_names = None if class_names is None else _class_names(class_names)
    pixels = counts.sum(axis=(1, 2))
    diag = np.diagonal(counts, axis1=1, axis2=2)  # [Z, K + 1]
    stable = diag.sum(axis=1)
    changed = pixels - stable
    t["zone"] = zone_ids
    t["pixels"] = pixels
    t["area"] = pixels * area
    t["changed"] = changed
    t["changed_area"] = changed * area
    with np.errstate(divide="ignore", invalid="ignore"):
        t["changed_fraction"] = np.where(pixels > 0, changed / pixels.astype(np.float64), np.nan)
    t["stable"] = stable
    gain = counts.sum(axis=1) - diag  # column sums: everything that became k, minus what already was
    loss = counts.sum(axis=2) - diag
    for k in range(K):
        t[f"gain_{k}"] = gain[:, k].copy()
        t[f"loss_{k}"] = loss[:, k].copy()
        t[f"net_{k}"] = gain[:, k] - loss[:, k]
    if sums is not None:
        off = sums.sum(axis=(1, 2)) - np.diagonal(sums, axis1=1, axis2=2).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t["confidence_changed"] = np.where(changed > 0, off / (255.0 * changed), np.nan)
    z, a, b = np.nonzero(counts)  # row-major: (zone, from, to) order, "other" (index K) last on either side
    n = counts[z, a, b]
    long = {"zone": zone_ids[z], "from": np.where(a == K, -1, a).astype(np.int64),
            "to": np.where(b == K, -1, b).astype(np.int64), "pixels": n, "area": n * area}
    if sums is not None:
        long["confidence"] = sums[z, a, b] / (255.0 * n)
    t.transitions = long
    return t


def _same_grid_band(before, shape, bounds, res, name: str) -> np.ndarray:
    """The one uint8 band of the class raster ``before`` (path, raster object, outputs dict or closed writer), which
    must lie on the grid of ``after``: its ``shape``, ``bounds`` (left, bottom, right, top; to within 1e-6 of a pixel)
    and ``res`` -- the check inference._compare_source makes for a reference raster --, else ValueError starting with
    ``name``."""
    from flair_zonal_detection.inference import _bounds4, _polygon_source
    bsrc = _polygon_source(before)
    if bsrc.count != 1:
        raise ValueError(f"{name}: the before raster must have one band, got {bsrc.count}")
    band = np.asarray(bsrc.read(1))
    if band.dtype != np.uint8:
        raise ValueError(f"{name}: uint8 before raster expected, got {band.dtype}")
    if band.shape != tuple(shape):
        raise ValueError(f"{name}: before raster is {band.shape}, the after raster {tuple(shape)}")
    bres, bbounds = tuple(float(v) for v in bsrc.res), _bounds4(bsrc)
    tol = 1e-6 * max(float(v) for v in res)
    if bres != tuple(float(v) for v in res) or any(abs(a - b) > tol for a, b in zip(bbounds, bounds)):
        raise ValueError(f"{name}: the before raster's bounds / resolution differ from the after raster's "
                         f"({bbounds}, {bres} vs {tuple(bounds)}, {tuple(res)}); the two runs must share one grid")
    return band


def _pair(before, after, name: str):
    """(after's source, after band, before band, left, top, xres, yres) of two class rasters on one grid"""
    from flair_zonal_detection.inference import _bounds4, _class_band, _polygon_source
    src = _polygon_source(after)
    data = _class_band(src, name)
    xres, yres = (float(v) for v in src.res)
    if not (xres > 0 and yres > 0):
        raise ValueError(f"{name}: positive pixel sizes expected, got {(xres, yres)}")
    left, _, _, top = _bounds4(src)
    old = _same_grid_band(before, data.shape, _bounds4(src), (xres, yres), name)
    return src, data, old, left, top, xres, yres


def _n_classes(n_classes, names, name: str) -> int:
    if n_classes is None:
        n_classes = max(names) + 1 if names else DEFAULT_CLASSES
    return _check_classes(n_classes, name)


def transition_specs(transitions, n_classes: Optional[int] = None, class_names=None) -> List[Tuple[object, object]]:
    """the parsed specs transition_lut returns for ``transitions``, with K resolved as change_polygons resolves it"""
    names = None if class_names is None else _class_names(class_names)
    return transition_lut(transitions, _n_classes(n_classes, names, "transition_specs"))[1]


def zonal_change_stats(before, after, zones=None, id_field: Optional[str] = None, confidence=None, zone_crs=None,
                       class_names=None, n_classes: Optional[int] = None) -> ZoneStatsTable:
    """Per-zone class transitions between two runs.

    ``before`` and ``after``: class rasters as zonal_class_stats accepts them (a path, a raster object or the outputs
    dict of run_inference; one uint8 band each); ``before`` must lie on ``after``'s grid (same shape, bounds to 1e-6 of
    a pixel, same resolution), else ValueError: nothing is resampled.  ``zones``: a zone layer as zone.zone_features
    reads it, or None = one zone, the raster's bounds.  ``id_field``, ``zone_crs``, ``class_names``: as for
    zonal_class_stats.  ``confidence``: None, the confidence raster of the *after* run, or True = the
    f"{task}_confidence" entry of ``after`` when that is an outputs dict.  ``n_classes``: K in 1..32; default: from
    ``class_names``, else 19.

    Returns the ZoneStatsTable of ``change_table``; areas are in the raster's map units squared."""
    import torch
    from flairhip import ops
    from flair_zonal_detection.inference import _confidence_band, _confidence_source
    from flair_zonal_detection.zonal_stats import _zones_in_pixels
    name = "zonal_change_stats"
    src, data, old, left, top, xres, yres = _pair(before, after, name)
    conf = None
    if confidence is not None and confidence is not False:
        conf = _confidence_band(_confidence_source(after, confidence), src, data, name)
    names = None if class_names is None else _class_names(class_names)
    K = _n_classes(n_classes, names, name)
    crs = getattr(src, "crs", None)
    H, W = data.shape
    if zones is None:
        ids = np.zeros(1, dtype=np.int64)
        zones_pix = [[np.array([[0.0, 0.0], [float(W), 0.0], [float(W), float(H)], [0.0, float(H)]])]]
    else:
        ids, zones_pix = _zones_in_pixels(zones, id_field, zone_crs, crs, left, top, xres, yres, name)
    dev = torch.device("cuda", torch.cuda.current_device())

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    counts, sums = ops.zone_transition_stats(up(old), up(data), zones_pix, K, conf=None if conf is None else up(conf))
    return change_table(ids, counts.cpu().numpy(), None if sums is None else sums.cpu().numpy(), xres * yres, names, crs)


def _write_csv(cols, columns, path: str) -> str:
    with open(path, "w", newline="", encoding="utf-8") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for row in zip(*(columns[c] for c in cols)):
            w.writerow([repr(c) if isinstance(c, float) else c for c in map(_cell, row)])
    return path


def write_change_csv(table, path: str) -> str:
    """The wide form: one header line with the column names, one line per zone (floats with repr, NaN as ``nan``)."""
    return _write_csv(list(table), table, path)


def write_transitions_csv(table, path: str) -> str:
    """The long form (``table.transitions``): one line per non-zero (zone, from, to), "other" as -1."""
    long = table.transitions
    return _write_csv(list(long), long, path)


def _code_raster(codes: np.ndarray, left: float, top: float, xres: float, yres: float, crs):
    from flair_zonal_detection.raster import ArrayRaster

    class CodeRaster(ArrayRaster):  # an in-memory raster on after's grid, whose pixels need not be square
        @property
        def res(self):
            return (self._res, yres)

    return CodeRaster(codes[None], left, top, xres, crs)


def change_polygons(before, after, transitions=None, min_area: float = 1.0, simplification: float = 0.1,
                    n_jobs: Optional[int] = None, zone=None, zone_crs=None, sieve_area: float = 0.0, target_crs=None,
                    confidence=None, n_classes: Optional[int] = None, class_names=None):
    """Polygons of the listed transitions between two class rasters on one grid (``before``, ``after``, ``confidence``
    and ``n_classes`` as for zonal_change_stats; ``transitions`` as for transition_lut, None = "became k" for every k).

    The two rasters are recoded on the GPU into one raster of transition codes (ops.change_codes), which goes through
    raster_to_polygons with 255 = "no listed transition" as the background: one polygon per 4-connected region of one
    code.  ``min_area``, ``simplification``, ``n_jobs``, ``zone``, ``zone_crs``, ``sieve_area``, ``target_crs`` and
    the confidence columns are raster_to_polygons' own and mean what they mean there (the sieve merges small regions
    of one code into a neighbouring code, never into the background).

    Returns raster_to_polygons' frame with ``class_id`` replaced by ``transition`` (the spec string, e.g. "*:6"),
    ``from_class`` and ``to_class`` (int64, -1 for a wildcard side); an unchanged pair gives an empty frame."""
    import torch
    from flairhip import ops
    from flair_zonal_detection.inference import _confidence_source, raster_to_polygons
    name = "change_polygons"
    src, data, old, left, top, xres, yres = _pair(before, after, name)
    names = None if class_names is None else _class_names(class_names)
    lut, specs = transition_lut(transitions, _n_classes(n_classes, names, name))
    conf = None
    if confidence is not None and confidence is not False:
        conf = _confidence_source(after, confidence)
    dev = torch.device("cuda", torch.cuda.current_device())
    d_old = torch.from_numpy(np.ascontiguousarray(old)).to(dev)
    d_new = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    codes = ops.change_codes(d_old, d_new, lut, out=d_new).cpu().numpy()
    raster = _code_raster(codes, getattr(src, "left", left), getattr(src, "top", top), xres, yres,
                          getattr(src, "crs", None))
    frame = raster_to_polygons(raster, ignore_background=True, background_value=NO_TRANSITION, min_area=min_area,
                               simplification=simplification, n_jobs=n_jobs, confidence=conf, zone=zone,
                               zone_crs=zone_crs, target_crs=target_crs, sieve_area=sieve_area)
    code = frame["class_id"].to_numpy().astype(np.int64)
    side = np.array([[-1 if s == ANY else s for s in spec] for spec in specs], dtype=np.int64).reshape(-1, 2)
    crs = getattr(frame, "crs", None)
    out = frame.drop(columns=["class_id"])
    out.insert(0, "transition", np.array([spec_string(specs[c]) for c in code], dtype=object))
    out.insert(1, "from_class", side[code, 0] if len(code) else np.zeros(0, np.int64))
    out.insert(2, "to_class", side[code, 1] if len(code) else np.zeros(0, np.int64))
    if getattr(out, "crs", None) is None and crs is not None:
        out.crs = crs
    return out


def write_change_polygons(frame, path: str, specs) -> str:
    """The frame of ``change_polygons`` as a GeoPackage.  The layer's ``class_id`` column holds the transition code
    (the index of the polygon's spec in ``specs``, the parsed list transition_lut returns), the columns from_class and
    to_class follow, then the frame's other numeric columns (confidence, pixels)."""
    from flair_zonal_detection.gpkg import write_polygons
    from flair_zonal_detection.polygons import Polygon
    index = {spec_string(s): i for i, s in reversed(list(enumerate(specs)))}

    def rings_of(g):
        if isinstance(g, Polygon):
            return g._store.rings(g._q)
        return [np.asarray(g.exterior.coords)] + [np.asarray(r.coords) for r in g.interiors]

    extra = {c: frame[c].to_numpy() for c in frame.columns
             if c not in ("transition", "geometry") and frame[c].dtype.kind in "fiub"}
    return write_polygons(path, ((index[t], rings_of(g)) for t, g in zip(frame["transition"], frame["geometry"])),
                          crs=getattr(frame, "crs", None), **({"columns": extra} if extra else {}))
