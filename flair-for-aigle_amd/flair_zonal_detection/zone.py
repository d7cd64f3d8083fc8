"""Geozone contours without shapely / geopandas: rings, bounds and the GPU inside mask.

The fork's driver clips its result to an administrative zone (scripts/run_fast_aigle_segmentation.py:135-167,
postprocess_results: intersects + intersection with the contour union).  Here the zone is rasterised on the pixel
grid of the raster it clips (a pixel belongs to the zone when its centre is inside the contour, what
rasterio.mask.mask / GDAL rasterize with all_touched=False mean by "inside") and applied before polygonisation
(raster_to_polygons(zone=...)), and the tile loop may skip the tiles that hold no zone pixel (run_inference with
``skip_tiles_outside_zone``).

The zone must be in the CRS of the raster: nothing here reprojects (the fork reprojects before the call too).
"""
from __future__ import annotations

import json
import os
from typing import List, Sequence, Tuple

import numpy as np

Rings = List[np.ndarray]

_POLYGONAL = ("Polygon", "MultiPolygon", "Feature", "FeatureCollection", "GeometryCollection")


def _is_bounds(obj) -> bool:
    return (isinstance(obj, Sequence) and not isinstance(obj, (str, bytes)) and len(obj) == 4
            and all(isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) for v in obj))


def _ring(coords) -> np.ndarray:
    try:
        r = np.asarray(coords, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("zone: a ring must be a list of (x, y) positions") from None
    if r.ndim != 2 or r.shape[1] < 2 or len(r) < 3:
        raise ValueError(f"zone: a ring must be a list of at least 3 (x, y) positions, got shape {r.shape}")
    return np.ascontiguousarray(r[:, :2])


def _from_geojson(obj: dict, out: List[Rings]) -> None:
    kind = obj.get("type")
    if kind == "Polygon":
        rings = [_ring(c) for c in obj.get("coordinates", [])]
        if rings:
            out.append(rings)
    elif kind == "MultiPolygon":
        for poly in obj.get("coordinates", []):
            _from_geojson({"type": "Polygon", "coordinates": poly}, out)
    elif kind == "Feature":
        if obj.get("geometry") is None:
            raise ValueError("zone: GeoJSON Feature without a geometry")
        _from_geojson(obj["geometry"], out)
    elif kind == "FeatureCollection":
        for f in obj.get("features", []):
            _from_geojson(f, out)
    elif kind == "GeometryCollection":
        for g in obj.get("geometries", []):
            _from_geojson(g, out)
    else:
        raise ValueError(f"zone: GeoJSON type {kind!r} is not polygonal (one of {', '.join(_POLYGONAL)} expected)")


def _collect(geozone, out: List[Rings]) -> None:
    if hasattr(geozone, "__geo_interface__"):
        _from_geojson(dict(geozone.__geo_interface__), out)
    elif isinstance(geozone, dict):
        _from_geojson(geozone, out)
    elif isinstance(geozone, (str, os.PathLike)):
        path = os.fspath(geozone)
        if not str(path).lower().endswith((".geojson", ".json")):
            raise ValueError(f"zone: {path!r} is not a .geojson / .json file")
        with open(path, "r", encoding="utf-8") as f:
            _from_geojson(json.load(f), out)
    elif _is_bounds(geozone):
        left, bottom, right, top = (float(v) for v in geozone)
        out.append([np.array([[left, bottom], [right, bottom], [right, top], [left, top]], dtype=np.float64)])
    elif isinstance(geozone, Sequence) and not isinstance(geozone, bytes):
        for g in geozone:
            _collect(g, out)
    else:
        raise ValueError(f"zone: cannot read a geozone from {type(geozone).__name__}")


def zone_rings(geozone) -> List[Rings]:
    """The polygons of a geozone, each a list of float64 [n, 2] rings in map coordinates (exterior first, then the
    holes; rings as given, closed or not).  Accepted: anything with ``__geo_interface__`` (shapely geometries,
    GeoSeries elements), GeoJSON dicts (Polygon, MultiPolygon, Feature, FeatureCollection, GeometryCollection of
    those), a path to a .geojson / .json file, a (left, bottom, right, top) 4-tuple of bounds (a box), or a sequence of
    any of these.  Anything else raises ValueError."""
    out: List[Rings] = []
    _collect(geozone, out)
    return out


def zone_bounds(geozone) -> Tuple[float, float, float, float]:
    """(minx, miny, maxx, maxy) over every ring of the zone -- what ``.bounds`` of the geometry would give."""
    polys = zone_rings(geozone)
    if not polys:
        raise ValueError("zone: the geozone holds no polygon")
    pts = np.concatenate([r for rings in polys for r in rings])
    return (float(pts[:, 0].min()), float(pts[:, 1].min()), float(pts[:, 0].max()), float(pts[:, 1].max()))


def rings_to_pixels(rings: Rings, left: float, top: float, xres: float, yres: float):
    """(float64 [V, 2] pixel coordinates, int32 [R + 1] ring offsets) of one polygon's rings on a north-up grid:
    px = (x - left) / xres, py = (top - y) / yres"""
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    pix = np.empty_like(xy, dtype=np.float64)
    pix[:, 0] = (xy[:, 0] - float(left)) / float(xres)
    pix[:, 1] = (float(top) - xy[:, 1]) / float(yres)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
    return pix, offsets


def zone_mask(geozone, left: float, top: float, xres: float, yres: float, H: int, W: int):
    """Device uint8 [H, W] inside mask of the zone on the north-up grid whose pixel (r, c) has its centre at
    (left + (c + 0.5) xres, top - (r + 0.5) yres): 1 where that centre is inside the zone.  Each polygon is filled
    even-odd over its rings (holes) and the polygons are united, like unary_union in the fork.  The zone must be in
    the CRS of the grid."""
    import torch
    from flairhip import ops
    if not (xres > 0 and yres > 0):
        raise ValueError(f"zone_mask: positive pixel sizes expected, got {(xres, yres)}")
    polys = zone_rings(geozone)
    mask = None
    for rings in polys:
        pix, offsets = rings_to_pixels(rings, left, top, xres, yres)
        mask = ops.rasterize_zone(pix, offsets, H, W, out=mask, accumulate=mask is not None)
    if mask is None:
        mask = torch.zeros((int(H), int(W)), dtype=torch.uint8, device="cuda")
    return mask
