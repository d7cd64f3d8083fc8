"""Geozone contours without shapely / geopandas: rings, bounds and the GPU inside mask.

The fork's driver clips its result to an administrative zone (scripts/run_fast_aigle_segmentation.py:135-167,
postprocess_results: intersects + intersection with the contour union).  Here the zone is rasterised on the pixel
grid of the raster it clips (a pixel belongs to the zone when its centre is inside the contour, what
rasterio.mask.mask / GDAL rasterize with all_touched=False mean by "inside") and applied before polygonisation
(raster_to_polygons(zone=...)), and the tile loop may skip the tiles that hold no zone pixel (run_inference with
``skip_tiles_outside_zone``).

A zone given in another CRS than the raster's is reprojected first, vertex by vertex with straight edges kept, exactly
what ``gdf_geozone.to_crs(config.input_crs)`` does in the reference (inference.py:249): ``reproject_zone`` and the
``zone_crs`` argument of ``zone_mask`` (one ffa_crs_transform_f64 pass over all vertices, crs.py for the supported
systems).  Without a ``zone_crs`` the zone is taken to be in the CRS of the raster, as before.
"""
from __future__ import annotations

import json
import logging
import os
from typing import List, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

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


def _one_zone(obj) -> Rings:
    """every ring of a geometry (or bounds, or anything zone_rings reads), as one zone"""
    return [r for poly in zone_rings(obj) for r in poly]


def _collect_features(geozone, out: List[Tuple[dict, Rings]]) -> None:
    if hasattr(geozone, "__geo_interface__"):
        geozone = dict(geozone.__geo_interface__)
    if isinstance(geozone, (str, os.PathLike)):
        path = os.fspath(geozone)
        if not str(path).lower().endswith((".geojson", ".json")):
            raise ValueError(f"zone: {path!r} is not a .geojson / .json file")
        with open(path, "r", encoding="utf-8") as f:
            geozone = json.load(f)
    if isinstance(geozone, dict):
        kind = geozone.get("type")
        if kind == "FeatureCollection":
            for f in geozone.get("features", []):
                _collect_features(f, out)
        elif kind == "Feature":
            geom = geozone.get("geometry")
            if geom is None:
                raise ValueError("zone: GeoJSON Feature without a geometry")
            if geom.get("type") not in ("Polygon", "MultiPolygon"):
                raise ValueError(f"zone: a zone Feature needs a Polygon or MultiPolygon, got {geom.get('type')!r}")
            out.append((dict(geozone.get("properties") or {}), _one_zone(geom)))
        else:  # a bare geometry; a type that is not polygonal raises in zone_rings
            out.append(({}, _one_zone(geozone)))
    elif _is_bounds(geozone):
        out.append(({}, _one_zone(geozone)))
    elif isinstance(geozone, Sequence) and not isinstance(geozone, bytes):
        for g in geozone:
            _collect_features(g, out)
    else:
        raise ValueError(f"zone: cannot read zones from {type(geozone).__name__}")


def zone_features(geozone) -> List[Tuple[dict, Rings]]:
    """The zones of a zone layer as (properties, rings) pairs, the rings float64 [n, 2] in map coordinates as given.
    A GeoJSON Feature with a Polygon or MultiPolygon is one zone with its properties: the rings of all parts of a
    MultiPolygon together (parts of a valid MultiPolygon do not overlap, so even-odd over all of them is their union).
    A FeatureCollection is its Features in order.  A bare geometry or a (left, bottom, right, top) tuple is one zone
    with empty properties; paths to .geojson / .json files and objects with ``__geo_interface__`` are read first;
    sequences concatenate.  Anything that is not polygonal raises ValueError.  ``zone_rings`` reads the same inputs as
    one contour and stays as it is."""
    out: List[Tuple[dict, Rings]] = []
    _collect_features(geozone, out)
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


def _load_geojson(geozone):
    """the GeoJSON dict behind a dict or a .geojson / .json path, else None"""
    if isinstance(geozone, dict):
        return geozone
    if isinstance(geozone, (str, os.PathLike)) and str(os.fspath(geozone)).lower().endswith((".geojson", ".json")):
        with open(os.fspath(geozone), "r", encoding="utf-8") as f:
            return json.load(f)
    return None


def detect_zone_crs(geozone) -> str:
    """'EPSG:NNNN' of a GeoJSON dict or file (``zone_crs="auto"``): the legacy ``crs`` member when there is one
    (``urn:ogc:def:crs:EPSG::NNNN``, ``EPSG:NNNN``, ``urn:ogc:def:crs:OGC:1.3:CRS84`` = 4326), else EPSG:4326 as RFC 7946
    defines GeoJSON.  Anything that is not GeoJSON, or a member that names no EPSG code, raises ValueError."""
    obj = _load_geojson(geozone)
    if obj is None:
        raise ValueError(f"zone: zone_crs='auto' reads the CRS of a GeoJSON dict or a .geojson / .json file, not of "
                         f"{type(geozone).__name__}; name the CRS instead")
    member = obj.get("crs")
    if member is None:
        return "EPSG:4326"
    name = member.get("properties", {}).get("name") if isinstance(member, dict) else None
    if not isinstance(name, str):
        raise ValueError(f"zone: cannot read a CRS name from the GeoJSON crs member {member!r}")
    tail = name.strip().upper()
    if tail in ("URN:OGC:DEF:CRS:OGC:1.3:CRS84", "URN:OGC:DEF:CRS:OGC::CRS84", "OGC:CRS84", "CRS84"):
        return "EPSG:4326"
    if tail.startswith("URN:OGC:DEF:CRS:EPSG:"):
        tail = "EPSG:" + tail.split(":")[-1]
    if tail.startswith("EPSG:") and tail[5:].isdigit():
        return tail
    raise ValueError(f"zone: the GeoJSON crs member names {name!r}, which is no EPSG code")


def reproject_zone(geozone, src_crs, dst_crs) -> dict:
    """The zone in ``dst_crs`` as a GeoJSON MultiPolygon dict (no ``crs`` member).  Vertices are transformed one by one
    and edges stay straight -- what GeoDataFrame.to_crs does; ring count, ring order, vertex count and closedness are
    kept.  All rings go through one ops.reproject_points call.  A vertex without an image (a latitude beyond 90
    degrees, say) raises ValueError."""
    from flairhip import ops
    polys = zone_rings(geozone)
    rings = [r for poly in polys for r in poly]
    if not rings:
        return {"type": "MultiPolygon", "coordinates": []}
    xy = np.ascontiguousarray(np.concatenate(rings), dtype=np.float64)
    out = np.asarray(ops.reproject_points(xy, src_crs, dst_crs))
    if out.shape != xy.shape or not np.all(np.isfinite(out)):
        raise ValueError(f"zone: a vertex of the zone has no image in {dst_crs} (is the zone really in {src_crs}?)")
    coords, k = [], 0
    for poly in polys:
        new = []
        for r in poly:
            new.append(out[k:k + len(r)].tolist())
            k += len(r)
        coords.append(new)
    return {"type": "MultiPolygon", "coordinates": coords}


_lonlat_warned = False


def _warn_if_lonlat(geozone, raster_crs) -> None:
    """one warning per process: a zone without a CRS whose coordinates all look like degrees, on a projected raster"""
    global _lonlat_warned
    if _lonlat_warned or raster_crs is None:
        return
    from flair_zonal_detection import crs
    try:
        if crs.parse(raster_crs).is_geographic:
            return
        polys = zone_rings(geozone)
    except ValueError:
        return
    if not polys:
        return
    pts = np.concatenate([r for rings in polys for r in rings])
    if np.all(np.abs(pts[:, 0]) <= 180.0) and np.all(np.abs(pts[:, 1]) <= 90.0):
        _lonlat_warned = True
        logger.warning("the zone looks like lon/lat (all coordinates within [-180, 180] x [-90, 90]) but the raster is "
                       "in %s; pass zone_crs (e.g. 'EPSG:4326', or 'auto' for GeoJSON) to reproject it", raster_crs)


def zone_in_raster_crs(geozone, zone_crs, raster_crs):
    """The geozone as the raster's CRS sees it.  ``zone_crs`` None: the zone itself (it is taken to be in the raster's
    CRS; nothing is launched).  A CRS (anything crs.parse accepts) or "auto" (GeoJSON dicts and files, detect_zone_crs):
    the zone reprojected to ``raster_crs``, or the zone itself when the two are the same.  A ``zone_crs`` with a raster
    whose CRS is unknown or unsupported raises ValueError."""
    if geozone is None:
        return None
    if zone_crs is None:
        _warn_if_lonlat(geozone, raster_crs)
        return geozone
    from flair_zonal_detection import crs
    from flair_zonal_detection.gpkg import epsg_code
    if isinstance(zone_crs, str) and zone_crs.strip().lower() == "auto":
        zone_crs = detect_zone_crs(geozone)
    src = crs.parse(zone_crs)
    if not isinstance(raster_crs, crs.CrsParams) and epsg_code(raster_crs) is None:
        raise ValueError(f"zone: a zone_crs ({src}) needs a raster with a recognisable CRS to reproject to, got "
                         f"{raster_crs!r}")
    dst = crs.parse(raster_crs)
    if crs.same(src, dst):
        return geozone
    return reproject_zone(geozone, src, dst)


def zone_mask(geozone, left: float, top: float, xres: float, yres: float, H: int, W: int, zone_crs=None,
              raster_crs=None):
    """Device uint8 [H, W] inside mask of the zone on the north-up grid whose pixel (r, c) has its centre at
    (left + (c + 0.5) xres, top - (r + 0.5) yres): 1 where that centre is inside the zone.  Each polygon is filled
    even-odd over its rings (holes) and the polygons are united, like unary_union in the fork.  ``zone_crs`` None:
    the zone is in the CRS of the grid, as it always was.  Otherwise the zone is in ``zone_crs`` (a CRS, or "auto")
    and is reprojected to ``raster_crs``, the CRS of the grid, first (zone_in_raster_crs)."""
    import torch
    from flairhip import ops
    if not (xres > 0 and yres > 0):
        raise ValueError(f"zone_mask: positive pixel sizes expected, got {(xres, yres)}")
    polys = zone_rings(zone_in_raster_crs(geozone, zone_crs, raster_crs))
    mask = None
    for rings in polys:
        pix, offsets = rings_to_pixels(rings, left, top, xres, yres)
        mask = ops.rasterize_zone(pix, offsets, H, W, out=mask, accumulate=mask is not None)
    if mask is None:
        mask = torch.zeros((int(H), int(W)), dtype=torch.uint8, device="cuda")
    return mask
