"""Polygon results of raster_to_polygons without geopandas / shapely.

``FlatPolygons`` holds the polygons as flat arrays (class ids, ring offsets per polygon, vertex offsets per ring,
float64 map coordinates, rings not closed).  ``PolygonFrame`` is the small pandas.DataFrame subclass returned when
geopandas is not importable: columns ``class_id`` and ``geometry`` like the reference's GeoDataFrame (plus optional
numeric attribute columns between them, e.g. ``confidence`` and ``pixels``), a ``crs`` attribute,
``to_crs(crs)`` (the flat coordinates through the GPU transform, once) and ``to_file(path, driver="GPKG")``.  Its geometry values are ``Polygon`` views that read the flat arrays
only when asked (exterior / interiors as closed float64 [n, 2] arrays, ``area``, ``wkb``).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import pandas as pd


@dataclass
class FlatPolygons:
    class_id: np.ndarray          # int32 [P]
    poly_ring_offsets: np.ndarray  # int32 [P + 1]
    ring_vertex_offsets: np.ndarray  # int32 [R + 1]
    xy: np.ndarray                # float64 [V, 2]

    def __len__(self) -> int:
        return len(self.class_id)

    def rings(self, q: int):
        r0, r1 = int(self.poly_ring_offsets[q]), int(self.poly_ring_offsets[q + 1])
        return [self.xy[self.ring_vertex_offsets[j]:self.ring_vertex_offsets[j + 1]] for j in range(r0, r1)]


def _closed(r: np.ndarray) -> np.ndarray:
    return np.concatenate([r, r[:1]]) if len(r) else r


def _shoelace(r: np.ndarray) -> float:
    x, y = r[:, 0] - r[0, 0], r[:, 1] - r[0, 1]  # about the first vertex: map coordinates are large
    return 0.5 * float(np.dot(x, np.roll(y, -1)) - np.dot(np.roll(x, -1), y))


class Polygon:
    """Minimal polygon value: exterior first, holes after (closed float64 arrays, map coordinates)."""
    __slots__ = ("_store", "_q")
    geom_type = "Polygon"

    def __init__(self, store: FlatPolygons, q: int):
        self._store, self._q = store, q

    @property
    def exterior(self) -> np.ndarray:
        return _closed(self._store.rings(self._q)[0])

    @property
    def interiors(self):
        return [_closed(r) for r in self._store.rings(self._q)[1:]]

    @property
    def is_empty(self) -> bool:
        return False

    @property
    def area(self) -> float:
        rings = self._store.rings(self._q)
        return abs(_shoelace(rings[0])) - sum(abs(_shoelace(r)) for r in rings[1:])

    @property
    def bounds(self):
        e = self._store.rings(self._q)[0]
        return (float(e[:, 0].min()), float(e[:, 1].min()), float(e[:, 0].max()), float(e[:, 1].max()))

    @property
    def wkb(self) -> bytes:
        rings = [_closed(r) for r in self._store.rings(self._q)]
        out = [struct.pack("<BII", 1, 3, len(rings))]
        for r in rings:
            out.append(struct.pack("<I", len(r)))
            out.append(np.ascontiguousarray(r, dtype="<f8").tobytes())
        return b"".join(out)

    def __repr__(self) -> str:
        rings = self._store.rings(self._q)
        return f"<Polygon: {len(rings[0])} exterior vertices, {len(rings) - 1} holes>"


class PolygonFrame(pd.DataFrame):
    """DataFrame(class_id, [numeric attribute columns,] geometry) with ``crs`` and ``to_file`` (GeoPackage only)."""
    _metadata = ["crs"]

    @property
    def _constructor(self):
        return PolygonFrame

    @classmethod
    def from_flat(cls, flat: FlatPolygons, crs=None, columns=None) -> "PolygonFrame":
        """``columns``: optional {name: array of len(flat)} of float / int attributes, placed after class_id."""
        geoms = np.empty(len(flat), dtype=object)
        for q in range(len(flat)):
            geoms[q] = Polygon(flat, q)
        data = {"class_id": flat.class_id.astype(np.int64)}
        for name, v in (columns or {}).items():
            v = np.asarray(v)
            if v.shape != (len(flat),) or v.dtype.kind not in "fiub":
                raise ValueError(f"PolygonFrame: column {name!r} needs {len(flat)} float or int values")
            data[name] = v
        data["geometry"] = geoms
        df = cls(data)
        df.crs = crs
        return df

    def to_crs(self, crs) -> "PolygonFrame":
        """A new frame in ``crs`` (anything crs.parse accepts), like GeoDataFrame.to_crs: every vertex transformed,
        edges straight, rings, order and the other columns as they are.  The flat coordinate store behind the
        geometries goes through ops.reproject_points once; ``area`` / ``bounds`` / ``wkb`` of the new geometries come
        from the transformed coordinates.  A frame without a (supported) ``crs`` raises ValueError."""
        from flairhip import ops
        from flair_zonal_detection import crs as crs_table
        if self.crs is None:
            raise ValueError("PolygonFrame.to_crs: the frame has no crs to transform from")
        src, dst = crs_table.parse(self.crs), crs_table.parse(crs)
        out = self.copy()
        out.crs = str(dst)
        if crs_table.same(src, dst):
            return out
        stores = {}
        geoms = np.empty(len(self), dtype=object)
        for i, g in enumerate(self["geometry"]):
            if not isinstance(g, Polygon):
                raise TypeError(f"PolygonFrame.to_crs: geometry {i} is {type(g).__name__}, not a polygons.Polygon")
            st = stores.get(id(g._store))
            if st is None:
                s = g._store
                xy = ops.reproject_points(np.ascontiguousarray(s.xy, dtype=np.float64), src, dst)
                st = stores[id(s)] = FlatPolygons(s.class_id, s.poly_ring_offsets, s.ring_vertex_offsets, xy)
            geoms[i] = Polygon(st, g._q)
        out["geometry"] = geoms
        return out

    def to_file(self, path: str, driver: str = "GPKG", layer=None, **_ignored) -> str:
        if str(driver).upper() != "GPKG":
            raise ValueError(f"PolygonFrame.to_file writes GeoPackage only (driver='GPKG'), not {driver!r}")
        from flair_zonal_detection.gpkg import write_polygons

        def rings_of(g):
            if isinstance(g, Polygon):
                return g._store.rings(g._q)
            return [np.asarray(g.exterior)] + [np.asarray(r) for r in g.interiors]
        extra = {c: self[c].to_numpy() for c in self.columns
                 if c not in ("class_id", "geometry") and self[c].dtype.kind in "fiub"}
        return write_polygons(path, ((int(c), rings_of(g)) for c, g in zip(self["class_id"], self["geometry"])),
                              crs=self.crs, layer=layer, **({"columns": extra} if extra else {}))
