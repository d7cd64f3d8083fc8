"""GeoPackage writer for polygon layers (OGC GeoPackage 1.2 encoding standard, Python's sqlite3 only, no GDAL).

The reference writes its polygons with ``gdf.to_file(path, driver="GPKG")`` (GDAL / OGR).  This module writes the
same kind of file from the flat polygon arrays of ``raster_to_polygons``:

  * ``PRAGMA application_id`` = 0x47504B47 ("GPKG"), ``PRAGMA user_version`` = 10200 (version 1.2.0)
  * ``gpkg_spatial_ref_sys`` with the three mandatory rows (-1 undefined Cartesian, 0 undefined geographic, 4326
    WGS 84) plus one row for the layer's EPSG code (none for 4326: polygons reprojected to EPSG:4326 use the mandatory
    row), ``gpkg_contents``, ``gpkg_geometry_columns``
  * one feature table: ``fid`` INTEGER PRIMARY KEY, ``geom`` POLYGON, ``class_id`` INTEGER, then the optional extra
    attribute columns (``REAL`` for float values, ``INTEGER`` for int values; e.g. ``confidence``, ``pixels``)
  * geometry blobs: the GeoPackage header ("GP", version 0, flags = little endian + [minx, maxx, miny, maxy] envelope,
    srs_id) followed by little-endian WKB (Polygon, rings closed)

The row of the raster's CRS carries organization "EPSG", the code, and the definition "undefined" -- nothing here
produces WKT.  That GDAL resolves such a row to the CRS through its EPSG code has NOT been verified (no GDAL in the
build image).  The file is deterministic: the same polygons give the same bytes (``last_change`` is a fixed time).
"""
from __future__ import annotations

import os
import sqlite3
import struct
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

APPLICATION_ID = 0x47504B47
USER_VERSION = 10200
LAST_CHANGE = "1970-01-01T00:00:00.000Z"

_WGS84_WKT = ('GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563,AUTHORITY["EPSG","7030"]],'
              'AUTHORITY["EPSG","6326"]],PRIMEM["Greenwich",0,AUTHORITY["EPSG","8901"]],UNIT["degree",'
              '0.0174532925199433,AUTHORITY["EPSG","9122"]],AXIS["Latitude",NORTH],AXIS["Longitude",EAST],'
              'AUTHORITY["EPSG","4326"]]')

_SCHEMA = """
CREATE TABLE gpkg_spatial_ref_sys (srs_name TEXT NOT NULL, srs_id INTEGER NOT NULL PRIMARY KEY,
  organization TEXT NOT NULL, organization_coordsys_id INTEGER NOT NULL, definition TEXT NOT NULL, description TEXT);
CREATE TABLE gpkg_contents (table_name TEXT NOT NULL PRIMARY KEY, data_type TEXT NOT NULL, identifier TEXT UNIQUE,
  description TEXT DEFAULT '', last_change DATETIME NOT NULL DEFAULT (strftime('%Y-%m-%dT%H:%M:%fZ','now')),
  min_x DOUBLE, min_y DOUBLE, max_x DOUBLE, max_y DOUBLE, srs_id INTEGER,
  CONSTRAINT fk_gc_r_srs_id FOREIGN KEY (srs_id) REFERENCES gpkg_spatial_ref_sys(srs_id));
CREATE TABLE gpkg_geometry_columns (table_name TEXT NOT NULL, column_name TEXT NOT NULL,
  geometry_type_name TEXT NOT NULL, srs_id INTEGER NOT NULL, z TINYINT NOT NULL, m TINYINT NOT NULL,
  CONSTRAINT pk_geom_cols PRIMARY KEY (table_name, column_name),
  CONSTRAINT uk_gc_table_name UNIQUE (table_name),
  CONSTRAINT fk_gc_tn FOREIGN KEY (table_name) REFERENCES gpkg_contents(table_name),
  CONSTRAINT fk_gc_srs FOREIGN KEY (srs_id) REFERENCES gpkg_spatial_ref_sys (srs_id));
"""


def epsg_code(crs) -> Optional[int]:
    """EPSG code of a CRS given as 'EPSG:2154', an int, or an object with to_epsg() (rasterio / pyproj); else None."""
    if crs is None:
        return None
    if isinstance(crs, (int, np.integer)):
        return int(crs)
    if hasattr(crs, "to_epsg"):
        code = crs.to_epsg()
        return int(code) if code else None
    s = str(crs).strip()
    if s.upper().startswith("EPSG:") and s[5:].isdigit():
        return int(s[5:])
    return None


def polygon_blob(rings: Sequence[np.ndarray], srs_id: int) -> bytes:
    """GeoPackage geometry blob of one polygon; rings: float64 [n, 2] arrays, closed or not (closed on write)."""
    closed = []
    for r in rings:
        r = np.asarray(r, dtype="<f8").reshape(-1, 2)
        if len(r) and not np.array_equal(r[0], r[-1]):
            r = np.concatenate([r, r[:1]])
        closed.append(np.ascontiguousarray(r))
    if closed:
        ext = closed[0]
        env = (ext[:, 0].min(), ext[:, 0].max(), ext[:, 1].min(), ext[:, 1].max())
    else:
        env = (0.0, 0.0, 0.0, 0.0)
    head = b"GP" + struct.pack("<BBi4d", 0, 0b011, srs_id, *env)
    parts = [head, struct.pack("<BII", 1, 3, len(closed))]
    for r in closed:
        parts.append(struct.pack("<I", len(r)))
        parts.append(r.tobytes())
    return b"".join(parts)


def parse_blob(blob: bytes) -> Tuple[int, Tuple[float, ...], list]:
    """(srs_id, envelope, rings) of a blob written by polygon_blob (header flags and WKB byte order honoured)."""
    if blob[:2] != b"GP":
        raise ValueError("not a GeoPackage geometry blob")
    flags = blob[3]
    bo = "<" if flags & 1 else ">"
    srs_id = struct.unpack(bo + "i", blob[4:8])[0]
    env_n = {0: 0, 1: 4, 2: 6, 3: 6, 4: 8}[(flags >> 1) & 7]
    env = struct.unpack(bo + f"{env_n}d", blob[8:8 + 8 * env_n])
    o = 8 + 8 * env_n
    wbo = "<" if blob[o] == 1 else ">"
    gtype, nr = struct.unpack(wbo + "II", blob[o + 1:o + 9])
    if gtype != 3:
        raise ValueError(f"WKB type {gtype} is not Polygon")
    o += 9
    rings = []
    for _ in range(nr):
        n = struct.unpack(wbo + "I", blob[o:o + 4])[0]
        o += 4
        rings.append(np.frombuffer(blob, dtype=wbo + "f8", count=2 * n, offset=o).reshape(n, 2).copy())
        o += 16 * n
    return srs_id, env, rings


def _column_type(name: str, values) -> str:
    kind = np.asarray(values).dtype.kind
    if kind == "f":
        return "REAL"
    if kind in "iub":
        return "INTEGER"
    raise ValueError(f"write_polygons: column {name!r} must hold float or int values, not dtype kind {kind!r}")


def write_polygons(path: str, polygons: Iterable[Tuple[int, Sequence[np.ndarray]]], crs=None,
                   layer: Optional[str] = None, columns: Optional[dict] = None) -> str:
    """Write (class_id, rings) pairs as one POLYGON layer (default name: the file's base name, as OGR does).
    ``columns``: optional {name: values} of extra attribute columns after class_id, one value per polygon, float ->
    REAL, int -> INTEGER; without it the table is (fid, geom, class_id)."""
    columns = dict(columns or {})
    for name in columns:
        if not (isinstance(name, str) and name.isidentifier()) or name.lower() in ("fid", "geom", "class_id"):
            raise ValueError(f"write_polygons: {name!r} is not a usable attribute column name")
    types = {name: _column_type(name, v) for name, v in columns.items()}
    columns = {name: np.asarray(v).tolist() for name, v in columns.items()}  # Python float / int for sqlite3
    layer = layer or os.path.splitext(os.path.basename(path))[0]
    code = epsg_code(crs)
    srs_id = code if code is not None else -1
    if os.path.exists(path):
        os.remove(path)
    con = sqlite3.connect(path)
    try:
        con.execute(f"PRAGMA application_id = {APPLICATION_ID}")
        con.execute(f"PRAGMA user_version = {USER_VERSION}")
        con.executescript(_SCHEMA)
        srs_rows = [("Undefined cartesian SRS", -1, "NONE", -1, "undefined", "undefined cartesian coordinate reference system"),
                    ("Undefined geographic SRS", 0, "NONE", 0, "undefined", "undefined geographic coordinate reference system"),
                    ("WGS 84 geodetic", 4326, "EPSG", 4326, _WGS84_WKT, "longitude/latitude coordinates in decimal degrees on the WGS 84 spheroid")]
        if code is not None and code not in (-1, 0, 4326):
            srs_rows.append((f"EPSG:{code}", code, "EPSG", code, "undefined", None))
        con.executemany("INSERT INTO gpkg_spatial_ref_sys VALUES (?, ?, ?, ?, ?, ?)", srs_rows)
        con.execute(f'CREATE TABLE "{layer}" (fid INTEGER PRIMARY KEY AUTOINCREMENT NOT NULL, geom POLYGON, '
                    f'class_id INTEGER' + "".join(f', "{n}" {t}' for n, t in types.items()) + ')')
        bbox = [np.inf, np.inf, -np.inf, -np.inf]
        rows = []
        for fid, (cid, rings) in enumerate(polygons, start=1):
            blob = polygon_blob(rings, srs_id)
            env = struct.unpack("<4d", blob[8:40])
            bbox = [min(bbox[0], env[0]), min(bbox[1], env[2]), max(bbox[2], env[1]), max(bbox[3], env[3])]
            rows.append((fid, blob, int(cid)))
        for name, v in columns.items():
            if len(v) != len(rows):
                raise ValueError(f"write_polygons: column {name!r} has {len(v)} values for {len(rows)} polygons")
        if columns:
            rows = [r + extra for r, extra in zip(rows, zip(*columns.values()))]
        names = "".join(f', "{n}"' for n in columns)
        con.executemany(f'INSERT INTO "{layer}" (fid, geom, class_id{names}) VALUES (?, ?, ?{", ?" * len(columns)})',
                        rows)
        ext = bbox if rows else [None] * 4
        con.execute("INSERT INTO gpkg_contents VALUES (?, 'features', ?, '', ?, ?, ?, ?, ?, ?)",
                    (layer, layer, LAST_CHANGE, ext[0], ext[1], ext[2], ext[3], srs_id))
        con.execute("INSERT INTO gpkg_geometry_columns VALUES (?, 'geom', 'POLYGON', ?, 0, 0)", (layer, srs_id))
        con.commit()
    finally:
        con.close()
    return path
