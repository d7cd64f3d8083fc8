"""Coordinate reference systems by EPSG code, without pyproj: the parameter table behind ops.reproject_points.

The reference reprojects with geopandas (``gdf_geozone.to_crs(config.input_crs)``, inference.py:249;
``clean_results_gdf.to_crs(target_crs)``, scripts/run_fast_aigle_segmentation.py:165).  Here a CRS is the small
parameter set of include/flairhip.h's FfaCrs -- geographic, Lambert conformal conic with two standard parallels
(EPSG method 9802) or transverse Mercator (EPSG method 9807) on GRS80 or WGS 84 -- and the projections themselves run
on the GPU (csrc/crs_transform.hip).  The parameter values are those of the EPSG registry.

Datum rule: geodetic longitude and latitude are carried across unchanged between the supported datums (the registry's
RGF93 / ETRS89 / RGAF09 / RGR92 / RGFG95 / RGM04 / RGSPM06 -> WGS 84 operations are null transformations); each
projection uses the ellipsoid of its own CRS.
"""
from __future__ import annotations

from dataclasses import dataclass

from flair_zonal_detection.gpkg import epsg_code

GEOGRAPHIC, LCC2SP, TMERC = 0, 1, 2  # FFA_CRS_*

GRS80 = (6378137.0, 298.257222101)
WGS84 = (6378137.0, 298.257223563)

SUPPORTED = ("geographic 4326 / 4171 / 4258; Lambert-93 2154; RGF93 CC42-CC50 3942-3950; WGS 84 UTM 32601-32660 and "
             "32701-32760; ETRS89 UTM 25828-25838; GRS80 UTM 5490, 2972, 4467, 2975, 4471")


@dataclass(frozen=True)
class CrsParams:
    epsg: int
    kind: int
    a: float
    inv_flattening: float
    lon0: float = 0.0
    lat0: float = 0.0
    lat1: float = 0.0
    lat2: float = 0.0
    k0: float = 1.0
    false_easting: float = 0.0
    false_northing: float = 0.0

    @property
    def is_geographic(self) -> bool:
        return self.kind == GEOGRAPHIC

    def parameters(self) -> tuple:
        """everything but the code: what a transform depends on"""
        return (self.kind, self.a, self.inv_flattening, self.lon0, self.lat0, self.lat1, self.lat2, self.k0,
                self.false_easting, self.false_northing)

    def __str__(self) -> str:
        return f"EPSG:{self.epsg}"


def _utm(code: int, ellipsoid, zone: int, south: bool) -> CrsParams:
    return CrsParams(code, TMERC, *ellipsoid, lon0=6.0 * zone - 183.0, lat0=0.0, k0=0.9996, false_easting=500000.0,
                     false_northing=10000000.0 if south else 0.0)


# UTM zones on GRS80 of the overseas departments: RGAF09 20N, RGFG95 22N, RGSPM06 21N, RGR92 40S, RGM04 38S
_GRS80_UTM = {5490: (20, False), 2972: (22, False), 4467: (21, False), 2975: (40, True), 4471: (38, True)}


def from_epsg(code: int) -> CrsParams:
    code = int(code)
    if code == 4326:
        return CrsParams(code, GEOGRAPHIC, *WGS84)
    if code in (4171, 4258):
        return CrsParams(code, GEOGRAPHIC, *GRS80)
    if code == 2154:
        return CrsParams(code, LCC2SP, *GRS80, lon0=3.0, lat0=46.5, lat1=49.0, lat2=44.0, false_easting=700000.0,
                         false_northing=6600000.0)
    if 3942 <= code <= 3950:
        zone = code - 3900
        return CrsParams(code, LCC2SP, *GRS80, lon0=3.0, lat0=float(zone), lat1=zone - 0.75, lat2=zone + 0.75,
                         false_easting=1700000.0, false_northing=(zone - 41) * 1000000.0 + 200000.0)
    if 32601 <= code <= 32660:
        return _utm(code, WGS84, code - 32600, False)
    if 32701 <= code <= 32760:
        return _utm(code, WGS84, code - 32700, True)
    if 25828 <= code <= 25838:
        return _utm(code, GRS80, code - 25800, False)
    if code in _GRS80_UTM:
        return _utm(code, GRS80, *_GRS80_UTM[code])
    raise ValueError(f"crs: EPSG:{code} is not supported (supported: {SUPPORTED})")


def parse(crs) -> CrsParams:
    """CrsParams of 'EPSG:2154', an int, or an object with to_epsg() (rasterio / pyproj); a CrsParams passes through.
    Anything without an EPSG code, or a code outside the table, raises ValueError: there is no silent identity."""
    if isinstance(crs, CrsParams):
        return crs
    if isinstance(crs, bool):
        raise ValueError(f"crs: {crs!r} names no CRS")
    code = epsg_code(crs)
    if code is None:
        raise ValueError(f"crs: no EPSG code in {crs!r} ('EPSG:2154', an int or an object with to_epsg() expected; "
                         f"supported: {SUPPORTED})")
    return from_epsg(code)


def same(a, b) -> bool:
    """True when a transform between the two is the identity, so nothing needs to be launched: equal parameter sets,
    or two geographic CRSs (the datum rule carries longitude and latitude across unchanged)."""
    a, b = parse(a), parse(b)
    return a.parameters() == b.parameters() or (a.is_geographic and b.is_geographic)
