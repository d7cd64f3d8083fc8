"""Reprojection on the GPU (csrc/crs_transform.hip through ops.reproject_points, zone.reproject_zone / zone_mask(zone_crs=),
raster_to_polygons(target_crs=), PolygonFrame.to_crs, run_inference(geozone_crs=)).

The oracle is written here in mpmath (40 digits) and shares no formula with the product where that matters:

  * Lambert conformal conic: the EPSG Guidance Note 7-2 definition of method 9802 with t = tan(pi/4 - lat/2) /
    ((1 - e sin lat) / (1 + e sin lat))^(e/2) (the product works through the isometric latitude and exp / log).
  * Transverse Mercator: no Krueger series.  The defining property  northing + i (easting - FE) = k0 M(lat_c)  with
    psi(lat_c) = psi(lat) + i dlon, where psi(lat) = asinh(tan lat) - e atanh(e sin lat) is the isometric latitude and
    M(lat) = integral of a (1 - e^2) (1 - e^2 sin^2 t)^(-3/2) dt from 0 the meridian arc, continued analytically:
    mp.findroot from lat + i dlon cos lat, mp.quad for M.

Only forward (geodetic -> projected) oracles exist.  An inverse is checked by feeding the kernel the oracle's projected
point rounded to float64 and comparing with the geodetic point it came from: the rounding moves the input by at most
half an ulp, 4.7e-10 m at 6.6e6 m or 4.2e-15 degrees, 2000 times below the bounds.  Projected -> projected likewise.

Bounds (set by the issue, not by what the kernel reaches): |d| <= 1e-6 m in projected coordinates, <= 1e-11 degrees in
geographic ones.  float64 has an ulp of 9.3e-10 m at 6.6e6 m; a numpy float64 transcription of the conic agreed with
mpmath to 2.8e-9 m and its inverse round trip to 3.6e-14 degrees, which leaves ~350x for the device math library and
the truncation of the series.  Every test prints the maxima it found before it asserts.
"""
import copy
import logging
import os
import re
import sqlite3

import mpmath as mp
import numpy as np
import pytest
import torch

from helpers import TASK

pytestmark = pytest.mark.gpu

mp.mp.dps = 40
TOL_M = 1e-6
TOL_DEG = 1e-11


# ---- oracle ------------------------------------------------------------------------------------------------------------

def _ellipsoid(p):
    a = mp.mpf(p.a)
    f = 1 / mp.mpf(p.inv_flattening)
    return a, mp.sqrt(f * (2 - f))


def oracle_lcc(p, lon_deg, lat_deg):
    """EPSG 9802, forward, mpmath"""
    a, e = _ellipsoid(p)
    rad = mp.pi / 180

    def m(lat):
        return mp.cos(lat) / mp.sqrt(1 - (e * mp.sin(lat)) ** 2)

    def t(lat):
        return mp.tan(mp.pi / 4 - lat / 2) / ((1 - e * mp.sin(lat)) / (1 + e * mp.sin(lat))) ** (e / 2)

    l0, l1, l2 = (mp.mpf(v) * rad for v in (p.lat0, p.lat1, p.lat2))
    n = (mp.log(m(l1)) - mp.log(m(l2))) / (mp.log(t(l1)) - mp.log(t(l2)))
    F = m(l1) / (n * t(l1) ** n)
    r0 = a * F * t(l0) ** n
    r = a * F * t(mp.mpf(lat_deg) * rad) ** n
    theta = n * (mp.mpf(lon_deg) - mp.mpf(p.lon0)) * rad
    return mp.mpf(p.false_easting) + r * mp.sin(theta), mp.mpf(p.false_northing) + r0 - r * mp.cos(theta)


def oracle_tmerc(p, lon_deg, lat_deg):
    """the defining property of the (Gauss-Krueger) transverse Mercator projection, forward, mpmath; lat0 = 0"""
    assert p.lat0 == 0.0
    a, e = _ellipsoid(p)
    rad = mp.pi / 180
    lat, dlon = mp.mpf(lat_deg) * rad, (mp.mpf(lon_deg) - mp.mpf(p.lon0)) * rad

    def psi(v):
        return mp.asinh(mp.tan(v)) - e * mp.atanh(e * mp.sin(v))

    target = psi(lat) + 1j * dlon
    lat_c = mp.findroot(lambda v: psi(v) - target, mp.mpc(lat, dlon * mp.cos(lat)))
    arc = mp.quad(lambda v: a * (1 - e * e) * (1 - (e * mp.sin(v)) ** 2) ** mp.mpf(-1.5), [0, lat_c])
    z = mp.mpf(p.k0) * arc
    return mp.mpf(p.false_easting) + z.imag, mp.mpf(p.false_northing) + z.real


def oracle_project(code, lonlat):
    """float64 [N, 2] oracle image of geodetic points (degrees) in the projected CRS ``code``, rounded once"""
    from flair_zonal_detection import crs
    p = crs.parse(code)
    fn = oracle_lcc if p.kind == crs.LCC2SP else oracle_tmerc
    return np.array([[float(v) for v in fn(p, lon, lat)] for lon, lat in lonlat], dtype=np.float64)


def _domain_points(seed, lon, lat, n, extra=()):
    g = np.random.default_rng(seed)
    pts = np.stack([g.uniform(*lon, n), g.uniform(*lat, n)], axis=1)
    return np.concatenate([np.asarray(extra, dtype=np.float64).reshape(-1, 2), pts])


# geodetic test points per projected CRS (the issue's domains; <= 40 points each)
DOMAINS = {
    2154: lambda: _domain_points(1, (-5.5, 10.0), (41.0, 51.5), 30, [(3.0, 46.5), (-5.5, 41.0), (10.0, 51.5)]),
    3946: lambda: _domain_points(2, (-5.5, 10.0), (44.5, 47.5), 12, [(3.0, 46.0)]),
    # UTM 20N (RGAF09, lon0 -63): +-3.5 degrees, |lat| <= 80; Guadeloupe / Martinique first
    5490: lambda: _domain_points(3, (-66.5, -59.5), (-80.0, 80.0), 20, [(-61.5, 16.2), (-61.0, 14.6), (-63.0, 0.0),
                                                                         (-59.5, 80.0), (-66.5, 0.0)]),
    # UTM 40S (RGR92, lon0 57, false northing 10 000 000); La Reunion first
    2975: lambda: _domain_points(4, (53.5, 60.5), (-80.0, 80.0), 20, [(55.5, -21.1), (57.0, 0.0), (60.5, -80.0)]),
    # UTM 31N points that also lie in Lambert-93's domain: the projected -> projected pair
    32631: lambda: _domain_points(5, (-0.5, 6.5), (41.0, 51.5), 18, [(3.0, 46.5), (0.0, 48.0)]),
}


@pytest.fixture(scope="module")
def reference():
    """{code: (lonlat float64 [N, 2], projected float64 [N, 2])}, evaluated once for the module, read-only"""
    out = {}
    for code, make in DOMAINS.items():
        lonlat = make()
        xy = oracle_project(code, lonlat)
        lonlat.setflags(write=False)
        xy.setflags(write=False)
        out[code] = (lonlat, xy)
    lonlat = out[32631][0]
    xy = oracle_project(2154, lonlat)
    xy.setflags(write=False)
    out["32631->2154"] = (lonlat, xy)
    return out


def gpu(xy, src, dst, **kw):
    from flairhip import ops
    out = ops.reproject_points(torch.from_numpy(np.array(xy, dtype=np.float64)).cuda(), src, dst, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def max_abs(a, b, what):
    d = float(np.abs(np.asarray(a) - np.asarray(b)).max())
    print(f"{what}: max |d| = {d:.3e}")
    return d


# ---- 1. the oracle itself ----------------------------------------------------------------------------------------------

def test_oracle_fixed_points():
    """by definition: the origin of Lambert-93 maps to its false origin; UTM: the equator on the central meridian"""
    from flair_zonal_detection import crs
    e, n = oracle_lcc(crs.parse(2154), 3.0, 46.5)
    assert abs(e - 700000) < mp.mpf(10) ** -25 and abs(n - 6600000) < mp.mpf(10) ** -25
    e, n = oracle_tmerc(crs.parse(2975), 57.0, 0.0)
    assert abs(e - 500000) < mp.mpf(10) ** -25 and abs(n - 10000000) < mp.mpf(10) ** -25
    # on the central meridian the northing is k0 times the meridian arc, a real integral
    p = crs.parse(32631)
    a, ecc = _ellipsoid(p)
    arc = mp.quad(lambda v: a * (1 - ecc ** 2) * (1 - (ecc * mp.sin(v)) ** 2) ** mp.mpf(-1.5), [0, mp.pi / 4])
    e, n = oracle_tmerc(p, 3.0, 45.0)
    assert abs(e - 500000) < mp.mpf(10) ** -25 and abs(n - mp.mpf(p.k0) * arc) < mp.mpf(10) ** -25


# ---- 2. accuracy, each required pair, forward and inverse -----------------------------------------------------------------

PAIRS = [2154, 5490, 2975, 3946]


@pytest.mark.parametrize("code", PAIRS)
def test_forward_from_4326(cuda, reference, code):
    lonlat, want = reference[code]
    assert max_abs(gpu(lonlat, 4326, code), want, f"4326 -> {code} [m]") <= TOL_M


@pytest.mark.parametrize("code", PAIRS)
def test_inverse_to_4326(cuda, reference, code):
    lonlat, xy = reference[code]
    assert max_abs(gpu(xy, code, 4326), lonlat, f"{code} -> 4326 [deg]") <= TOL_DEG


def test_lambert93_fixed_point(cuda):
    assert max_abs(gpu([[3.0, 46.5]], "EPSG:4326", "EPSG:2154"), [[700000.0, 6600000.0]], "origin [m]") <= TOL_M
    assert max_abs(gpu([[700000.0, 6600000.0]], "EPSG:2154", "EPSG:4326"), [[3.0, 46.5]], "origin [deg]") <= TOL_DEG


def test_projected_to_projected_in_one_pass(cuda, reference):
    _, utm = reference[32631]
    _, l93 = reference["32631->2154"]
    assert max_abs(gpu(utm, 32631, 2154), l93, "32631 -> 2154 [m]") <= TOL_M
    assert max_abs(gpu(l93, 2154, 32631), utm, "2154 -> 32631 [m]") <= TOL_M


@pytest.mark.parametrize("code", PAIRS + [32631])
def test_round_trips(cuda, reference, code):
    lonlat, xy = reference[code]
    assert max_abs(gpu(gpu(lonlat, 4326, code), code, 4326), lonlat, f"4326 -> {code} -> 4326 [deg]") <= TOL_DEG
    assert max_abs(gpu(gpu(xy, code, 4326), 4326, code), xy, f"{code} -> 4326 -> {code} [m]") <= TOL_M


# ---- 3. edge shapes ------------------------------------------------------------------------------------------------------

def _many(n, seed=9):
    g = np.random.default_rng(seed)
    return np.stack([g.uniform(-5.5, 10.0, n), g.uniform(41.0, 51.5, n)], axis=1)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025])
def test_sizes_in_place_and_determinism(cuda, reference, n):
    from flairhip import ops
    pts = _many(n)
    x = torch.from_numpy(pts).cuda()
    guard = torch.full((n + 2, 2), 7.0, dtype=torch.float64, device=cuda)  # out-of-place target between two sentinels
    out = ops.reproject_points(x, 4326, 2154, out=guard[1:n + 1])
    assert out.data_ptr() == guard[1:n + 1].data_ptr() and out.shape == (n, 2)
    again = ops.reproject_points(x, 4326, 2154)
    inplace = x.clone()
    assert ops.reproject_points(inplace, 4326, 2154, out=inplace) is inplace
    torch.cuda.synchronize()
    assert x.cpu().numpy().tobytes() == pts.tobytes()                      # the input of an out-of-place call stays
    assert bool((guard[0] == 7.0).all()) and bool((guard[n + 1] == 7.0).all())
    got = out.cpu().numpy()
    assert got.tobytes() == again.cpu().numpy().tobytes() == inplace.cpu().numpy().tobytes()
    if n == 0:
        assert again is x  # nothing to do, nothing launched
        return
    # the same points one by one give the same bytes: no element depends on its position or its neighbours
    assert got[n // 2].tobytes() == gpu(pts[n // 2:n // 2 + 1], 4326, 2154).tobytes()
    # numpy in, numpy out
    host = ops.reproject_points(pts, 4326, 2154)
    assert isinstance(host, np.ndarray) and host.tobytes() == got.tobytes() and host is not pts
    # and they are right: the mpmath image of the first and the last point
    ends = pts[[0, n - 1]]
    assert max_abs(got[[0, n - 1]], oracle_project(2154, ends), f"n = {n} ends [m]") <= TOL_M


def test_bad_points_come_out_nan_and_their_neighbours_do_not_care(cuda):
    pts = _many(130, seed=10)
    clean = gpu(pts, 4326, 2154)
    bad = pts.copy()
    bad[5] = (np.nan, 45.0)
    bad[63] = (2.0, np.inf)
    bad[64] = (-np.inf, 45.0)
    bad[100] = (2.0, 91.0)
    bad[129] = (2.0, -90.5)
    rows = [5, 63, 64, 100, 129]
    got = gpu(bad, 4326, 2154)
    assert np.isnan(got[rows]).all()
    keep = np.setdiff1d(np.arange(130), rows)
    assert got[keep].tobytes() == clean[keep].tobytes()
    # projected input: non-finite coordinates
    proj = clean.copy()
    proj[7] = (np.nan, np.nan)
    proj[8] = (700000.0, np.inf)
    back = gpu(proj, 2154, 32631)
    assert np.isnan(back[[7, 8]]).all() and np.isfinite(np.delete(back, [7, 8], axis=0)).all()
    assert np.delete(back, [7, 8], axis=0).tobytes() == np.delete(gpu(clean, 2154, 32631), [7, 8], axis=0).tobytes()
    # the apex of the cone (radius 0).  With false origin (0, 0) it is the point (0, r0) for the r0 the library derives
    # in float64, which lies within a few ulp of the oracle's: of the 33 neighbours of that value exactly the one
    # with radius 0 comes out NaN, the others are points next to the pole
    import dataclasses
    from flair_zonal_detection import crs
    cone = dataclasses.replace(crs.parse(2154), false_easting=0.0, false_northing=0.0)
    r0 = float(oracle_lcc(cone, 3.0, 90.0)[1])
    ys = r0 + np.arange(-16, 17) * np.spacing(r0)
    got = gpu(np.stack([np.zeros(33), ys], axis=1), cone, 4326)
    at_apex = np.isnan(got).all(axis=1)
    assert int(at_apex.sum()) == 1 and not np.isnan(got[~at_apex]).any()
    assert np.abs(got[~at_apex, 1] - 90.0).max() < 1e-6
    # the poles themselves are finite in both projections' forward direction or NaN, never a fault
    poles = gpu([[3.0, 90.0], [3.0, -90.0]], 4326, 32631)
    assert poles.shape == (2, 2)


def test_same_crs_launches_nothing(cuda, monkeypatch):
    from flairhip import lib as L
    from flairhip import ops

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} called")

    pts = _many(10)
    x = torch.from_numpy(pts).cuda()
    monkeypatch.setattr(L, "load", lambda: NoLaunch())
    assert ops.reproject_points(x, "EPSG:2154", 2154) is x
    assert ops.reproject_points(x, 4326, 4258) is x  # geographic to geographic: the datum rule makes it the identity
    assert ops.reproject_points(pts, 32631, "EPSG:32631") is pts
    assert ops.reproject_points(x[:0], 4326, 2154).shape == (0, 2)
    out = torch.zeros_like(x)
    assert ops.reproject_points(x, 2154, 2154, out=out) is out and bool((out == x).all())
    with pytest.raises(AssertionError):
        ops.reproject_points(x, 4326, 2154)


def test_argument_errors(cuda):
    from flairhip import ops
    x = torch.zeros((4, 2), dtype=torch.float64, device=cuda)
    for bad in (x.float(), x.t(), x[:, :1], x.reshape(-1), torch.zeros((4, 3), dtype=torch.float64, device=cuda),
                np.zeros((4, 2), np.float32), np.zeros((2, 4)).T, [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            ops.reproject_points(bad, 4326, 2154)
    with pytest.raises(ValueError):
        ops.reproject_points(x, 4326, 2154, out=torch.zeros((3, 2), dtype=torch.float64, device=cuda))
    with pytest.raises(ValueError, match="3857"):
        ops.reproject_points(x, 4326, 3857)


# ---- 4. zone -------------------------------------------------------------------------------------------------------------

H0, W0, RES, LEFT, TOP = 97, 131, 0.2, 651992.4, 6860417.8


def _star(cx, cy, radii, points, phase=0.0):
    k = np.arange(2 * points)
    ang = phase + np.pi * k / points
    rad = np.where(k % 2 == 0, radii[0], radii[1])
    return np.stack([cx + rad * np.sin(ang), cy + rad * np.cos(ang)], axis=1)


def _oracle_mask(rings, H, W):
    """the definition of include/flairhip.h in numpy, as in tests/test_zone_gpu.py"""
    tog = np.zeros((H, W + 1), dtype=bool)
    rows = np.arange(H)
    yc = rows + 0.5
    for ring in rings:
        ring = np.asarray(ring, dtype=np.float64)
        for (x0, y0), (x1, y1) in zip(ring, np.roll(ring, -1, axis=0)):
            if y0 == y1:
                continue
            cross = (y0 <= yc) != (y1 <= yc)
            xc = x0 + ((yc[cross] - y0) * (x1 - x0)) / (y1 - y0)
            c0 = np.clip(np.floor(xc - 0.5) + 1, 0, W).astype(np.int64)
            np.logical_xor.at(tog, (rows[cross], c0), True)
    return np.logical_xor.accumulate(tog[:, :W], axis=1).astype(np.uint8)


def _crossing_margin(pix, H):
    """smallest distance, in pixels, of a ring's row crossings from a pixel-centre column and of its vertices from a
    pixel-centre row: beyond 1e-4 a micrometre (5e-6 pixel) cannot move a crossing over a pixel centre"""
    yc = np.arange(H) + 0.5
    margin = np.inf
    for (x0, y0), (x1, y1) in zip(pix, np.roll(pix, -1, axis=0)):
        margin = min(margin, np.abs(yc - y0).min())
        cross = (y0 <= yc) != (y1 <= yc)
        xc = x0 + ((yc[cross] - y0) * (x1 - x0)) / (y1 - y0)
        if len(xc):
            margin = min(margin, np.abs(xc - 0.5 - np.round(xc - 0.5)).min())
    return margin


@pytest.fixture(scope="module")
def lonlat_star():
    """a star like tests/test_zone_gpu.py's STAR, given in EPSG:4326 around a point of the 97 x 131 Lambert-93 raster:
    (contour in degrees, its mpmath image in Lambert-93 rounded to float64)"""
    pix = _star(63.3, 47.7, (22.0, 70.0), 7, 0.1)
    target = np.stack([LEFT + pix[:, 0] * RES, TOP - pix[:, 1] * RES], axis=1)
    # lon / lat whose Lambert-93 image is the star: Newton on the oracle from a point near the raster (Paris)
    lonlat = np.tile([2.3488, 48.8534], (len(target), 1))
    for _ in range(4):
        d = 1e-5
        here = oracle_project(2154, lonlat)
        je = (oracle_project(2154, lonlat + [d, 0.0]) - here) / d   # d(E, N) / d lon, per vertex
        jn = (oracle_project(2154, lonlat + [0.0, d]) - here) / d
        det = je[:, 0] * jn[:, 1] - jn[:, 0] * je[:, 1]
        r = target - here
        lonlat = lonlat + np.stack([(r[:, 0] * jn[:, 1] - jn[:, 0] * r[:, 1]) / det,
                                    (je[:, 0] * r[:, 1] - r[:, 0] * je[:, 1]) / det], axis=1)
    l93 = oracle_project(2154, lonlat)
    assert np.abs(l93 - target).max() < 1e-6  # the contour is tests/test_zone_gpu.py's STAR to a micrometre
    lonlat.setflags(write=False)
    l93.setflags(write=False)
    return lonlat, l93


def _geojson(ring, crs_member=None):
    g = {"type": "Polygon", "coordinates": [np.vstack([ring, ring[:1]]).tolist()]}
    if crs_member is not None:
        g["crs"] = {"type": "name", "properties": {"name": crs_member}}
    return g


def test_zone_mask_with_a_zone_crs_equals_the_premapped_contour(cuda, lonlat_star):
    from flair_zonal_detection.zone import zone_mask
    lonlat, l93 = lonlat_star
    pix = np.stack([(l93[:, 0] - LEFT) / RES, (TOP - l93[:, 1]) / RES], axis=1)
    margin = _crossing_margin(pix, H0)
    print(f"crossing margin {margin:.3e} pixel")
    assert margin > 1e-4  # so 1e-6 m = 5e-6 pixel cannot flip a pixel: every pixel is compared
    want = _oracle_mask([pix], H0, W0)
    assert 0.15 < want.mean() < 0.6 and want[0].any() and want[-1].any() and want[:, 0].any() and want[:, -1].any()
    grid = (LEFT, TOP, RES, RES, H0, W0)
    pre = zone_mask(_geojson(l93), *grid).cpu().numpy()
    assert np.array_equal(pre, want)
    got = zone_mask(_geojson(lonlat), *grid, zone_crs="EPSG:4326", raster_crs="EPSG:2154").cpu().numpy()
    assert np.array_equal(got, want)
    # auto: no crs member = RFC 7946 lon / lat; the legacy member naming the raster's CRS = nothing to do
    auto = zone_mask(_geojson(lonlat), *grid, zone_crs="auto", raster_crs="EPSG:2154").cpu().numpy()
    assert np.array_equal(auto, want)
    crs84 = zone_mask(_geojson(lonlat, "urn:ogc:def:crs:OGC:1.3:CRS84"), *grid, zone_crs="auto", raster_crs=2154)
    assert np.array_equal(crs84.cpu().numpy(), want)
    legacy = zone_mask(_geojson(l93, "urn:ogc:def:crs:EPSG::2154"), *grid, zone_crs="auto", raster_crs="EPSG:2154")
    assert np.array_equal(legacy.cpu().numpy(), want)
    # None is today's behaviour: the same bytes with and without the new arguments, whatever the raster's CRS
    assert zone_mask(_geojson(l93), *grid, zone_crs=None, raster_crs="EPSG:2154").cpu().numpy().tobytes() == pre.tobytes()
    assert not zone_mask(_geojson(lonlat), *grid).any()  # lon / lat taken for metres: the silent miss the option cures
    with pytest.raises(ValueError):
        zone_mask(_geojson(lonlat), *grid, zone_crs="EPSG:4326", raster_crs=None)


# ---- 5. raster_to_polygons(target_crs=) ------------------------------------------------------------------------------------

def _small_raster():
    cls = np.full((64, 80), 7, np.uint8)
    cls[5:40, 6:50] = 2
    cls[15:25, 20:35] = 7     # a hole in the 2
    cls[17:22, 23:30] = 4     # an island in the hole
    cls[45:60, 10:30] = 3
    cls[50:64, 60:80] = 5     # touches the raster's corner
    cls[1:4, 66:78] = 2
    return cls


def test_raster_to_polygons_in_a_target_crs(cuda, tmp_path):
    from flair_zonal_detection.gpkg import parse_blob
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls = _small_raster()
    conf = np.random.default_rng(11).integers(0, 256, cls.shape).astype(np.uint8)
    ras = ArrayRaster(cls[None], LEFT, TOP, RES, "EPSG:2154")
    cras = ArrayRaster(conf[None], LEFT, TOP, RES, "EPSG:2154")
    kw = dict(background_value=7, confidence=cras)
    plain = raster_to_polygons(ras, **kw)
    got = raster_to_polygons(ras, target_crs="EPSG:4326", **kw)
    assert len(plain) == 5 and list(got.columns) == list(plain.columns)
    assert str(plain.crs) == "EPSG:2154" and str(got.crs) == "EPSG:4326"
    for col in ("class_id", "pixels", "confidence"):
        assert got[col].to_numpy().tobytes() == plain[col].to_numpy().tobytes(), col

    def rings(g):
        return [np.asarray(g.exterior)] + [np.asarray(r) for r in g.interiors]

    holes = 0
    worst = 0.0
    for ga, gb in zip(got["geometry"], plain["geometry"]):
        ra, rb = rings(ga), rings(gb)
        assert [len(r) for r in ra] == [len(r) for r in rb]
        holes += len(ra) - 1
        for a, b in zip(ra, rb):
            # b is Lambert-93: its inverse image is checked through the forward oracle (see the module docstring)
            worst = max(worst, float(np.abs(oracle_project(2154, a[:-1]) - b[:-1]).max()))
        # area and bounds come from the transformed coordinates
        ext = ra[0]
        assert ga.bounds == (ext[:, 0].min(), ext[:, 1].min(), ext[:, 0].max(), ext[:, 1].max())
        assert 0.0 < ga.area < 1e-6  # square degrees
    print(f"polygon vertices: max |d| = {worst:.3e} m")
    assert holes == 1 and worst <= TOL_M
    # PolygonFrame.to_crs of the untransformed frame: a new frame with the same bytes, the old one untouched
    if hasattr(plain, "_constructor") and type(plain).__name__ == "PolygonFrame":
        moved = plain.to_crs("EPSG:4326")
        assert moved is not plain and str(plain.crs) == "EPSG:2154" and str(moved.crs) == "EPSG:4326"
        for ga, gb in zip(moved["geometry"], got["geometry"]):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(rings(ga), rings(gb)))
        assert moved["confidence"].to_numpy().tobytes() == plain["confidence"].to_numpy().tobytes()
    # GeoPackage: one 4326 row, blobs in 4326, envelopes from the ring coordinates
    path = str(tmp_path / "p.gpkg")
    got.to_file(path, driver="GPKG")
    con = sqlite3.connect(path)
    try:
        assert con.execute("SELECT COUNT(*) FROM gpkg_spatial_ref_sys WHERE srs_id = 4326").fetchone()[0] == 1
        assert con.execute("SELECT COUNT(*) FROM gpkg_spatial_ref_sys").fetchone()[0] == 3
        table, srs = con.execute("SELECT table_name, srs_id FROM gpkg_contents").fetchone()
        assert srs == 4326 and con.execute("SELECT srs_id FROM gpkg_geometry_columns").fetchone()[0] == 4326
        blobs = [r[0] for r in con.execute(f'SELECT geom FROM "{table}" ORDER BY fid')]
    finally:
        con.close()
    assert len(blobs) == len(got)
    for blob, g in zip(blobs, got["geometry"]):
        srs_id, env, brings = parse_blob(blob)
        ext = rings(g)[0]
        assert srs_id == 4326 and all(x.tobytes() == y.tobytes() for x, y in zip(brings, rings(g)))
        assert env == (ext[:, 0].min(), ext[:, 0].max(), ext[:, 1].min(), ext[:, 1].max())
    # the raster's own CRS as the target changes nothing
    same = raster_to_polygons(ras, target_crs=2154, **kw)
    for ga, gb in zip(same["geometry"], plain["geometry"]):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(rings(ga), rings(gb)))
    with pytest.raises(ValueError):
        raster_to_polygons(ArrayRaster(cls[None], LEFT, TOP, RES, None), target_crs=4326, **kw)


# ---- 6. run_inference(geozone_crs=) ------------------------------------------------------------------------------------------

def test_run_inference_with_a_lonlat_zone_drops_the_same_tiles(cuda, tmp_path, caplog):
    """the smallest geometry of tests/test_zone_gpu.py (200 x 260 pixels, 128-pixel tiles, 3 x 3 grid) and its L zone,
    once in Lambert-93 and once as the kernel's own EPSG:4326 image of it"""
    import yaml
    from flair_zonal_detection.inference import run_inference
    from flair_zonal_detection.raster import ArrayRaster
    from flairhip import ops
    from helpers import MOD, ROOT, oracle_to_product_keys
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(1, 255, (3, 200, 260)).astype(np.uint8), LEFT, TOP, RES)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "tests", "golden", "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp_path), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": 0.2, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}, "skip_tiles_outside_zone": True})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    oracle = UnetResNet34(3, 19)
    sd = fill_state_dict(oracle.state_dict(), seed=5)
    sd["segmentation_head.0.bias"] = sd["segmentation_head.0.bias"] + torch.linspace(0, 3, 19)  # class 0 = never written
    oracle.load_state_dict(sd)
    cfg["model_weights"] = str(tmp_path / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    b = ras.bounds
    x0, x1, x2 = b.left - 3.0, b.left + 50.3 * 0.2, b.right + 3.0
    y0, y1, y2 = b.bottom - 3.0, b.bottom + 40.6 * 0.2, b.top + 3.0
    ring = np.array([[x0, y0], [x2, y0], [x2, y1], [x1, y1], [x1, y2], [x0, y2]])
    zone = _geojson(ring)
    zone_ll = _geojson(ops.reproject_points(ring, 2154, 4326))

    def run(z, **kw):
        caplog.clear()
        with caplog.at_level(logging.INFO, logger="flair_zonal_detection.inference"):
            out = run_inference(copy.deepcopy(cfg), geozone=z, **kw)
        logged = [re.search(r"(\d+) of (\d+) tiles outside the zone skipped", r.getMessage()) for r in caplog.records]
        logged = [m for m in logged if m]
        assert len(logged) == 1
        return out[TASK].data, (int(logged[0].group(1)), int(logged[0].group(2)))

    want, dropped = run(zone)
    assert dropped[1] == 9 and 0 < dropped[0] < 9 and not want.all()
    got, dropped_ll = run(zone_ll, geozone_crs="EPSG:4326")
    assert dropped_ll == dropped
    assert np.array_equal(got == 0, want == 0)  # the same tiles were never written
    assert got.tobytes() == want.tobytes()
    # the config key does what the argument does
    cfg["geozone_crs"] = "EPSG:4326"
    got2, dropped2 = run(zone_ll)
    assert dropped2 == dropped and got2.tobytes() == want.tobytes()
