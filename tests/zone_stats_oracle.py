"""The oracle of the zonal-statistics tests (tests/test_zone_stats_gpu.py, tests/test_zone_stats_cpu.py): the inside
mask of include/flairhip.h restated in numpy, operation for operation -- ``oracle_mask`` as tests/test_zone_gpu.py
writes it --, applied zone by zone, then np.bincount.  Also the zone shapes those tests share.  No GPU."""
import numpy as np


def oracle_mask(rings, H, W):
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
            np.logical_xor.at(tog, (rows[cross], c0), True)  # a toggle at column W falls off the mask
    return np.logical_xor.accumulate(tog[:, :W], axis=1).astype(np.uint8)


def oracle_masks(zones, H, W):
    """bool [Z, H, W]: the mask of every zone (a zone = a list of rings; no ring = nothing inside)"""
    return np.stack([oracle_mask(rings, H, W).astype(bool) for rings in zones]) if len(zones) else np.zeros((0, H, W), bool)


def oracle_stats(cls, conf, masks, K):
    """(counts, conf_sums) int64 [Z, K + 1] from the masks: bincount of the member pixels' classes with the values
    >= K folded into column K, and the same with the confidence bytes as int64 weights (exact: integer sums well
    below 2^53).  conf None: conf_sums is None."""
    folded = np.minimum(cls.astype(np.int64), K)
    counts = np.zeros((len(masks), K + 1), np.int64)
    sums = np.zeros((len(masks), K + 1), np.int64)
    for z, m in enumerate(masks):
        counts[z] = np.bincount(folded[m], minlength=K + 1)
        if conf is not None:
            sums[z] = np.bincount(folded[m], weights=conf[m].astype(np.int64), minlength=K + 1).astype(np.int64)
    return counts, (sums if conf is not None else None)


def window_rule(rings, H, W):
    """(r0, c0, r1, c1) of one zone by the conservative rule of include/flairhip_zonestats.h, or None without a vertex"""
    if not len(rings):
        return None
    pts = np.concatenate([np.asarray(r, dtype=np.float64) for r in rings])
    xmin, ymin, xmax, ymax = pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max()
    r0 = int(min(max(0.0, np.floor(ymin - 0.5)), H))
    r1 = int(max(min(float(H), np.ceil(ymax - 0.5) + 1), 0))
    c0 = int(min(max(0.0, np.floor(xmin - 0.5)), W)) & ~31
    c1 = int(max(min(float(W), np.floor(xmax - 0.5) + 2), 0))
    return r0, c0, r1, c1


def star(cx, cy, radii, points, phase=0.0):
    """2 * points vertices, radii alternating from radii[0], vertex k at the angle phase + k pi / points from +y"""
    k = np.arange(2 * points)
    ang = phase + np.pi * k / points
    rad = np.where(k % 2 == 0, radii[0], radii[1])
    return np.stack([cx + rad * np.sin(ang), cy + rad * np.cos(ang)], axis=1)


H0, W0 = 97, 131  # W is no multiple of 32: 5 words per row, the last one partial
STAR = star(63.3, 47.7, (22.0, 70.0), 7, 0.1)   # sticks out of the 97 x 131 raster on all four sides
STAR_HOLE = star(60.2, 50.1, (12.0, 5.0), 5)
CENTRE_BOX = np.array([[10.5, 20.5], [30.5, 20.5], [30.5, 40.5], [10.5, 40.5]])


def random_polygons():
    g = np.random.default_rng(0)
    out = []
    for _ in range(20):
        n = int(g.integers(3, 40))
        cx, cy = g.uniform(20, 110), g.uniform(20, 80)
        ang = np.sort(g.uniform(0, 2 * np.pi, n))
        rad = g.uniform(5, 80, n)
        out.append(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1))
    return out


def base_rasters(H=H0, W=W0, seed=11):
    """(cls, conf): classes random in 0..18 with a sprinkling of 255, confidence random uint8"""
    g = np.random.default_rng(seed)
    cls = g.integers(0, 19, (H, W)).astype(np.uint8)
    cls[g.random((H, W)) < 0.03] = 255
    conf = g.integers(0, 256, (H, W)).astype(np.uint8)
    return cls, conf


def parcel_grid(H=H0, W=W0, n=24, seed=0):
    """n x n quads over shared jittered vertices: the grid linspace(-6, W + 6, n + 1) x linspace(-6, H + 6, n + 1), x
    jittered by U(-1.8, 1.8) and y by U(-1.3, 1.3), drawn X then Y; orientation alternates with (i + j) parity"""
    g = np.random.default_rng(seed)
    X, Y = np.meshgrid(np.linspace(-6, W + 6, n + 1), np.linspace(-6, H + 6, n + 1))
    X = X + g.uniform(-1.8, 1.8, X.shape)
    Y = Y + g.uniform(-1.3, 1.3, Y.shape)
    zones = []
    for i in range(n):
        for j in range(n):
            quad = np.array([[X[i, j], Y[i, j]], [X[i, j + 1], Y[i, j + 1]], [X[i + 1, j + 1], Y[i + 1, j + 1]],
                             [X[i + 1, j], Y[i + 1, j]]])
            zones.append([quad[::-1].copy() if (i + j) % 2 else quad])
    return zones
