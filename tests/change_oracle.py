"""The oracle of the land-cover change tests (tests/test_zone_change_gpu.py, tests/test_change_zonal_gpu.py): the
transition matrix of include/flairhip_change.h stated in numpy over the zone masks of tests/zone_stats_oracle.py.  Per
zone mask ``m``: np.bincount(fa[m] * (K + 1) + fb[m], minlength=(K + 1)**2) with fa = min(before, K), fb = min(after, K),
and the same with the confidence bytes as int64 weights (exact: integer sums well below 2^53).  No GPU."""
import numpy as np


def fold(raster, K):
    return np.minimum(raster.astype(np.int64), K)


def cross_tab(before, after, K, conf=None, mask=None):
    """int64 [K + 1, K + 1] over the pixels of ``mask`` (None: every pixel); with ``conf`` the sums of its bytes"""
    fa, fb = fold(before, K), fold(after, K)
    m = np.ones(before.shape, bool) if mask is None else mask
    key = fa[m] * (K + 1) + fb[m]
    if conf is None:
        return np.bincount(key, minlength=(K + 1) ** 2).reshape(K + 1, K + 1)
    return np.bincount(key, weights=conf[m].astype(np.int64), minlength=(K + 1) ** 2).astype(np.int64).reshape(K + 1, K + 1)


def oracle_change(before, after, conf, masks, K):
    """(counts, conf_sums) int64 [Z, K + 1, K + 1] from the masks; conf None: conf_sums is None"""
    counts = np.zeros((len(masks), K + 1, K + 1), np.int64)
    sums = np.zeros((len(masks), K + 1, K + 1), np.int64)
    for z, m in enumerate(masks):
        counts[z] = cross_tab(before, after, K, None, m)
        if conf is not None:
            sums[z] = cross_tab(before, after, K, conf, m)
    return counts, (sums if conf is not None else None)


def oracle_codes(before, after, lut):
    K = lut.shape[0] - 1
    return lut[np.minimum(before, K), np.minimum(after, K)]
