"""Object matching (include/flairhip_objects.h, flairhip/objects.py) restated in plain numpy / Python on top of the
flood fill of tests/sieve_oracle.py: region tables, the overlap list as a dict, the head count that bounds it and the
greedy one-to-one matching.  The yardstick of tests/test_region_overlap_gpu.py and tests/test_objects_zonal_gpu.py,
itself pinned by the hand-worked cases of tests/test_objects_cpu.py.  No scipy, no call into the product."""
import numpy as np

from sieve_oracle import label


def regions(cls, background=None, min_pixels=1):
    """(index int64 [H, W]: the region index of every pixel, -1 for background and dropped regions; table: the list of
    (first_pixel, class, pixels) of the kept regions in ascending label order)"""
    cls = np.asarray(cls)
    W = cls.shape[1]
    lab, counts = label(cls, background)
    kept = sorted(root for root, n in counts.items() if n >= max(int(min_pixels), 1))
    table = [(root, int(cls[root // W, root % W]), counts[root]) for root in kept]
    lut = {root: i for i, root in enumerate(kept)}
    index = np.array([lut.get(v, -1) for v in lab.ravel().tolist()], np.int64).reshape(lab.shape)
    return index, table


def overlaps(index_a, index_b):
    """{(ia, ib): shared pixels} over the pixels that lie in a kept region of both"""
    out = {}
    both = (index_a >= 0) & (index_b >= 0)
    for key in zip(index_a[both].tolist(), index_b[both].tolist()):
        out[key] = out.get(key, 0) + 1
    return out


def head_count(index_a, index_b):
    """the pair bound Q: pixels with a pair whose left and upper neighbours do not exist or have none or another"""
    H, W = index_a.shape
    a, b = index_a.tolist(), index_b.tolist()
    q = 0
    for r in range(H):
        for c in range(W):
            if a[r][c] < 0 or b[r][c] < 0:
                continue
            pair = (a[r][c], b[r][c])
            left = c > 0 and (a[r][c - 1], b[r][c - 1]) == pair
            up = r > 0 and (a[r - 1][c], b[r - 1][c]) == pair
            q += not (left or up)
    return q


def class_order(table):
    """the permutation that puts a region table into polygon order: a stable sort by class"""
    return sorted(range(len(table)), key=lambda i: table[i][1])


def match(table_a, table_b, pairs, iou_threshold=0.5, classes="same"):
    """Greedy one-to-one matching by descending IoU, ties to the smaller (ia, ib).  Returns six lists: match index (-1:
    none), greatest IoU with any candidate and covered share per region of A, then the same for B, and the dict
    {(ia, ib): IoU} of the accepted pairs."""
    cand = []
    for (ia, ib), n in pairs.items():
        if classes == "same" and table_a[ia][1] != table_b[ib][1]:
            continue
        cand.append((n / (table_a[ia][2] + table_b[ib][2] - n), ia, ib, n))
    a_match, b_match = [-1] * len(table_a), [-1] * len(table_b)
    a_best, b_best = [0.0] * len(table_a), [0.0] * len(table_b)
    a_cov, b_cov = [0] * len(table_a), [0] * len(table_b)
    for iou, ia, ib, n in cand:
        a_best[ia], b_best[ib] = max(a_best[ia], iou), max(b_best[ib], iou)
        a_cov[ia] += n
        b_cov[ib] += n
    accepted = {}
    for iou, ia, ib, _ in sorted(cand, key=lambda c: (-c[0], c[1], c[2])):
        if iou >= iou_threshold and a_match[ia] < 0 and b_match[ib] < 0:
            a_match[ia], b_match[ib] = ib, ia
            accepted[(ia, ib)] = iou
    a_cov = [s / t[2] for s, t in zip(a_cov, table_a)]
    b_cov = [s / t[2] for s, t in zip(b_cov, table_b)]
    return a_match, a_best, a_cov, b_match, b_best, b_cov, accepted


def counts(table_a, table_b, a_match, b_match, accepted, num_classes):
    """([K][3] TP, FP, FN per class, [K] sums of matched IoU); A is the prediction, B the reference"""
    out = [[0, 0, 0] for _ in range(num_classes)]
    sums = [0.0] * num_classes
    for i, (_, c, _) in enumerate(table_a):
        if c < num_classes:
            out[c][0 if a_match[i] >= 0 else 1] += 1
    for i, (_, c, _) in enumerate(table_b):
        if c < num_classes and b_match[i] < 0:
            out[c][2] += 1
    for (ia, _), iou in sorted(accepted.items()):
        if table_a[ia][1] < num_classes:
            sums[table_a[ia][1]] += iou
    return out, sums


def full(a, b, background_a=None, background_b=None, min_pixels_a=1, min_pixels_b=1):
    """everything ops.region_overlaps returns, as Python values: (table_a, table_b, sorted [(ia, ib, n)], Q)"""
    ia, ta = regions(a, background_a, min_pixels_a)
    ib, tb = regions(b, background_b, min_pixels_b)
    pairs = overlaps(ia, ib)
    return ta, tb, sorted((x, y, n) for (x, y), n in pairs.items()), head_count(ia, ib)
