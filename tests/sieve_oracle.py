"""The sieve's semantics (include/flairhip.h, ffa_sieve_round_u8) restated in plain numpy / Python: the yardstick of
tests/test_sieve_gpu.py, itself pinned by the hand-worked cases of tests/test_sieve_cpu.py.  No scipy, no call into the
product."""
import numpy as np


def label(cls, background=None):
    """(labels int64 [H, W], counts {root: pixels}): explicit flood fill in row-major order, so the first pixel of a
    4-connected component of equal class is its root = its label; background pixels get -1"""
    cls = np.asarray(cls)
    H, W = cls.shape
    lab = np.full((H, W), -1, np.int64)
    rows = cls.tolist()
    seen = [[(background is not None and v == background) for v in row] for row in rows]
    counts = {}
    for r0 in range(H):
        for c0 in range(W):
            if seen[r0][c0]:
                continue
            v, root, n = rows[r0][c0], r0 * W + c0, 0
            seen[r0][c0] = True
            stack = [(r0, c0)]
            while stack:
                r, c = stack.pop()
                lab[r, c] = root
                n += 1
                for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                    if 0 <= rr < H and 0 <= cc < W and not seen[rr][cc] and rows[rr][cc] == v:
                        seen[rr][cc] = True
                        stack.append((rr, cc))
            counts[root] = n
    return lab, counts


def neighbours(lab):
    """{root: set of roots of the components sharing a pixel side with it}; background (-1) is nobody's neighbour"""
    out = {}
    for a, b in ((lab[:, :-1], lab[:, 1:]), (lab[:-1, :], lab[1:, :])):
        m = (a != b) & (a >= 0) & (b >= 0)
        for x, y in set(zip(a[m].tolist(), b[m].tolist())):
            out.setdefault(x, set()).add(y)
            out.setdefault(y, set()).add(x)
    return out


def sieve_round(cls, min_pixels, background=None):
    """one round on the state at its start -> (new raster, [small components at the start, components relabelled,
    pixels relabelled, components in all])"""
    cls = np.asarray(cls, dtype=np.uint8)
    lab, counts = label(cls, background)
    W = cls.shape[1]
    nb = neighbours(lab)
    key = lambda root: (counts[root], -root)  # noqa: E731  more pixels win, then the smaller root
    new_class = {}
    small = 0
    for root, n in counts.items():
        if n >= min_pixels:
            continue
        small += 1
        if not nb.get(root):
            continue
        best = max(nb[root], key=key)
        if key(best) > key(root):
            new_class[root] = int(cls[best // W, best % W])  # the class best had at the start of the round
    out = cls.copy()
    pixels = 0
    for root, v in new_class.items():
        m = lab == root
        out[m] = v
        pixels += int(m.sum())
    return out, [small, len(new_class), pixels, len(counts)]


def sieve(cls, min_pixels, background=None, max_rounds=16):
    """rounds until one relabels nothing or max_rounds have run -> (raster, the dict ops.sieve_ returns)"""
    cls = np.asarray(cls, dtype=np.uint8).copy()
    stats = {"rounds": 0, "relabelled_components": 0, "relabelled_pixels": 0, "remaining_small": 0}
    if min_pixels <= 1 or cls.size == 0:
        return cls, stats
    while stats["rounds"] < max_rounds:
        cls, (small, comps, pixels, _) = sieve_round(cls, min_pixels, background)
        stats["rounds"] += 1
        stats["relabelled_components"] += comps
        stats["relabelled_pixels"] += pixels
        if pixels == 0:
            break
    stats["remaining_small"] = sum(n < min_pixels for n in label(cls, background)[1].values())
    return cls, stats
