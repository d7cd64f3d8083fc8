"""numpy restatement of the overview definition of include/flairhip.h (ffa_overview_pyramid_u8), shared by the COG and
overview tests.  Written from the definition, pixel block by pixel block in vectorised form; no code of the kernel."""
import numpy as np


def n_levels(H: int, W: int, block: int) -> int:
    L = 0
    while max(-(-H // (1 << L)), -(-W // (1 << L))) > block:
        L += 1
    return L


def _block_members(prev: np.ndarray):
    """the four members of every 2 x 2 block of prev [bands, H, W] and, per member, whether it exists: rows
    2r .. min(2r + 1, H - 1), columns 2c .. min(2c + 1, W - 1)"""
    _, H, W = prev.shape
    h, w = -(-H // 2), -(-W // 2)
    rows, cols = 2 * np.arange(h), 2 * np.arange(w)
    members, exists = [], []
    for dr in (0, 1):
        for dc in (0, 1):
            rr, cc = rows + dr, cols + dc
            ok = (rr < H)[:, None] & (cc < W)[None, :]
            vals = prev[:, np.minimum(rr, H - 1)[:, None], np.minimum(cc, W - 1)[None, :]]
            members.append(vals.astype(np.int64))
            exists.append(np.broadcast_to(ok[None], vals.shape))
    return members, exists


def next_level(prev: np.ndarray, method: str, ignore=None) -> np.ndarray:
    members, exists = _block_members(prev)
    if method == "nearest":
        return members[0].astype(np.uint8)
    if method == "average":
        assert ignore is None
        s = sum(np.where(e, m, 0) for m, e in zip(members, exists))
        n = sum(e.astype(np.int64) for e in exists)
        return ((2 * s + n) // (2 * n)).astype(np.uint8)
    assert method == "mode"
    votes = [e & (m != ignore) if ignore is not None else e for m, e in zip(members, exists)]
    best_count = np.zeros(members[0].shape, np.int64)
    best_value = np.full(members[0].shape, -1 if ignore is None else int(ignore), np.int64)
    for v in np.unique(prev).tolist():  # ascending: a later value replaces the best only with strictly more votes
        count = sum((vt & (m == v)).astype(np.int64) for m, vt in zip(members, votes))
        better = count > best_count
        best_count = np.where(better, count, best_count)
        best_value = np.where(better, v, best_value)
    assert (best_value >= 0).all()
    return best_value.astype(np.uint8)


def pyramid(base: np.ndarray, levels: int, method: str, ignore=None):
    """levels 1 .. levels of base [bands, H, W] (mode and average cascade; nearest does too, which is the same thing)"""
    out, cur = [], base
    for _ in range(levels):
        cur = next_level(cur, method, ignore)
        out.append(cur)
    return out
