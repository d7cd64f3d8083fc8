"""Per-zone class transitions between two rasters on the GPU (ffa_zone_change_u8 in csrc/zone_stats.hip through
ops.zone_transition_stats).

The oracle is tests/change_oracle.py: over the zone masks of tests/zone_stats_oracle.py, np.bincount of
min(before, K) * (K + 1) + min(after, K), and the same with the confidence bytes as int64 weights.  Every result is an
integer and every comparison is ``==``.  The marginals are also tied to the existing kernel (ops.zone_class_stats),
whose planes the new entry point shares.
"""
import numpy as np
import pytest
import torch

from change_oracle import cross_tab, oracle_change
from zone_stats_oracle import (CENTRE_BOX, H0, STAR, STAR_HOLE, W0, base_rasters, oracle_masks, parcel_grid,
                               random_polygons)

pytestmark = pytest.mark.gpu

K0 = 19


def gpu_change(before, after, zones, K, conf=None, **kw):
    """(counts, conf_sums) of ops.zone_transition_stats as numpy arrays"""
    from flairhip import ops
    dev = torch.device("cuda")
    counts, sums = ops.zone_transition_stats(torch.tensor(before, device=dev), torch.tensor(after, device=dev), zones, K,
                                             conf=None if conf is None else torch.tensor(conf, device=dev), **kw)
    torch.cuda.synchronize()
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (len(zones), K + 1, K + 1) and counts.is_cuda
    if conf is None:
        assert sums is None
        return counts.cpu().numpy(), None
    assert sums.dtype == torch.int64 and sums.shape == counts.shape
    return counts.cpu().numpy(), sums.cpu().numpy()


def gpu_stats(cls, zones, K, conf=None):
    from flairhip import ops
    dev = torch.device("cuda")
    counts, sums = ops.zone_class_stats(torch.tensor(cls, device=dev), zones, K,
                                        conf=None if conf is None else torch.tensor(conf, device=dev))
    return counts.cpu().numpy(), None if sums is None else sums.cpu().numpy()


def check(before, after, conf, zones, K, **kw):
    masks = oracle_masks(zones, *before.shape)
    want_c, want_s = oracle_change(before, after, conf, masks, K)
    got_c, got_s = gpu_change(before, after, zones, K, conf, **kw)
    assert np.array_equal(got_c, want_c)
    if conf is not None:
        assert np.array_equal(got_s, want_s)
    return got_c, got_s


@pytest.fixture(scope="module")
def pair():
    """(before, after, conf): two seeds of base_rasters, about 3 % of 255 in each; conf is the after run's"""
    before, _ = base_rasters(seed=11)
    after, conf = base_rasters(seed=12)
    assert before.shape == (H0, W0) and (before == 255).sum() > 100 and (after == 255).sum() > 100
    assert (before != after).mean() > 0.9
    for a in (before, after, conf):
        a.setflags(write=False)
    return before, after, conf


def mixed_zones():
    outside = CENTRE_BOX + [500.0, 0.0]
    larger = np.array([[-9.0, -7.0], [W0 + 8.0, -7.0], [W0 + 8.0, H0 + 6.0], [-9.0, H0 + 6.0]])
    return [[STAR, STAR_HOLE], [CENTRE_BOX], [outside], [larger], []] + [[p] for p in random_polygons()]


@pytest.fixture(scope="module")
def mixed(pair):
    """the 25 mixed zones with their oracle tables (computed once, read-only)"""
    before, after, conf = pair
    zones = mixed_zones()
    assert len(zones) == 25
    counts, sums = oracle_change(before, after, conf, oracle_masks(zones, H0, W0), K0)
    counts.setflags(write=False)
    sums.setflags(write=False)
    return zones, counts, sums


@pytest.fixture(scope="module")
def parcels():
    zones = parcel_grid()
    masks = oracle_masks(zones, H0, W0)
    masks.setflags(write=False)
    return zones, masks


# ---- 1. mixed zones ----------------------------------------------------------------------------------------------------

def test_mixed_zones(cuda, pair, mixed):
    before, after, conf = pair
    zones, want_c, want_s = mixed
    got_c, got_s = gpu_change(before, after, zones, K0, conf)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_s, want_s)
    total = got_c.sum(axis=(1, 2))
    assert total[0] == 4319 and total[1] == 400 and total[2] == 0 and total[3] == H0 * W0 and total[4] == 0
    # the fold: the "other" row and column are in use, and so is their corner
    assert got_c[:, K0, :K0].sum() > 0 and got_c[:, :K0, K0].sum() > 0 and got_c[3, K0, K0] > 0
    assert got_s[:, K0, :].sum() > 0 and got_s[:, :, K0].sum() > 0
    # without a confidence raster: the same counts, no sums
    plain, none = gpu_change(before, after, zones, K0)
    assert none is None and np.array_equal(plain, want_c)


# ---- 2. marginals -----------------------------------------------------------------------------------------------------

def test_marginals_are_the_class_stats_of_either_raster(cuda, pair, mixed):
    before, after, conf = pair
    zones, _, _ = mixed
    counts, sums = gpu_change(before, after, zones, K0, conf)
    assert np.array_equal(counts.sum(axis=2), gpu_stats(before, zones, K0)[0])
    after_c, after_s = gpu_stats(after, zones, K0, conf)
    assert np.array_equal(counts.sum(axis=1), after_c)
    assert np.array_equal(sums.sum(axis=1), after_s)


# ---- 3. identical rasters ---------------------------------------------------------------------------------------------

def test_identical_rasters_fill_the_diagonal_only(cuda, pair, mixed):
    _, after, conf = pair
    zones, _, _ = mixed
    counts, sums = gpu_change(after, after, zones, K0, conf)
    eye = np.eye(K0 + 1, dtype=bool)
    assert not counts[:, ~eye].any() and not sums[:, ~eye].any()
    want_c, want_s = gpu_stats(after, zones, K0, conf)
    assert np.array_equal(counts[:, eye], want_c) and np.array_equal(sums[:, eye], want_s)
    assert want_c.sum() > 0


# ---- 4. parcel grid ---------------------------------------------------------------------------------------------------

def test_parcel_grid_sums_to_the_whole_raster(cuda, pair, parcels):
    before, after, conf = pair
    zones, masks = parcels
    assert len(zones) == 576 and np.all(masks.sum(axis=0) == 1)
    assert int((masks.reshape(576, -1).sum(axis=1) == 0).sum()) == 67
    got_c, got_s = check(before, after, conf, zones, K0)
    assert np.array_equal(got_c.sum(axis=0), cross_tab(before, after, K0))
    assert np.array_equal(got_s.sum(axis=0), cross_tab(before, after, K0, conf))
    fa, fb = np.minimum(before.astype(np.int64), K0), np.minimum(after.astype(np.int64), K0)
    assert np.array_equal(got_c.sum(axis=0).ravel(), np.bincount((fa * (K0 + 1) + fb).ravel(), minlength=(K0 + 1) ** 2))


# ---- 5. partial last word, raster tail --------------------------------------------------------------------------------

def test_partial_last_word_and_raster_tail(cuda, pair):
    before, after, conf = pair
    # the last rows to the last pixel: the final word of the final row is read by load32's tail path in all three rasters
    low = np.array([[90.3, H0 - 2.4], [W0 + 3.0, H0 - 2.4], [W0 + 3.0, H0 + 3.0], [90.3, H0 + 3.0]])
    got, _ = check(before, after, conf, [[low]], K0)
    assert got.sum() == 2 * (W0 - 90) and W0 % 32 != 0
    last = oracle_masks([[low]], H0, W0)[0]
    assert last[H0 - 1, W0 - 1] and last[H0 - 1, 96:].all()  # the partial fifth word of the last row is all inside
    # a small raster whose every row ends in a partial word, one zone over everything
    b2, _ = base_rasters(33, 35, seed=21)
    a2, c2 = base_rasters(33, 35, seed=22)
    whole = np.array([[-1.0, -1.0], [36.0, -1.0], [36.0, 34.0], [-1.0, 34.0]])
    got, sums = check(b2, a2, c2, [[whole]], K0)
    assert got.sum() == 33 * 35 and sums.sum() == c2.astype(np.int64).sum()


# ---- 6. several chunks per zone ---------------------------------------------------------------------------------------

def test_a_zone_of_several_chunks_with_the_largest_partial_sums(cuda):
    from flairhip import ops
    side = 300
    before = np.full((side, side), 3, np.uint8)
    after = np.full((side, side), 7, np.uint8)
    conf = np.full((side, side), 255, np.uint8)
    whole = np.array([[-1.0, -1.0], [side + 1.0, -1.0], [side + 1.0, side + 1.0], [-1.0, side + 1.0]])
    win = ops.zone_stats_windows(*ops.zone_stats_flatten([[whole]]), side, side)
    chunks = ops.zone_stats_plan(win)[3]
    assert ops.zone_stats_plane_words(win)[2][0] == 300 * 10 > ops.ZONE_STATS_CHUNK_WORDS == 2048 and len(chunks) == 2
    counts, sums = gpu_change(before, after, [[whole]], K0, conf)  # 32 equal keys per full word: one run each
    assert np.count_nonzero(counts) == 1 and np.count_nonzero(sums) == 1
    assert counts[0, 3, 7] == 90000 and sums[0, 3, 7] == 255 * 90000


# ---- 7. K edges -------------------------------------------------------------------------------------------------------

def test_k_edges(cuda, pair):
    from flairhip import lib as L
    from flairhip import ops
    before, after, conf = pair
    zones = mixed_zones()[:5]
    got, _ = check(before, after, conf, zones, 1)  # everything that is not 0 is "other"
    assert got[3, 1, 1] == ((before != 0) & (after != 0)).sum() and got[3, 0, 0] == ((before == 0) & (after == 0)).sum()
    g = np.random.default_rng(5)
    b32 = g.integers(0, 32, (H0, W0)).astype(np.uint8)
    a32 = g.integers(0, 32, (H0, W0)).astype(np.uint8)
    b32[g.random((H0, W0)) < 0.03] = 255
    a32[g.random((H0, W0)) < 0.03] = 255
    got, _ = check(b32, a32, conf, zones, 32)
    assert got[3, 31, :].sum() > 0 and got[3, :, 31].sum() > 0 and got[3, 32, 32] > 0
    d_b, d_a = torch.tensor(before).cuda(), torch.tensor(after).cuda()
    for K in (33, 0, -1, 256):
        with pytest.raises(ValueError, match="n_classes"):
            ops.zone_transition_stats(d_b, d_a, zones, K)
    # the raw entry point: an argument error, before anything is read or launched
    lib = L.load()
    for K in (33, 0):
        rc = lib.ffa_zone_change_u8(d_b.data_ptr(), d_a.data_ptr(), None, H0, W0, K, None, 0, None, 0, None, 1, None,
                                    None, 0, None, 0, None, 0, None, None, None, 0, None)
        assert rc == -1  # FFA_ERR_ARG
        assert b"classes outside 1..32" in lib.ffa_last_error()


# ---- 8. batches -------------------------------------------------------------------------------------------------------

def test_batches_give_the_bytes_of_the_single_call(cuda, pair, parcels):
    from flairhip import ops
    before, after, conf = pair
    zones, _ = parcels
    win = ops.zone_stats_windows(*ops.zone_stats_flatten(zones), H0, W0)
    words = ops.zone_stats_plane_words(win)[2]
    budget = 4 * int(words.sum()) // 3
    assert len(ops.zone_stats_batches(words, budget)) >= 3
    one_c, one_s = gpu_change(before, after, zones, K0, conf)
    got_c, got_s = gpu_change(before, after, zones, K0, conf, max_workspace_bytes=budget)
    assert got_c.tobytes() == one_c.tobytes() and got_s.tobytes() == one_s.tobytes()
    assert one_c.sum() == H0 * W0


# ---- 9. determinism, written not accumulated --------------------------------------------------------------------------

def test_outputs_are_written_and_equal_from_call_to_call(cuda, pair, mixed, monkeypatch):
    from flairhip import ops
    before, after, conf = pair
    zones, want_c, want_s = mixed
    dev = torch.device("cuda")
    d = [torch.tensor(a, device=dev) for a in (before, after, conf)]
    real_empty = torch.empty

    def garbage(*args, **kw):  # the outputs come from torch.empty: hand them out full of a large value
        t = real_empty(*args, **kw)
        return t.fill_(0x5A5A5A5A5A5A) if t.dtype == torch.int64 else t

    monkeypatch.setattr(torch, "empty", garbage)
    c1, s1 = ops.zone_transition_stats(d[0], d[1], zones, K0, conf=d[2])
    ops.workspace(1, cuda, "zone_stats").fill_(0xA5)
    c2, s2 = ops.zone_transition_stats(d[0], d[1], zones, K0, conf=d[2])
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert torch.equal(c1, c2) and torch.equal(s1, s2)
    assert np.array_equal(c1.cpu().numpy(), want_c) and np.array_equal(s1.cpu().numpy(), want_s)
    assert (want_c[2] == 0).all() and (c1[2] == 0).all() and (c1[4] == 0).all()  # zones without a pixel: cleared too


# ---- 10. orientation and closedness -----------------------------------------------------------------------------------

def test_orientation_and_closedness_do_not_matter(cuda, pair, mixed):
    before, after, conf = pair
    zones, want_c, want_s = mixed
    flipped = [[np.vstack([r[::-1], r[::-1][:1]]) for r in rings] for rings in zones]
    got_c, got_s = gpu_change(before, after, flipped, K0, conf)
    assert np.array_equal(got_c, want_c) and np.array_equal(got_s, want_s)
