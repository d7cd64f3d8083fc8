"""Object matching on the host (flairhip/objects.py) on hand-worked cases, the oracle of the GPU tests
(tests/objects_oracle.py) on the same cases, the ABI of include/flairhip_objects.h against
flairhip.lib.OBJECT_SIGNATURES by the method of tests/test_eval_abi_cpu.py, and the two host-only size functions.
No GPU."""
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import objects_oracle as oracle
import test_abi_cpu as abi
from helpers import ROOT
from flairhip import lib as L
from flairhip import objects

HEADER = os.path.join(ROOT, "include", "flairhip_objects.h")


def ov_of(table_a, table_b, pairs):
    """what objects.py reads of a RegionOverlaps, from (first, class, pixels) tables and {(ia, ib): n}"""
    def cols(table):
        return [np.array([r[k] for r in table], dt) for k, dt in ((0, np.int32), (1, np.int32), (2, np.int64))]
    keys = sorted(pairs)
    return SimpleNamespace(**dict(zip(("a_first", "a_class", "a_pixels"), cols(table_a))),
                           **dict(zip(("b_first", "b_class", "b_pixels"), cols(table_b))),
                           pair_a=np.array([k[0] for k in keys], np.int32),
                           pair_b=np.array([k[1] for k in keys], np.int32),
                           pair_pixels=np.array([pairs[k] for k in keys], np.int64))


def both(table_a, table_b, pairs, thr=0.5, classes="same"):
    """the product's matching, after checking that the oracle's is the same"""
    m = objects.match_objects(ov_of(table_a, table_b, pairs), thr, classes)
    a_match, a_best, a_cov, b_match, b_best, b_cov, _ = oracle.match(table_a, table_b, pairs, thr, classes)
    assert m.a_match.tolist() == a_match and m.b_match.tolist() == b_match
    assert m.a_best_iou.tolist() == a_best and m.b_best_iou.tolist() == b_best
    assert m.a_covered.tolist() == a_cov and m.b_covered.tolist() == b_cov
    return m


# ---- hand-worked matching ---------------------------------------------------------------------------------------------

def test_two_regions_compete_for_one_reference_and_the_tie_goes_to_the_smaller_index():
    # both regions of A have 6 pixels, 4 of them in the 8-pixel reference: IoU 4 / (6 + 8 - 4) = 0.4 each
    ta, tb = [(0, 1, 6), (50, 1, 6)], [(3, 1, 8)]
    m = both(ta, tb, {(0, 0): 4, (1, 0): 4}, thr=0.4)
    assert m.a_match.tolist() == [0, -1] and m.b_match.tolist() == [0]
    assert m.a_best_iou.tolist() == [0.4, 0.4] and m.a_match_iou.tolist() == [0.4, 0.0]
    assert m.a_covered.tolist() == [4 / 6, 4 / 6] and m.b_covered.tolist() == [1.0]
    # the greater IoU wins whatever the index
    m = both(ta, tb, {(0, 0): 3, (1, 0): 5}, thr=0.25)
    assert m.a_match.tolist() == [-1, 0] and m.b_match_iou.tolist() == [5 / 9]


def test_greedy_keeps_the_loser_free_for_its_next_candidate():
    ta, tb = [(0, 1, 10), (20, 1, 10)], [(0, 1, 10), (30, 1, 10)]
    # IoU: (0,0) 8/12, (1,0) 2/18, (1,1) 6/14, (0,1) 1/19
    m = both(ta, tb, {(0, 0): 8, (1, 0): 2, (1, 1): 6, (0, 1): 1}, thr=0.3)
    assert m.a_match.tolist() == [0, 1] and m.b_match.tolist() == [0, 1]
    assert m.a_covered.tolist() == [0.9, 0.8]


def test_the_threshold_exactly_met_is_accepted():
    ta, tb = [(0, 2, 6)], [(1, 2, 6)]  # n = 4: IoU 4 / 8 = 0.5 exactly
    assert both(ta, tb, {(0, 0): 4}, thr=0.5).a_match.tolist() == [0]
    assert both(ta, tb, {(0, 0): 4}, thr=np.nextafter(0.5, 1.0)).a_match.tolist() == [-1]


def test_same_against_any():
    ta, tb = [(0, 1, 4), (9, 2, 4)], [(0, 2, 4), (9, 2, 5)]
    pairs = {(0, 0): 4, (1, 1): 3}
    same, any_ = both(ta, tb, pairs, classes="same"), both(ta, tb, pairs, classes="any")
    assert same.a_match.tolist() == [-1, 1] and same.a_best_iou.tolist() == [0.0, 0.5] and same.a_covered[0] == 0.0
    assert any_.a_match.tolist() == [0, 1] and any_.a_best_iou.tolist() == [1.0, 0.5]
    with pytest.raises(ValueError):
        objects.match_objects(ov_of(ta, tb, pairs), classes="both")


def test_an_empty_side():
    ta = [(0, 1, 4), (9, 2, 4)]
    m = both(ta, [], {})
    assert m.a_match.tolist() == [-1, -1] and len(m.b_match) == 0 and m.a_best_iou.tolist() == [0.0, 0.0]
    counts, sums = objects.object_counts(ov_of(ta, [], {}), m, 3)
    assert counts.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 0]] and sums.tolist() == [0.0, 0.0, 0.0]
    m = both([], ta, {})
    counts, _ = objects.object_counts(ov_of([], ta, {}), m, 3)
    assert counts.tolist() == [[0, 0, 0], [0, 0, 1], [0, 0, 1]]
    m = both([], [], {})
    assert len(m.a_match) == 0 and len(m.b_match) == 0


def test_above_one_half_greedy_equals_all_pairs_above_the_threshold():
    """two regions whose IoU exceeds 1/2 share more than half of each, so no region has two such partners"""
    g = np.random.default_rng(0)
    a = np.repeat(np.repeat(g.integers(0, 3, (8, 9)), 4, 0), 5, 1).astype(np.uint8)
    b = np.roll(a, 1, 1)  # a lone 4 x 5 cell keeps 16 of its 20 pixels: IoU 16 / 24
    ia, ta = oracle.regions(a)
    ib, tb = oracle.regions(b)
    pairs = oracle.overlaps(ia, ib)
    for thr in (0.51, 0.6, 0.75):
        m = both(ta, tb, pairs, thr=thr)
        want = sorted((x, y) for (x, y), n in pairs.items()
                      if ta[x][1] == tb[y][1] and n / (ta[x][2] + tb[y][2] - n) >= thr)
        assert want and sorted((i, int(j)) for i, j in enumerate(m.a_match) if j >= 0) == want


def test_counts_against_the_oracle_and_additivity():
    g = np.random.default_rng(1)
    a = np.repeat(np.repeat(g.integers(0, 4, (6, 7)), 3, 0), 4, 1).astype(np.uint8)
    b = np.roll(a, 1, 1)
    b[5:9, 3:11] = 2
    ia, ta = oracle.regions(a, 0)
    ib, tb = oracle.regions(b, 0)
    pairs = oracle.overlaps(ia, ib)
    ov = ov_of(ta, tb, pairs)
    m = objects.match_objects(ov, 0.5)
    a_match, _, _, b_match, _, _, accepted = oracle.match(ta, tb, pairs, 0.5)
    counts, sums = objects.object_counts(ov, m, 4)
    want_counts, want_sums = oracle.counts(ta, tb, a_match, b_match, accepted, 4)
    assert counts.dtype == np.int64 and counts.tolist() == want_counts and counts[:, 0].sum() > 0
    assert sums.dtype == np.float64 and np.allclose(sums, want_sums, rtol=1e-15, atol=0)
    assert counts[:, :2].sum() == len(ta) and counts[:, 0].sum() + counts[:, 2].sum() == len(tb)
    # a class beyond K counts nowhere
    assert objects.object_counts(ov, m, 2)[0].tolist() == want_counts[:2]


# ---- scores -----------------------------------------------------------------------------------------------------------

def test_scores_and_zero_denominators():
    counts = np.array([[3, 1, 2], [0, 0, 0], [0, 2, 0], [0, 0, 4]], np.int64)
    s = objects.object_scores(counts, np.array([2.4, 0.0, 0.0, 0.0]))
    assert s["precision"][0] == 0.75 and s["recall"][0] == 0.6 and s["f1"][0] == 6 / 9
    assert s["mean_matched_iou"][0] == 2.4 / 3
    assert all(np.isnan(s[k][1]) for k in ("precision", "recall", "f1", "mean_matched_iou"))
    assert s["precision"][2] == 0.0 and np.isnan(s["recall"][2]) and s["f1"][2] == 0.0
    assert np.isnan(s["precision"][3]) and s["recall"][3] == 0.0
    assert s["micro"]["tp"] == 3 and s["micro"]["precision"] == 0.5 and s["micro"]["recall"] == 3 / 9
    j = json.loads(json.dumps(objects.scores_json(s, ["a", "b", "c", "d"])))
    assert j["classes"]["b"] == {"tp": 0, "fp": 0, "fn": 0, "precision": None, "recall": None, "f1": None,
                                 "mean_matched_iou": None}
    assert j["classes"]["a"]["tp"] == 3 and j["classes"]["a"]["precision"] == 0.75
    empty = objects.object_scores(np.zeros((2, 3), np.int64), np.zeros(2))
    assert all(np.isnan(empty["micro"][k]) for k in ("precision", "recall", "f1", "mean_matched_iou"))
    assert objects.scores_json(empty)["micro"]["f1"] is None


# ---- the oracle's own pieces on a raster small enough to check by eye ------------------------------------------------

def test_oracle_on_a_hand_worked_raster():
    a = np.array([[1, 1, 0, 2],
                  [1, 0, 0, 2],
                  [3, 3, 3, 2]], np.uint8)
    b = np.array([[1, 1, 1, 1],
                  [0, 0, 2, 2],
                  [2, 2, 2, 2]], np.uint8)
    ia, ta = oracle.regions(a, 0)
    ib, tb = oracle.regions(b, 0)
    assert ta == [(0, 1, 3), (3, 2, 3), (8, 3, 3)] and tb == [(0, 1, 4), (6, 2, 6)]
    assert oracle.overlaps(ia, ib) == {(0, 0): 2, (1, 0): 1, (1, 1): 2, (2, 1): 3}
    # heads: (0,0) at pixel 0; (1,0) at 3; (1,1) at 7; (2,1) at 8; pixel 4 has no pair in b
    assert oracle.head_count(ia, ib) == 4
    assert oracle.regions(a, 0, 4)[1] == [] and oracle.class_order([(0, 2, 1), (1, 1, 1), (2, 2, 1)]) == [1, 0, 2]
    assert oracle.full(a, b, 0, 0) == (ta, tb, [(0, 0, 2), (1, 0, 1), (1, 1, 2), (2, 1, 3)], 4)


# ---- ABI --------------------------------------------------------------------------------------------------------------

def header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def test_object_table_equals_the_objects_header(monkeypatch):
    monkeypatch.setattr(abi, "header_text", header_text)
    header = abi.header_signatures()
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", header_text())), "the parser missed a prototype"
    assert sorted(header) == ["ffa_region_overlap_bytes", "ffa_region_overlap_count", "ffa_region_overlap_pairs",
                              "ffa_region_overlap_table_bytes"]
    assert abi.mismatches(header, L.OBJECT_SIGNATURES) == []
    for other in (L.SIGNATURES, L.EVAL_SIGNATURES, L.GATHER_SIGNATURES, L.SERIES_SIGNATURES, L.CALIB_SIGNATURES):
        assert not set(L.OBJECT_SIGNATURES) & set(other)


def test_the_main_header_includes_the_objects_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_objects\.h"$', main, flags=re.M)
    at = main.index('#include "flairhip_objects.h"')
    assert main.index('extern "C" {') < at < main.rindex("#ifdef __cplusplus")
    assert main.index("typedef struct ihipStream_t* ffa_stream_t;") < at


def test_the_header_says_what_it_must():
    text = " ".join(open(HEADER).read().replace("*", " ").split())
    assert "in unspecified order" in text
    assert "does not promise equal bytes for equal inputs" in text
    assert "the set and every number in it are deterministic" in text
    assert "is exactly the polygon order of ffa_polygonize_emit" in text


# ---- the size functions: host only ------------------------------------------------------------------------------------

def test_overlap_bytes_and_its_limit(lib):
    n = lib.ffa_region_overlap_bytes(300, 300)
    assert 22 * 90000 <= n <= 22 * 90000 + (1 << 16)
    assert lib.ffa_region_overlap_bytes(1, 1) > 0
    assert lib.ffa_region_overlap_bytes(1 << 15, (1 << 15) - 1) > 0
    assert lib.ffa_region_overlap_bytes(1 << 15, 1 << 15) == -1  # FFA_ERR_ARG
    assert b"32768 x 32768" in lib.ffa_last_error() and b"2^30" in lib.ffa_last_error()
    assert lib.ffa_region_overlap_bytes(0, 5) == -1


def test_table_bytes(lib):
    assert lib.ffa_region_overlap_table_bytes(0) == 64 * 16
    assert lib.ffa_region_overlap_table_bytes(32) == 64 * 16
    assert lib.ffa_region_overlap_table_bytes(33) == 128 * 16
    assert lib.ffa_region_overlap_table_bytes(64) == 128 * 16
    assert lib.ffa_region_overlap_table_bytes(65) == 256 * 16
    assert lib.ffa_region_overlap_table_bytes(-1) == -1
    assert lib.ffa_region_overlap_table_bytes(1 << 30) == -1 and b"2^30" in lib.ffa_last_error()
