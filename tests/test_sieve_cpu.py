"""The sieve's host side (no GPU): the numpy oracle of tests/test_sieve_gpu.py against hand-worked 5 x 7 cases, the
config key, the command-line option and the library's exports."""
import os
import re

import numpy as np
import pytest

from helpers import ROOT
from sieve_oracle import label, sieve, sieve_round


def grid(text):
    return np.array([[int(v) for v in row.split()] for row in text.strip().splitlines()], dtype=np.uint8)


def stats(rounds, comps, pixels, remaining):
    return {"rounds": rounds, "relabelled_components": comps, "relabelled_pixels": pixels, "remaining_small": remaining}


def test_labels_are_first_pixels_in_row_major_order():
    # the two arms of class 1 meet along the bottom row: one component, root 0
    lab, counts = label(grid("""
        1 1 2 2 2 1 1
        1 2 2 0 2 1 1
        1 1 1 0 2 2 1
        3 3 1 0 0 0 1
        3 1 1 1 1 1 1"""), background=0)
    assert lab.tolist() == [[0, 0, 2, 2, 2, 0, 0],
                            [0, 2, 2, -1, 2, 0, 0],
                            [0, 0, 0, -1, 2, 2, 0],
                            [21, 21, 0, -1, -1, -1, 0],
                            [21, 0, 0, 0, 0, 0, 0]]
    assert counts == {0: 19, 2: 8, 21: 3}


def test_an_island_is_absorbed_and_a_large_region_never_moves():
    cls = np.ones((5, 7), np.uint8)
    cls[2, 3] = 2
    out, st = sieve(cls, 2)
    assert out.tolist() == np.ones((5, 7), np.uint8).tolist() and st == stats(2, 1, 1, 0)
    # threshold 1: nothing is small, nothing runs
    out, st = sieve(cls, 1)
    assert out.tolist() == cls.tolist() and st == stats(0, 0, 0, 0)


def test_corners_are_no_neighbours_and_background_is_no_target():
    cls = grid("""
        0 0 0 0 0 0 0
        0 2 0 0 0 0 0
        0 0 3 3 0 0 0
        0 0 0 0 0 0 0
        0 0 0 0 0 0 0""")
    out, st = sieve(cls, 5, background=0)
    assert out.tolist() == cls.tolist() and st == stats(1, 0, 0, 2)
    # without a background the zeros are a class of 32 pixels, and both islands join it
    out, st = sieve(cls, 5)
    assert not out.any() and st == stats(2, 2, 3, 0)


CHAIN = """
    0 0 0 0 0 0 0
    1 2 2 3 3 3 4
    0 0 0 0 0 0 4
    0 0 0 4 4 4 4
    0 0 0 4 4 4 4"""


def test_a_chain_takes_the_classes_of_the_start_of_the_round():
    # components of 1, 2 and 3 pixels next to one of 10: each takes its right neighbour's class as it was when the
    # round began, although that neighbour is relabelled in the same round
    cls = grid(CHAIN)
    one, counts = sieve_round(cls, 4, background=0)
    assert one[1].tolist() == [2, 3, 3, 4, 4, 4, 4] and counts == [3, 3, 6, 4]
    assert np.array_equal(one[[0, 2, 3, 4]], cls[[0, 2, 3, 4]])
    two, counts = sieve_round(one, 4, background=0)
    assert two[1].tolist() == [3, 4, 4, 4, 4, 4, 4] and counts == [2, 2, 3, 3]
    out, st = sieve(cls, 4, background=0)
    assert out[1].tolist() == [4] * 7 and st == stats(4, 6, 10, 0)
    out, st = sieve(cls, 4, background=0, max_rounds=1)
    assert out.tolist() == one.tolist() and st == stats(1, 3, 6, 2)


def test_equal_counts_the_smaller_root_wins():
    cls = grid("""
        0 0 0 0 0 0 0
        0 1 1 2 2 3 3
        0 0 0 0 0 0 0
        0 0 0 0 0 0 0
        0 0 0 0 0 0 0""")
    # three components of two pixels, roots 8 < 10 < 12: the first has no greater neighbour and stays, the second
    # takes the first's class, the third the second's class of the start of the round
    one, counts = sieve_round(cls, 3, background=0)
    assert one[1].tolist() == [0, 1, 1, 1, 1, 2, 2] and counts == [3, 2, 4, 3]
    out, st = sieve(cls, 3, background=0)
    assert out[1].tolist() == [0, 1, 1, 1, 1, 1, 1] and st == stats(3, 3, 6, 0)


def test_a_raster_of_one_small_component_is_left_alone():
    cls = np.full((5, 7), 7, np.uint8)
    out, st = sieve(cls, 100)
    assert out.tolist() == cls.tolist() and st == stats(1, 0, 0, 1)


def test_all_small_with_a_strict_maximum_ends_as_one_component():
    cls = np.tile(np.array([1, 1, 1, 2, 2, 3, 4], np.uint8), (5, 1))
    one, counts = sieve_round(cls, 36)
    # 15, 10, 5 and 5 pixels: the columns of 3 (root 5) and of 4 (root 6) tie, the smaller root is the greater
    assert one[0].tolist() == [1, 1, 1, 1, 1, 2, 3] and (one == one[0]).all() and counts == [4, 3, 20, 4]
    out, st = sieve(cls, 36)
    assert (out == 1).all() and st == stats(4, 6, 35, 1)


# ---- config key, command line, exports ------------------------------------------------------------------------------

@pytest.mark.parametrize("value,want", [(0, 0.0), (2.5, 2.5), ("3", 3.0)])
def test_config_accepts_numbers(value, want):
    from flair_zonal_detection.config import validate_sieve_area
    got = validate_sieve_area({"sieve_area": value})
    assert isinstance(got, float) and got == want
    assert validate_sieve_area({}) == 0.0


@pytest.mark.parametrize("value", [-1, "x", True])
def test_config_rejects_what_is_no_area(value):
    from flair_zonal_detection.config import validate_sieve_area
    with pytest.raises(ValueError, match="sieve_area"):
        validate_sieve_area({"sieve_area": value})


def test_validate_config_checks_the_key():
    from flair_zonal_detection.config import REQUIRED_KEYS, validate_config
    cfg = {k: None for k in REQUIRED_KEYS}
    cfg["sieve_area"] = -2.0
    with pytest.raises(ValueError, match="sieve_area"):
        validate_config(cfg)


def test_parser_carries_the_option():
    from flair_zonal_detection.main import build_parser
    args = build_parser().parse_args(["--config", "c.yaml", "--polygons", "p.gpkg", "--sieve-area", "1.5"])
    assert args.sieve_area == 1.5
    assert build_parser().parse_args(["--config", "c.yaml"]).sieve_area is None


def test_sieve_area_converts_like_min_area():
    from flair_zonal_detection.inference import sieve_pixels_for_area
    assert sieve_pixels_for_area(0.0, 0.04) == 0
    assert sieve_pixels_for_area(0.2, 0.04) == 5      # five pixels of 0.04 reach 0.2: four are below it
    assert sieve_pixels_for_area(0.21, 0.04) == 6
    with pytest.raises(ValueError, match="sieve_area"):
        sieve_pixels_for_area(-1.0, 0.04)


def test_library_exports_the_sieve(lib):
    from flairhip import lib as L
    header = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    declared = set(re.findall(r"\b(ffa_[a-z0-9_]+)\s*\(", header))
    for name in ("ffa_sieve_round_u8", "ffa_sieve_workspace_bytes"):
        assert name in declared, f"{name} is not declared in include/flairhip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
    # host-only calls: the size query and the argument checks need no device
    assert lib.ffa_sieve_workspace_bytes(40, 70) >= 17 * 40 * 70
    assert lib.ffa_sieve_workspace_bytes(0, 70) == -1 and lib.ffa_sieve_workspace_bytes(1 << 15, 1 << 15) == -1
    assert lib.ffa_sieve_round_u8(None, 4, 4, -1, 2, None, 0, None, None) == -1
    assert b"null" in lib.ffa_last_error()
