"""flairhip.augment (the host statement of the training augmentation) against tests/golden/augment_d4.npz: what the
reference's own apply_numpy_augmentations gave for 16 seeds that between them draw all 16 codes
(tests/golden/gen_augment_golden.py)."""
import os

import numpy as np
import pytest

from helpers import ROOT

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "augment_d4.npz"))
KEYS = ["AERIAL_RGBI", "DEM_ELEV", "SENTINEL2_TS", "AERIAL_LABEL-COSIA"]


def test_golden_covers_every_code():
    assert sorted(int(c) for c in GOLD["codes"]) == list(range(16))


@pytest.mark.parametrize("row", range(16))
def test_draw_codes_draws_what_the_reference_draws(row):
    from flairhip.augment import draw_codes
    np.random.seed(int(GOLD["seeds"][row]))
    codes = draw_codes(1)
    assert codes.dtype == np.uint8 and codes.shape == (1,)
    assert int(codes[0]) == int(GOLD["codes"][row])
    assert np.random.rand() == float(GOLD["next_rand"][row])  # the generator is where the reference left it


def test_draw_codes_takes_a_generator_of_its_own():
    from flairhip.augment import draw_codes, rank_epoch_rng
    np.random.seed(5)
    want = draw_codes(64)
    state = np.random.get_state()
    got = draw_codes(64, rng=np.random.RandomState(5))
    assert np.array_equal(want, got)
    assert np.array_equal(np.random.get_state()[1], state[1])  # the global generator was left alone
    assert len(set(want.tolist())) > 8  # all codes occur, not only the 8 distinct transforms
    a, b = draw_codes(64, rng=rank_epoch_rng(0, 0, 0)), draw_codes(64, rng=rank_epoch_rng(0, 1, 0))
    c, a2 = draw_codes(64, rng=rank_epoch_rng(0, 0, 1)), draw_codes(64, rng=rank_epoch_rng(0, 0, 0))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and np.array_equal(a, a2)
    assert np.array_equal(draw_codes(8, p_flip=0.0, p_rot=0.0), np.zeros(8, np.uint8))
    assert set(draw_codes(64, p_flip=1.0, p_rot=0.0).tolist()) == {3}


@pytest.mark.parametrize("row", range(16))
def test_source_index_reproduces_the_reference_outputs(row):
    from flairhip.augment import apply_code, d4_source_index
    code = int(GOLD["codes"][row])
    for key in KEYS:
        x, want = GOLD["in_" + key], GOLD[f"out{code:02d}_{key}"]
        si, sj = d4_source_index(code, x.shape[-1])
        got = x[..., si, sj]
        assert got.dtype == want.dtype and np.array_equal(got, want), key
        assert np.array_equal(apply_code(x, code), want)
        assert np.array_equal(apply_code(x, code | 0xF0), want)  # only the low four bits count


def test_sixteen_codes_are_eight_transforms():
    from flairhip.augment import d4_source_index
    seen = {tuple(np.stack(d4_source_index(c, 5)).ravel().tolist()) for c in range(16)}
    assert len(seen) == 8


def test_non_square_plane_raises():
    from flairhip.augment import apply_code
    with pytest.raises(ValueError):
        apply_code(np.zeros((3, 4, 5)), 4)
