"""Test-time augmentation, host side (no GPU): the inverse of an augmentation code, the named view sets, the float64
definition of the averaged probabilities (flairhip.augment), the config key ``tta`` and the CLI flag ``--tta``."""
import numpy as np
import pytest

from flairhip import augment


def softmax64(z, axis):
    z = np.asarray(z, dtype=np.float64)
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


@pytest.mark.parametrize("n", [5, 4])
def test_inverse_code_undoes_every_code(n):
    plane = np.arange(2 * n * n).reshape(2, n, n)  # every pixel distinct: equality pins the whole permutation
    for code in range(16):
        inv = augment.inverse_code(code)
        assert isinstance(inv, int) and 0 <= inv <= 7
        assert np.array_equal(augment.apply_code(augment.apply_code(plane, code), inv), plane), code
        assert augment.inverse_code(augment.inverse_code(inv)) == inv  # an involution on 0..7
    views = {augment.apply_code(plane, c).tobytes() for c in augment.TTA_VIEWS["d4"]}
    assert len(views) == 8  # the 8 codes of d4 are the 8 distinct transforms
    # codes 8..15 alias codes 0..7
    assert {augment.apply_code(plane, c).tobytes() for c in range(8, 16)} == views


def test_inverse_code_table():
    inv = [augment.inverse_code(c) for c in range(8)]
    assert inv == [0, 1, 2, 3, 7, 5, 6, 4]  # the quarter turns are each other's inverses, the rest their own


def test_tta_view_sets():
    assert augment.TTA_VIEWS == {"none": (0,), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
    for name, codes in augment.TTA_VIEWS.items():
        assert augment.tta_views(name) == codes
    for bad in ("rot", "D4", "", None, 4):
        with pytest.raises(ValueError):
            augment.tta_views(bad)


def test_one_identity_view_is_a_plain_softmax():
    z = np.random.default_rng(0).normal(0, 2, (2, 7, 5, 5))
    got = augment.tta_mean_probabilities([z], (0,))
    assert got.dtype == np.float64
    assert np.array_equal(got, softmax64(z, 1))


def test_all_views_of_an_orbit_give_the_plane_s_softmax():
    """view v holds the logits apply_code(z, code_v): every view, taken back, is the softmax of z itself"""
    z = np.random.default_rng(1).normal(0, 2, (2, 6, 5, 5))
    for name in ("flips", "d4"):
        codes = augment.TTA_VIEWS[name]
        got = augment.tta_mean_probabilities([augment.apply_code(z, c) for c in codes], codes)
        assert np.abs(got - softmax64(z, 1)).max() <= 4 * np.finfo(np.float64).eps  # a sum of V equal terms / V
    # and a view set in another order, with aliases of the same transforms
    codes = (12, 0, 9, 6)
    got = augment.tta_mean_probabilities([augment.apply_code(z, c) for c in codes], codes)
    assert np.abs(got - softmax64(z, 1)).max() <= 4 * np.finfo(np.float64).eps


def test_mean_probabilities_average_distinct_views():
    g = np.random.default_rng(2)
    a, b = g.normal(0, 2, (3, 4, 4)), g.normal(0, 2, (3, 4, 4))
    got = augment.tta_mean_probabilities([a, b], (0, 4))
    want = (softmax64(a, 0) + augment.apply_code(softmax64(b, 0), 7)) / 2
    assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        augment.tta_mean_probabilities([a, b], (0,))
    with pytest.raises(ValueError):
        augment.tta_mean_probabilities([], ())


def test_validate_tta():
    from flair_zonal_detection.config import validate_tta
    assert validate_tta({}) == "none"
    assert validate_tta({"tta": None}) == "none"
    for name in ("none", "flips", "d4"):
        assert validate_tta({"tta": name}) == name
    for bad in ("rot90", "all", 8, True, ["d4"]):
        with pytest.raises(ValueError):
            validate_tta({"tta": bad})


def test_validate_config_checks_tta(tmp_path):
    from flair_zonal_detection.config import validate_config
    weights = tmp_path / "w.ckpt"
    weights.write_bytes(b"")
    cfg = {"output_path": str(tmp_path), "output_name": "z", "model_weights": str(weights), "img_pixels_detection": 128,
           "margin": 16, "modalities": {}, "tasks": [], "output_px_meters": 0.2}
    validate_config(dict(cfg))
    validate_config(dict(cfg, tta="d4"))
    with pytest.raises(ValueError, match="tta"):
        validate_config(dict(cfg, tta="eight"))


def test_cli_accepts_tta():
    from flair_zonal_detection.main import build_parser
    parser = build_parser()
    assert parser.parse_args(["--config", "c.yaml"]).tta is None
    for name in ("none", "flips", "d4"):
        assert parser.parse_args(["--config", "c.yaml", "--tta", name]).tta == name
    with pytest.raises(SystemExit):
        parser.parse_args(["--config", "c.yaml", "--tta", "rot"])
