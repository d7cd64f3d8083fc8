"""Test-time augmentation in the zonal tile loop (config key ``tta``): the written rasters against an oracle loop that
feeds the same batches to the same model once per view with ``AUG`` set, takes the returned logits to float64 and
applies flairhip.augment.tta_mean_probabilities, the margin crop and the reference's window placement.

Setup of tests/test_zonal_gpu.py::test_run_inference_matches_oracle_loop: patch 128, margin 16, a 200 x 260 raster of
3 bands, resnet34-unet with the seeded weights (segmentation head scaled down, see base_cfg), batch size 4.  Comparison rule of tests/test_tta_gpu.py::test_views_against_float64: a uint8
band may differ from rint(255 p64) only where 255 p64 lies within 1e-3 of a half-integer, and then by 1; a label only
where the float64 top-two gap is below 1e-5; each exclusion set holds at most 1 % of the values, asserted on the oracle
alone before the rasters are looked at.
"""
import copy
import os

import numpy as np
import pytest
import torch

from flairhip import augment
from helpers import MOD, ROOT, TASK, oracle_to_product_keys

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
PATCH, MARGIN, RES, H, W, K = 128, 16, 0.2, 200, 260, 19
MEANS, STDS = [105.66, 111.35, 102.18], [52.23, 45.62, 44.30]


@pytest.fixture(scope="module")
def base_cfg(tmp_path_factory):
    import yaml
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    tmp = tmp_path_factory.mktemp("tta_zonal")
    img = np.random.default_rng(3).integers(0, 255, (3, H, W)).astype(np.uint8)
    ras = ArrayRaster(img, 651992.36, 6860417.84, RES)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp), "output_name": "z", "img_pixels_detection": PATCH, "margin": MARGIN,
                "output_px_meters": RES, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "fp32"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": MEANS, "stds": STDS}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(K)}}]
    oracle = UnetResNet34(3, K)
    state = fill_state_dict(oracle.state_dict(), seed=77)
    # The seeded weights give logits of several hundred: every softmax is one-hot, a mean over V views is a multiple
    # of 1 / V, classes tie exactly and 255 p sits exactly on half-integers.  With the head scaled by 2^-8 the logits
    # spread like N(0, 2) and the probabilities are graded like a trained network's (the float64 oracle's exclusion
    # shares are then about 0.2 % for bands and 0.01 % for labels; the test asserts the cap).
    for key in ("segmentation_head.0.weight", "segmentation_head.0.bias"):
        state[key] = state[key] * 2.0 ** -8
    oracle.load_state_dict(state)
    cfg["model_weights"] = str(tmp / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    return cfg


def run(base_cfg, **keys):
    from flair_zonal_detection.inference import run_inference
    cfg = copy.deepcopy(base_cfg)
    shard = keys.pop("shard", None)
    cfg.update(keys)
    return run_inference(cfg, shard=shard)


def oracle_probabilities(base_cfg, codes):
    """float64 [K, H, W] mean probabilities of the mosaic and the mask of written pixels: the product's model on the
    product's batches, one forward per view, everything after the logits on the host"""
    from flair_zonal_detection.dataset import TileBatcher
    from flair_zonal_detection.inference import prep_config, prep_dataset
    from flair_zonal_detection.model_utils import build_inference_model, compute_patch_sizes
    from flair_zonal_detection.slicing import generate_patches_from_reference
    from oracle.tile_bookkeeping import write_window
    config = prep_config(copy.deepcopy(base_cfg))
    ras = config["modalities"][MOD]["input_img_path"]
    tiles = generate_patches_from_reference(config, ras, None)
    patch_sizes = compute_patch_sizes(config)
    dev = config["device"]
    model = build_inference_model(config, patch_sizes).to(dev)
    ds = prep_dataset(config, tiles, patch_sizes)
    assert TileBatcher.supports(ds)
    norm = torch.tensor(np.stack(ds.norm_vectors(MOD)), dtype=torch.float32, device=dev)
    bounds = tuple(ras.bounds)
    lefts, tops = np.asarray(tiles["left"]), np.asarray(tiles["top"])
    canvas = np.zeros((K, H, W))
    written = np.zeros((H, W), dtype=bool)
    keep = PATCH - 2 * MARGIN
    with torch.no_grad():
        for batch in TileBatcher(ds, 4):
            x = batch[MOD].to(dev)
            views = []
            for code in codes:
                aug = torch.full((x.shape[0],), code, dtype=torch.uint8, device=dev)
                logits, _ = model({MOD: x, MOD + "_NORM": norm, "AUG": aug})
                views.append(logits[TASK].double().cpu().numpy())
            p = augment.tta_mean_probabilities(views, codes)[..., MARGIN:PATCH - MARGIN, MARGIN:PATCH - MARGIN]
            for i, ti in enumerate(batch["index"].cpu().numpy().flatten()):
                col, row, w, h, skip = write_window(lefts[ti], tops[ti], bounds, RES, keep, keep)
                if skip:
                    continue
                canvas[:, row:row + h, col:col + w] = p[i][:, :h, :w]
                written[row:row + h, col:col + w] = True
    return canvas, written


@pytest.mark.parametrize("name", ["d4", "flips"])
def test_tta_rasters_match_the_oracle_loop(cuda, base_cfg, name):
    codes = augment.TTA_VIEWS[name]
    p64, written = oracle_probabilities(base_cfg, codes)
    assert written.all()  # the tile grid covers the raster
    scaled = 255.0 * p64
    band_open = np.abs(scaled - np.floor(scaled) - 0.5) <= 1e-3
    top2 = np.sort(p64, axis=0)[-2:]
    label_open = (top2[1] - top2[0]) < 1e-5
    conf_open = np.take_along_axis(band_open, p64.argmax(axis=0)[None], axis=0)[0]  # the band of the largest probability
    for what, open_ in (("band", band_open), ("label", label_open), ("confidence", conf_open)):
        print(f"tta {name}: {what} exclusion share {open_.mean():.4%}")
        assert open_.mean() <= 0.01, what
    want_label, want_bands = p64.argmax(axis=0), np.rint(scaled).astype(np.int64)

    label = run(base_cfg, tta=name)[TASK].data
    assert label.shape == (1, H, W) and label.dtype == np.uint8
    assert not ((label[0] != want_label) & ~label_open).any()
    assert len(np.unique(label)) > 1

    bands = run(base_cfg, tta=name, output_type="class_prob")[TASK].data
    assert bands.shape == (K, H, W) and bands.dtype == np.uint8
    d = bands.astype(np.int64) - want_bands
    assert not (d != 0)[~band_open].any() and np.abs(d).max() <= 1

    both = run(base_cfg, tta=name, write_confidence=True)
    assert np.array_equal(both[TASK].data, label)
    conf = both[TASK + "_confidence"].data
    assert conf.shape == (1, H, W) and conf.dtype == np.uint8
    dc = conf[0].astype(np.int64) - np.rint(255.0 * p64.max(axis=0)).astype(np.int64)
    assert not (dc != 0)[~conf_open].any() and np.abs(dc).max() <= 1
    assert np.array_equal(conf[0], bands.max(axis=0))  # bit for bit the largest class_prob band


def test_tta_none_is_the_run_without_the_key(cuda, base_cfg):
    plain = run(base_cfg, write_confidence=True)
    for keys in ({"tta": "none"}, {"tta": None}):
        got = run(base_cfg, write_confidence=True, **keys)
        assert set(got) == set(plain)
        for key in plain:
            assert np.array_equal(got[key].data, plain[key].data), (keys, key)
    with pytest.raises(ValueError, match="tta"):
        run(base_cfg, tta="rot90")


def test_graph_and_eager_runs_write_the_same_bytes_under_d4(cuda, base_cfg):
    keys = {"tta": "d4", "write_confidence": True, "hardware": {"precision": "bf16"}}
    graphed = run(base_cfg, hip_graph=True, **keys)
    eager = run(base_cfg, hip_graph=False, **keys)
    for key in graphed:
        assert np.array_equal(graphed[key].data, eager[key].data), key
    assert graphed[TASK].data.any() and graphed[TASK + "_confidence"].data.any()


def test_two_shards_merge_to_the_unsharded_result_under_flips(cuda, base_cfg):
    from flair_zonal_detection.inference import merge_shard_outputs
    keys = {"tta": "flips", "write_confidence": True, "hardware": {"precision": "bf16"}}
    whole = run(base_cfg, **keys)
    parts = [run(base_cfg, shard=(r, 2), **keys) for r in range(2)]
    assert all(p[TASK].written.any() for p in parts)
    merged = merge_shard_outputs(parts)
    for key in whole:
        assert np.array_equal(merged[key].data, whole[key].data), key
