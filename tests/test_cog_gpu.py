"""COG conversion end to end: postprocess.convert_to_cog (GPU overview pyramid + geotiff.write_cog) and the
cog_conversion key of the zonal run.  All comparisons are exact."""
import copy
import os

import numpy as np
import pytest
import torch

from helpers import MOD, ROOT, TASK, oracle_to_product_keys
from overview_oracle import n_levels, pyramid

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def _levels_of(path):
    from flair_zonal_detection.geotiff import GeoTiffRaster
    with GeoTiffRaster(path) as r:
        n = r.overview_count
    out = []
    for k in range(n + 1):
        with GeoTiffRaster(path, overview=k) as r:
            out.append(r.read())
    return out


@pytest.mark.parametrize("method,ignore", [("nearest", None), ("mode", 255), ("average", None)])
def test_convert_to_cog(cuda, tmp_path, method, ignore):
    from flair_zonal_detection.geotiff import GeoTiffRaster, GeoTiffWriter, validate_cog
    from flair_zonal_detection.postprocess import convert_to_cog
    g = np.random.default_rng(21)
    data = g.integers(0, 5, (3, 300, 420), dtype=np.uint8)
    data[:, :90, 300:] = 255  # a clipped corner: blocks that are all ignore and part ignore
    src, dst = str(tmp_path / "pred.tif"), str(tmp_path / "pred_COG.tif")
    w = GeoTiffWriter(src, 420, 300, 3, 651992.4, 6860417.8, 0.2, crs="EPSG:2154", nodata=255)
    w.data[:] = data
    w.close()
    assert convert_to_cog(src, dst, overview_resampling=method, blocksize=128, ignore=ignore) is None
    assert not os.path.exists(src) and os.path.isfile(dst) and not os.path.exists(dst + ".part")
    assert validate_cog(dst) == []
    got = _levels_of(dst)
    want = [data] + pyramid(data, n_levels(300, 420, 128), method, ignore)
    assert len(want) == 3 and [lv.shape for lv in got] == [lv.shape for lv in want]
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"level {k}"
    with GeoTiffRaster(dst) as r:
        assert r.crs == "EPSG:2154" and r.res == (0.2, 0.2) and r.nodata == 255.0
        assert (r.bounds.left, r.bounds.top) == (651992.4, 6860417.8)
        assert r.profile["blockxsize"] == 128 and r.profile["compress"] == "lzw"


def test_convert_to_cog_refuses_what_it_cannot_convert(cuda, tmp_path):
    from flair_zonal_detection.geotiff import GeoTiffError, GeoTiffWriter
    from flair_zonal_detection.postprocess import convert_to_cog
    with pytest.raises(FileNotFoundError, match="missing.tif"):
        convert_to_cog(str(tmp_path / "missing.tif"), str(tmp_path / "out.tif"))
    p = str(tmp_path / "u16.tif")
    w = GeoTiffWriter(p, 40, 30, 1, 0.0, 30.0, 1.0, dtype=np.uint16)
    w.close()
    with pytest.raises(GeoTiffError, match="uint16"):
        convert_to_cog(p, str(tmp_path / "out.tif"))
    assert os.path.isfile(p) and not os.path.exists(str(tmp_path / "out.tif"))  # the input stays when nothing was written
    q = str(tmp_path / "u8.tif")
    w = GeoTiffWriter(q, 40, 30, 1, 0.0, 30.0, 1.0)
    w.close()
    with pytest.raises(ValueError, match="overview_resampling"):
        convert_to_cog(q, str(tmp_path / "out.tif"), overview_resampling="cubic")
    assert os.path.isfile(q)


def test_zonal_run_with_cog_conversion(cuda, tmp_path):
    """the file-based zonal set-up of tests/test_zonal_gpu.py on a two-row strip wider than one 512-pixel block: the run
    with cog_conversion writes <name>_COG.tif with the pixels of the plain run and one overview; the class raster's
    overview is the mode, the confidence raster's the average (cog_overview_resampling: mode)"""
    import yaml
    from flair_zonal_detection.config import validate_config
    from flair_zonal_detection.geotiff import GeoTiffRaster, GeoTiffWriter, validate_cog
    from flair_zonal_detection.inference import CONFIDENCE_SUFFIX, run_inference
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    patch, margin, res = 128, 16, 0.2
    g = np.random.default_rng(11)
    img = np.repeat(np.repeat(g.integers(0, 255, (3, 33, 133)), 4, 1), 4, 2)[:, :130, :530].astype(np.uint8)
    ras = ArrayRaster(img, 651992.36, 6860417.84, res)
    src_path = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src_path, ras, 3) as w:
        w.data[...] = img
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    assert cfg["cog_conversion"] is False  # the golden configuration: nothing changes for it
    cfg.update({"output_path": str(tmp_path / "plain"), "output_name": "z", "img_pixels_detection": patch,
                "margin": margin, "output_px_meters": res, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}, "write_confidence": True})
    cfg["modalities"][MOD].update({"input_img_path": src_path, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    oracle = UnetResNet34(3, 19)
    oracle.load_state_dict(fill_state_dict(oracle.state_dict(), seed=5))
    cfg["model_weights"] = str(tmp_path / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])

    plain = run_inference(copy.deepcopy(cfg))
    keys = [TASK, TASK + CONFIDENCE_SUFFIX]
    assert sorted(plain) == sorted(keys)
    pixels = {}
    for key, suffix in zip(keys, ("argmax", "confidence")):
        o = plain[key]
        assert os.path.basename(o.path) == f"z_{TASK}_{suffix}_i.tif" and os.path.isfile(o.path)
        with GeoTiffRaster(o.path) as r:
            pixels[key] = r.read()
            assert r.overview_count == 0
        # the bytes of today: what the plain writer gives for these pixels, IFD behind the data
        again = GeoTiffWriter.like(str(tmp_path / "again.tif"), o, 1)
        again.data[...] = pixels[key]
        again.close()
        assert open(o.path, "rb").read() == open(again.path, "rb").read()
    assert sorted(os.listdir(cfg["output_path"])) == sorted(os.path.basename(plain[k].path) for k in keys)
    assert pixels[TASK].any() and len(np.unique(pixels[TASK])) > 1

    ccfg = copy.deepcopy(cfg)
    ccfg.update({"output_path": str(tmp_path / "cog"), "cog_conversion": True, "cog_overview_resampling": "mode"})
    out = run_inference(ccfg)
    for key, suffix, method in zip(keys, ("argmax", "confidence"), ("mode", "average")):
        path = out[key].path
        assert os.path.basename(path) == f"z_{TASK}_{suffix}_i_COG.tif" and os.path.isfile(path)
        assert validate_cog(path) == []
        levels = _levels_of(path)
        assert len(levels) == 2 and levels[1].shape == (1, 65, 265)
        assert np.array_equal(levels[0], pixels[key])
        assert np.array_equal(levels[1], pyramid(pixels[key], 1, method)[0])
        with GeoTiffRaster(path) as r:
            assert r.crs == ras.crs and tuple(r.bounds) == tuple(ras.bounds) and r.res == (res, res)
    assert sorted(os.listdir(ccfg["output_path"])) == sorted(os.path.basename(out[k].path) for k in keys)

    bad = copy.deepcopy(cfg)
    bad["cog_overview_resampling"] = "cubic"
    with pytest.raises(ValueError, match="cog_overview_resampling"):
        validate_config(bad)
    bad = copy.deepcopy(cfg)
    bad["cog_conversion"] = "yes"
    with pytest.raises(ValueError, match="cog_conversion"):
        validate_config(bad)
