"""The sieve filter (csrc/sieve.hip, ops.sieve_, raster_to_polygons(sieve_area=...)) against its semantics restated in
numpy (tests/sieve_oracle.py, pinned by tests/test_sieve_cpu.py).  Every raster comparison is == on every pixel, and
the round count and the three counters are compared for equality as well."""
import logging
import os
import sqlite3

import numpy as np
import pytest
import torch

from helpers import MOD, ROOT, TASK, oracle_to_product_keys
from sieve_oracle import label, sieve, sieve_round

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")


# ---- inputs -------------------------------------------------------------------------------------------------------

def noise(H, W, seed=0):
    """i.i.d. over 3 classes: nearly every component is small"""
    return np.random.default_rng(seed).integers(0, 3, (H, W)).astype(np.uint8)


def voronoi(H, W, p, seed=1, cells=12, classes=6):
    """nearest-seed map of about a dozen cells with salt noise of density p: the benchmark's pattern in small"""
    g = np.random.default_rng(seed)
    sy, sx = g.random(cells) * H, g.random(cells) * W
    lab = g.integers(0, classes, cells)
    yy, xx = np.mgrid[0:H, 0:W]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    out = lab[d.argmin(-1)].astype(np.uint8)
    salt = g.random((H, W)) < p
    out[salt] = g.integers(0, classes, int(salt.sum()))
    return out


def checker(H, W):
    """every component has one pixel and all neighbours tie on the count: the smaller root decides everything"""
    return (np.add.outer(np.arange(H), np.arange(W)) % 2).astype(np.uint8)


INPUTS = {"noise": noise, "voronoi2": lambda H, W: voronoi(H, W, 0.02), "voronoi10": lambda H, W: voronoi(H, W, 0.10),
          "checker": checker}

_oracle_cache = {}


def oracle(cls, T, bg=None, max_rounds=16):
    key = (cls.tobytes(), cls.shape, T, bg, max_rounds)
    if key not in _oracle_cache:
        _oracle_cache[key] = sieve(cls, T, bg, max_rounds)
    out, st = _oracle_cache[key]
    return out.copy(), dict(st)


def product(cuda, cls, T, bg=None, **kw):
    from flairhip import ops
    x = torch.from_numpy(cls).to(cuda)
    st = ops.sieve_(x, T, background=bg, **kw)
    return x.cpu().numpy(), st


def check(cuda, cls, T, bg=None, max_rounds=16):
    want, want_st = oracle(cls, T, bg, max_rounds)
    got, got_st = product(cuda, cls, T, bg, max_rounds=max_rounds)
    assert got.shape == want.shape and (got == want).all(), f"{int((got != want).sum())} pixels differ"
    assert got_st == want_st
    return got, got_st


# ---- shapes, thresholds, background -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(INPUTS))
@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (70, 1), (33, 65), (97, 131)])
def test_shapes_against_the_oracle(cuda, H, W, name):
    # the checkerboard never converges within a cap (see below): four rounds of it show what sixteen would
    check(cuda, INPUTS[name](H, W), 5, max_rounds=4 if name == "checker" else 16)


@pytest.mark.parametrize("bg", [None, 0, 2])
@pytest.mark.parametrize("T", [0, 1, 2, 5, 50, 33 * 65 + 1])
@pytest.mark.parametrize("name", ["noise", "voronoi10"])
def test_thresholds_and_background(cuda, name, T, bg):
    cls = INPUTS[name](33, 65)
    got, st = check(cuda, cls, T, bg)
    if T <= 1:
        assert st["rounds"] == 0 and (got == cls).all()


def test_several_tiles_in_both_directions(cuda):
    _, st = check(cuda, voronoi(257, 300, 0.02), 5)
    assert st["relabelled_pixels"] > 1000 and st["rounds"] < 16


def test_checkerboard_runs_into_the_cap_and_says_so(cuda, caplog):
    # one-pixel components tie everywhere: each takes the class of the neighbour with the smaller root, the board
    # flips, and only the corner grows -- far more than 16 rounds
    with caplog.at_level(logging.WARNING, logger="flairhip.ops"):
        _, st = check(cuda, checker(33, 65), 2)
    assert st["rounds"] == 16 and st["remaining_small"] > 0
    assert any("max_rounds" in r.getMessage() for r in caplog.records)


# ---- constructed cases at 40 x 70 ---------------------------------------------------------------------------------------

CH, CW = 40, 70


def test_island_across_a_tile_corner_is_absorbed(cuda):
    cls = np.full((CH, CW), 4, np.uint8)
    cls[31:33, 31:33] = 9  # one pixel in each of the four tiles that meet at (32, 32)
    got, st = check(cuda, cls, 5)
    assert (got == 4).all() and st["relabelled_pixels"] == 4 and st["relabelled_components"] == 1


def test_components_touching_at_a_corner_do_not_vote_for_each_other(cuda):
    cls = np.zeros((CH, CW), np.uint8)
    cls[10, 10] = 2
    cls[11, 11:13] = 3
    cls[31, 31] = 5  # the same across the tile corner
    cls[32, 32] = 6
    got, st = check(cuda, cls, 5, bg=0)
    assert (got == cls).all() and st["relabelled_pixels"] == 0 and st["remaining_small"] == 4


def test_chain_uses_the_classes_of_the_start_of_the_round(cuda):
    cls = np.zeros((CH, CW), np.uint8)
    cls[5:30, 40:60] = 4            # large
    cls[20, 30:40] = 3              # S3: 10 pixels, touches the large one
    cls[20, 25:30] = 2              # S2: 5
    cls[20, 23:25] = 1              # S1: 2
    one, st = check(cuda, cls, 20, bg=0, max_rounds=1)
    assert one[20, 23:40].tolist() == [2] * 2 + [3] * 5 + [4] * 10 and st["relabelled_components"] == 3
    got, st = check(cuda, cls, 20, bg=0)
    assert (got[20, 23:40] == 4).all() and st["rounds"] == 4


def test_equal_sizes_the_smaller_root_wins(cuda):
    cls = np.zeros((CH, CW), np.uint8)
    cls[31:33, 20:24] = 1
    cls[31:33, 24:28] = 2           # same size, larger root: takes class 1; the first stays
    one, _ = check(cuda, cls, 9, bg=0, max_rounds=1)
    assert (one[31:33, 20:28] == 1).all()
    # vertically: the upper one has the smaller root
    cls = np.zeros((CH, CW), np.uint8)
    cls[30:32, 33:36] = 7
    cls[32:34, 33:36] = 8
    one, _ = check(cuda, cls, 7, bg=0, max_rounds=1)
    assert (one[30:34, 33:36] == 7).all()


def test_small_component_enclosed_by_background_stays(cuda):
    cls = np.full((CH, CW), 1, np.uint8)
    cls[8:13, 30:36] = 0
    cls[10, 32:34] = 5
    got, st = check(cuda, cls, 5, bg=0)
    assert (got == cls).all() and st == {"rounds": 1, "relabelled_components": 0, "relabelled_pixels": 0,
                                          "remaining_small": 1}


def test_raster_of_one_small_component_is_a_no_op(cuda):
    cls = np.full((CH, CW), 3, np.uint8)
    got, st = check(cuda, cls, CH * CW + 1)
    assert (got == 3).all() and st["rounds"] == 1 and st["remaining_small"] == 1


def test_all_small_with_a_strict_maximum(cuda):
    cls = np.zeros((CH, CW), np.uint8)
    cls[:, 30:] = 1
    cls[:, 50:] = 2
    cls[:, 62:] = 3                 # 1200, 800, 480 and 320 pixels, all below the threshold
    got, st = check(cuda, cls, CH * CW + 1)
    assert (got == 0).all() and st["remaining_small"] == 1


# ---- properties, on the product alone ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bg", [None, 0])
@pytest.mark.parametrize("T", [5, 50])
def test_properties_on_noise(cuda, T, bg):
    cls = noise(97, 131, seed=3)
    got, st = product(cuda, cls, T, bg, max_rounds=64)
    assert st["rounds"] < 64                                   # it converged (3 to 7 rounds on such maps)
    assert got.shape == cls.shape and got.dtype == np.uint8
    if bg is not None:
        assert ((got == bg) == (cls == bg)).all()              # background neither changes nor spreads
    lab, counts = label(cls, bg)
    big = np.isin(lab, [r for r, n in counts.items() if n >= T])
    assert (got[big] == cls[big]).all()
    assert int((got != cls).sum()) <= st["relabelled_pixels"]  # a pixel may be relabelled in more than one round
    again, st2 = product(cuda, got, T, bg, max_rounds=64)
    assert st2["relabelled_pixels"] == 0 and st2["rounds"] == 1 and (again == got).all()
    assert st2["remaining_small"] == st["remaining_small"]
    twice, st3 = product(cuda, cls, T, bg, max_rounds=64)
    assert twice.tobytes() == got.tobytes() and st3 == st


def test_max_rounds_1_is_one_oracle_round(cuda, caplog):
    cls = noise(97, 131, seed=4)
    want, counts = sieve_round(cls, 5)
    with caplog.at_level(logging.WARNING, logger="flairhip.ops"):
        got, st = product(cuda, cls, 5, max_rounds=1)
    assert (got == want).all()
    assert (st["rounds"], st["relabelled_components"], st["relabelled_pixels"]) == (1, counts[1], counts[2])
    assert st == oracle(cls, 5, None, 1)[1]
    assert oracle(cls, 5)[1]["rounds"] > 2                     # more were needed
    assert any("max_rounds" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="flairhip.ops"):
        product(cuda, cls, 5)
    assert not caplog.records


def test_one_round_counters_of_the_abi(cuda, lib):
    from flairhip import lib as L
    cls = voronoi(97, 131, 0.10)
    want, counts = sieve_round(cls, 5, 2)
    x = torch.from_numpy(cls).to(cuda)
    n = lib.ffa_sieve_workspace_bytes(97, 131)
    ws = torch.full((n,), 0xA5, dtype=torch.uint8, device=cuda)  # the workspace's contents do not matter
    out = torch.empty(4, dtype=torch.int64, device=cuda)
    L.check(lib.ffa_sieve_round_u8(x.data_ptr(), 97, 131, 2, 5, ws.data_ptr(), n, out.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream))
    assert out.cpu().tolist() == counts and (x.cpu().numpy() == want).all()
    rc = lib.ffa_sieve_round_u8(x.data_ptr(), 97, 131, 2, 5, ws.data_ptr(), n - 1, out.data_ptr(), None)
    assert rc == -3 and b"workspace" in lib.ffa_last_error()


# ---- argument errors ----------------------------------------------------------------------------------------------------

def test_argument_errors(cuda):
    from flairhip import ops
    good = torch.zeros((8, 8), dtype=torch.uint8, device=cuda)
    for bad, T in ((good.to(torch.int32), 2), (good.cpu(), 2), (good[None], 2), (good, -1), (good.t()[:, :4], 2)):
        with pytest.raises(ValueError, match="sieve_"):
            ops.sieve_(bad, T)
    with pytest.raises(ValueError, match="background"):
        ops.sieve_(good, 2, background=256)
    with pytest.raises(ValueError, match="max_rounds"):
        ops.sieve_(good, 2, max_rounds=0)
    assert not good.any()
    assert ops.sieve_(torch.zeros((0, 8), dtype=torch.uint8, device=cuda), 5)["rounds"] == 0


# ---- raster_to_polygons(sieve_area=...) -----------------------------------------------------------------------------------

RH, RW, RES, LEFT, TOP = 97, 131, 0.2, 651992.4, 6860417.8
AREA, AREA_PIXELS = 0.18, 5  # 4 pixels of 0.04 m2 are below 0.18 m2, 5 are not


def frames_equal(a, b):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for col in a.columns:
        if col == "geometry":
            for ga, gb in zip(a[col], b[col]):
                ra, rb = [ga.exterior] + list(ga.interiors), [gb.exterior] + list(gb.interiors)
                assert len(ra) == len(rb) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ra, rb))
        else:
            assert a[col].to_numpy().tobytes() == b[col].to_numpy().tobytes(), col
    return True


def n_rings(frame):
    return sum(1 + len(list(g.interiors)) for g in frame["geometry"])


@pytest.mark.parametrize("classes", [[4], None], ids=["one-class", "all-classes"])
def test_raster_to_polygons_with_sieve_area_equals_the_presieved_raster(cuda, classes):
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    cls = voronoi(RH, RW, 0.10, seed=5)
    conf = np.random.default_rng(8).integers(0, 256, (RH, RW)).astype(np.uint8)
    pre, st = oracle(cls, AREA_PIXELS, 5)
    assert st["relabelled_pixels"] > 100
    ras, ras_pre = ArrayRaster(cls[None], LEFT, TOP, RES), ArrayRaster(pre[None], LEFT, TOP, RES)
    cras = ArrayRaster(conf[None], LEFT, TOP, RES)
    kw = dict(background_value=5, min_area=0.0, simplification=0.0, classes=classes, confidence=cras)
    got = raster_to_polygons(ras, sieve_area=AREA, **kw)
    want = raster_to_polygons(ras_pre, **kw)
    assert len(want) > 3 and frames_equal(got, want)
    assert list(got.columns) == ["class_id", "confidence", "pixels", "geometry"]
    plain = raster_to_polygons(ras, **kw)
    assert n_rings(got) < n_rings(plain) and len(got) < len(plain)
    if classes is not None:
        assert int(got["pixels"].sum()) == int((pre == classes[0]).sum())
    # with the defaults (min_area, simplification) and no confidence columns as well
    kw = dict(background_value=5, classes=classes)
    assert frames_equal(raster_to_polygons(ras, sieve_area=AREA, **kw), raster_to_polygons(ras_pre, **kw))
    # 0 is today's call, and the input raster is not modified
    assert frames_equal(raster_to_polygons(ras, sieve_area=0, **kw), raster_to_polygons(ras, **kw))
    assert np.array_equal(ras.data[0], cls)


# ---- the command line ---------------------------------------------------------------------------------------------------

ZH, ZW = 200, 260


def test_cli_sieve_area(cuda, tmp_path):
    """the smallest multi-tile configuration of tests/test_zone_gpu.py through main(), GeoPackage read back"""
    import yaml
    from flair_zonal_detection.geotiff import GeoTiffRaster, GeoTiffWriter
    from flair_zonal_detection.gpkg import parse_blob
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.main import main
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(1, 255, (3, ZH, ZW)).astype(np.uint8), 651992.4, 6860417.8, 0.2)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp_path), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": 0.2, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "bf16"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [100.0] * 3, "stds": [50.0] * 3}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    net = UnetResNet34(3, 19)
    net.load_state_dict(fill_state_dict(net.state_dict(), seed=5))
    cfg["model_weights"] = str(tmp_path / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(net.state_dict()).items()}},
               cfg["model_weights"])

    area = 2.0  # 50 pixels of 0.04 m2
    src = str(tmp_path / "mosaic.tif")
    with GeoTiffWriter.like(src, ras, 3) as w:
        w.data[...] = ras.data
    cfg["modalities"][MOD]["input_img_path"] = src
    ypath = str(tmp_path / "zonal.yaml")
    with open(ypath, "w") as f:
        yaml.safe_dump(cfg, f)
    gpkg = str(tmp_path / "polygons.gpkg")
    main(["--config", ypath, "--polygons", gpkg, "--sieve-area", str(area)])

    # expected: the class raster the run wrote, sieved by the oracle, through today's raster_to_polygons
    with GeoTiffRaster(str(tmp_path / f"z_{TASK}_argmax_i.tif")) as r:
        data = r.read(1)
        plain = raster_to_polygons(r)
    pre, st = oracle(data, 50, 18)
    assert st["relabelled_pixels"] > 0
    want = raster_to_polygons(ArrayRaster(pre[None], 651992.4, 6860417.8, 0.2))
    assert len(want) > 0 and want["class_id"].tolist() != plain["class_id"].tolist()
    con = sqlite3.connect(gpkg)
    try:
        table = con.execute("SELECT table_name FROM gpkg_contents").fetchone()[0]
        rows = con.execute(f'SELECT class_id, geom FROM "{table}" ORDER BY fid').fetchall()
    finally:
        con.close()
    assert [r[0] for r in rows] == want["class_id"].tolist()
    for (_, blob), geom in zip(rows, want["geometry"]):  # every ring, every vertex
        rings = parse_blob(blob)[2]
        expected = [geom.exterior] + list(geom.interiors)
        assert len(rings) == len(expected)
        assert all(np.array_equal(a, np.asarray(b)) for a, b in zip(rings, expected))
