"""Per-polygon confidence on the GPU: label + confidence in one kernel pass (ffa_predict_u8 mode 2), exact per-polygon
sums over the polygoniser's labels (ffa_polygonize_zonal_sum_u8), the tile loop's optional confidence raster and the
``confidence`` / ``pixels`` columns of raster_to_polygons down to the GeoPackage.

Definitions: conf_u8 = rint(255 * max_k softmax(z)_k) in the arithmetic of the class_prob kernel, so it is the maximum
over the bands of the class_prob output of the same pixel; confidence[q] = sum of conf_u8 over the pixels of polygon
q / (255.0 * pixels[q]) in float64.  The sums are integers, so everything below that compares two evaluations of the
same definition asks for equality.  The oracle for the sums is scipy.ndimage.label per class (4-connected) followed by
np.bincount in int64.
"""
import copy
import os
import sqlite3
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import MOD, ROOT, TASK, oracle_to_product_keys

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


# ---- kernel 1: label + confidence ---------------------------------------------------------------------------------------

def to_nhwc(x_nchw, dtype, dev, cp):
    B, C, H, W = x_nchw.shape
    out = torch.full((B, H, W, cp), 7.0, dtype=torch.float32)  # garbage in the pad channels must be ignored
    out[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return out.to(dtype).to(dev).contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,cp", [(2, 8), (5, 8), (19, 24), (19, 32)])
@pytest.mark.parametrize("B,H,W,crop", [
    (1, 24, 20, None),
    (3, 37, 45, (4, 6, 29, 33)),   # batch > 1, odd h and w
    (2, 40, 56, (0, 0, 1, 1)),
    (2, 33, 31, (5, 3, 27, 1)),
])
def test_label_and_confidence_equal_the_argmax_and_class_prob_outputs(cuda, dtype, K, cp, B, H, W, crop):
    from flairhip import ops
    g = torch.Generator().manual_seed(K * 1000 + H)
    z = torch.randn(B, K, H, W, generator=g) * 3
    z[0, :, 0, 0] = 1.25            # all classes tie: lowest index, confidence rint(255 / K)
    z[-1, :, H // 2, W // 2] = -40.0
    z[-1, K - 1, H // 2, W // 2] = 40.0   # a saturated pixel: confidence 255
    zd = to_nhwc(z, dtype, cuda, cp)
    am = ops.predict_u8(zd, K, "argmax", crop)
    cprob = ops.predict_u8(zd, K, "class_prob", crop)
    both = ops.predict_u8(zd, K, "argmax_conf", crop)
    torch.cuda.synchronize()
    h, w = (H, W) if crop is None else crop[2:]
    assert both.shape == (B, 2, h, w) and both.dtype == torch.uint8
    assert torch.equal(both[:, 0], am)
    assert torch.equal(both[:, 1], cprob.max(dim=1).values)
    if crop is None:
        assert int(both[0, 1, 0, 0]) == int(np.rint(255.0 / K)) and int(both[0, 0, 0, 0]) == 0
        assert int(both[-1, 1, H // 2, W // 2]) == 255 and int(both[-1, 0, H // 2, W // 2]) == K - 1
    with pytest.raises(ValueError):
        ops.predict_u8(zd, K, "confidence", crop)


def test_label_and_confidence_on_the_reference_convert_fixture(cuda):
    """the reference's own convert outputs: label exactly; confidence under the bar the project uses for class_prob
    (tests/test_zonal_gpu.py::test_convert_matches_reference_outputs)"""
    from flairhip import ops
    d = np.load(os.path.join(GOLD, "convert.npz"))
    z = torch.from_numpy(d["logits"])[None]
    both = ops.predict_u8(to_nhwc(z, torch.float32, cuda, 24), 19, "argmax_conf").cpu().numpy()
    assert np.array_equal(both[0, 0], d["argmax"][0])
    want = d["class_prob"].max(0)
    diff = np.abs(both[0, 1].astype(int) - want.astype(int))
    z64 = d["logits"].astype(np.float64)
    e = np.exp(z64 - z64.max(0, keepdims=True))
    top = (e / e.sum(0, keepdims=True)).max(0) * 255.0
    print("confidence vs reference class_prob.max: max diff", diff.max(), "share", (diff > 0).mean())
    assert diff.max() <= 1 and (diff > 0).mean() < 2e-3
    assert np.all(np.abs(top[diff > 0] % 1.0 - 0.5) < 1e-3)


# ---- kernel 2: zonal sums -----------------------------------------------------------------------------------------------

def zonal(cls, values, background=None, min_pixels=1):
    from flairhip import ops
    out = ops.polygonize(torch.from_numpy(np.ascontiguousarray(cls, dtype=np.uint8)).cuda(), background, min_pixels,
                         values=torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint8)).cuda())
    torch.cuda.synchronize()
    assert len(out) == 6
    return [t.cpu().numpy() for t in out]


def oracle_sums(cls, values, background=None, min_pixels=1):
    """(class, first pixel, pixel count, int64 sum of values) of every kept 4-connected component, sorted by
    (class, first pixel) = the polygon order"""
    from scipy import ndimage
    rows = []
    for c in np.unique(cls):
        if background is not None and c == background:
            continue
        lab, n = ndimage.label(cls == c)  # default structure: 4-connected
        flat = lab.ravel()
        cnt = np.bincount(flat, minlength=n + 1)
        sums = np.bincount(flat, weights=values.ravel().astype(np.int64), minlength=n + 1).astype(np.int64)
        first = np.empty(n + 1, np.int64)
        first[flat[::-1]] = np.arange(flat.size - 1, -1, -1)  # the last assignment per label is its first pixel
        for k in range(1, n + 1):
            if cnt[k] >= min_pixels:
                rows.append((int(c), int(first[k]), int(cnt[k]), int(sums[k])))
    rows.sort()
    return rows


def first_pixels(pro, rvo, verts, W):
    """row-major index of each polygon's first pixel: the top-left pixel of the exterior's top row"""
    out = []
    for q in range(len(pro) - 1):
        ext = verts[rvo[pro[q]]:rvo[pro[q] + 1]].astype(np.int64)
        top = ext[:, 1].min()
        out.append(int(top * W + ext[ext[:, 1] == top, 0].min()))
    return out


def check_sums(cls, values, background=None, min_pixels=1):
    pc, pp, pro, rvo, verts, sums = zonal(cls, values, background, min_pixels)
    want = oracle_sums(cls, values, background, min_pixels)
    assert sums.dtype == np.int64 and len(sums) == len(pc) == len(want)
    got = list(zip(pc.tolist(), first_pixels(pro, rvo, verts, cls.shape[1]), pp.tolist(), sums.tolist()))
    assert got == want
    return pc, pp, sums


@pytest.mark.parametrize("K", [2, 5, 19])
@pytest.mark.parametrize("bg", [None, 1])
@pytest.mark.parametrize("shape", [(64, 64), (513, 771), (97, 33)])
def test_zonal_sums_on_random_maps_equal_the_label_oracle(cuda, K, bg, shape):
    g = np.random.default_rng(K * 100 + (bg or 0) + shape[0])
    blocky = np.repeat(np.repeat(g.integers(0, K, (shape[0] // 4 + 1, shape[1] // 4 + 1)), 4, 0), 4, 1)
    cls = blocky[:shape[0], :shape[1]]
    noise = g.random(shape) < 0.1
    cls = np.where(noise, g.integers(0, K, shape), cls).astype(np.uint8)
    values = g.integers(0, 256, shape).astype(np.uint8)
    check_sums(cls, values, bg)


def test_zonal_sums_constant_values(cuda):
    g = np.random.default_rng(4)
    cls = np.repeat(np.repeat(g.integers(0, 5, (40, 50)), 5, 0), 5, 1).astype(np.uint8)
    pc, pp, sums = check_sums(cls, np.full(cls.shape, 255, np.uint8), 2)
    assert len(pc) and np.array_equal(sums, 255 * pp)
    pc, pp, sums = check_sums(cls, np.zeros(cls.shape, np.uint8), 2)
    assert not sums.any()


def test_zonal_sums_skip_components_dropped_by_min_pixels(cuda):
    g = np.random.default_rng(6)
    cls = np.where(g.random((300, 400)) < 0.35, g.integers(0, 4, (300, 400)),
                   np.repeat(np.repeat(g.integers(0, 4, (30, 40)), 10, 0), 10, 1)).astype(np.uint8)
    values = g.integers(1, 256, cls.shape).astype(np.uint8)
    everything = oracle_sums(cls, values, 0, 1)
    for k in (2, 9, 50):
        pc, pp, sums = check_sums(cls, values, 0, k)
        kept_total = sum(s for _, _, m, s in everything if m >= k)
        assert 0 < len(pc) < len(everything) and int(sums.sum()) == kept_total


def test_zonal_sums_all_background_writes_nothing(cuda, lib):
    from flairhip import ops
    out = zonal(np.full((40, 50), 7, np.uint8), np.full((40, 50), 200, np.uint8), background=7)
    assert len(out[0]) == 0 and out[5].shape == (0,) and out[5].dtype == np.int64
    # the ABI call itself with P = 0: no write through the (here poisoned) pointer's neighbourhood
    cls = torch.full((40, 50), 7, dtype=torch.uint8, device=cuda)
    nbytes = lib.ffa_polygonize_workspace_bytes(40, 50)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=cuda)
    counts = torch.empty(4, dtype=torch.int64, device=cuda)
    st = ops._stream()
    assert lib.ffa_polygonize_label(cls.data_ptr(), 40, 50, 7, 1, ws.data_ptr(), int(nbytes), counts.data_ptr(), st) == 0
    guard = torch.full((8,), -5, dtype=torch.int64, device=cuda)
    assert int(counts[0]) == 0
    assert lib.ffa_polygonize_zonal_sum_u8(ws.data_ptr(), int(nbytes), 40, 50, cls.data_ptr(), 0, guard.data_ptr(),
                                           st) == 0
    torch.cuda.synchronize()
    assert bool((guard == -5).all())


@pytest.mark.parametrize("shape", [(1, 1), (1, 300), (300, 1)])
def test_zonal_sums_degenerate_shapes(cuda, shape):
    g = np.random.default_rng(shape[0] * 7 + shape[1])
    check_sums(g.integers(0, 3, shape).astype(np.uint8), g.integers(0, 256, shape).astype(np.uint8))


def test_zonal_sums_one_component_over_a_4096_raster(cuda):
    """the contention case: every pixel adds to the same polygon"""
    g = np.random.default_rng(8)
    values = g.integers(0, 256, (4096, 4096)).astype(np.uint8)
    pc, pp, pro, rvo, verts, sums = zonal(np.full((4096, 4096), 3, np.uint8), values)
    assert pc.tolist() == [3] and pp.tolist() == [4096 * 4096]
    assert sums.tolist() == [int(values.astype(np.int64).sum())]


def test_zonal_sums_checkerboard(cuda):
    """the many-tiny-components case: every pixel its own polygon"""
    H, W = 257, 311
    cls = (np.indices((H, W)).sum(0) % 2).astype(np.uint8)
    values = np.random.default_rng(10).integers(0, 256, (H, W)).astype(np.uint8)
    pc, pp, sums = check_sums(cls, values)
    assert len(pc) == H * W and np.all(pp == 1)
    # polygon order = class, then pixel order
    assert np.array_equal(sums, np.concatenate([values[cls == 0], values[cls == 1]]).astype(np.int64))


def test_zonal_sums_concentric_squares_do_not_leak_into_the_enclosing_polygon(cuda):
    cls = np.zeros((20, 20), np.uint8)
    cls[2:18, 2:18] = 1
    cls[5:15, 5:15] = 2
    cls[8:12, 8:12] = 3
    values = np.zeros((20, 20), np.uint8)
    values[cls == 0], values[cls == 1], values[cls == 2], values[cls == 3] = 10, 20, 30, 255
    pc, pp, sums = check_sums(cls, values)
    assert pc.tolist() == [0, 1, 2, 3]
    assert sums.tolist() == [10 * (400 - 256), 20 * (256 - 100), 30 * (100 - 16), 255 * 16]


def test_zonal_sums_are_deterministic_and_leave_the_polygons_alone(cuda):
    from flairhip import ops
    g = np.random.default_rng(9)
    cls = g.integers(0, 4, (700, 900)).astype(np.uint8)
    values = g.integers(0, 256, cls.shape).astype(np.uint8)
    a, b = zonal(cls, values, 3), zonal(cls, values, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    plain = ops.polygonize(torch.from_numpy(cls).cuda(), 3, 1)
    assert len(plain) == 5
    assert all(x.cpu().numpy().tobytes() == y.tobytes() for x, y in zip(plain, a))
    with pytest.raises(ValueError):
        ops.polygonize(torch.from_numpy(cls).cuda(), 3, 1, values=torch.from_numpy(values[:-1]).cuda())
    with pytest.raises(ValueError):
        ops.polygonize(torch.from_numpy(cls).cuda(), 3, 1, values=torch.from_numpy(values).cuda().float())


# ---- tile loop --------------------------------------------------------------------------------------------------------

MEANS, STDS = [105.66, 111.35, 102.18], [52.23, 45.62, 44.30]


def _array_cfg(tmp_path, H, W, out_res, seed=77):
    """the in-memory set-up of tests/test_zonal_gpu.py::test_run_inference_matches_oracle_loop (fp32 mode)"""
    import yaml
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    g = np.random.default_rng(3)
    ras = ArrayRaster(g.integers(0, 255, (3, H, W)).astype(np.uint8), 651992.36, 6860417.84, 0.2)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp_path), "output_name": "z", "img_pixels_detection": 128, "margin": 16,
                "output_px_meters": out_res, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "fp32"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": MEANS, "stds": STDS}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(19)}}]
    oracle = UnetResNet34(3, 19)
    oracle.load_state_dict(fill_state_dict(oracle.state_dict(), seed=seed))
    cfg["model_weights"] = str(tmp_path / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    return cfg, ras, oracle


@pytest.mark.parametrize("H,W,out_res", [(300, 410, 0.2), (100, 90, 0.2), (300, 410, 0.4), (200, 260, 0.1)],
                         ids=["ragged", "tiny", "coarser", "finer"])
def test_confidence_raster_equals_the_class_prob_run_and_leaves_the_class_raster_alone(cuda, tmp_path, H, W, out_res):
    from flair_zonal_detection.inference import run_inference
    cfg, _, _ = _array_cfg(tmp_path, H, W, out_res)
    plain = run_inference(copy.deepcopy(cfg))
    assert sorted(plain) == [TASK]
    with_conf = run_inference(dict(copy.deepcopy(cfg), write_confidence=True))
    assert sorted(with_conf) == sorted([TASK, TASK + "_confidence"])
    off = run_inference(dict(copy.deepcopy(cfg), write_confidence=False))
    assert sorted(off) == [TASK] and np.array_equal(off[TASK].data, plain[TASK].data)
    probs = run_inference(dict(copy.deepcopy(cfg), output_type="class_prob"))[TASK].data
    conf = with_conf[TASK + "_confidence"].data
    assert conf.shape == plain[TASK].data.shape == (1,) + probs.shape[1:] and conf.dtype == np.uint8
    assert np.array_equal(with_conf[TASK].data, plain[TASK].data)
    assert np.array_equal(conf[0], probs.max(0))
    assert conf.any()


def test_confidence_raster_matches_the_cpu_oracle_model(cuda, tmp_path):
    """the oracle loop of test_run_inference_matches_oracle_loop with rint(255 * max softmax) in float64"""
    from flair_zonal_detection.inference import run_inference
    from oracle.tile_bookkeeping import slice_tiles, write_window
    H, W, patch, margin, res = 300, 410, 128, 16, 0.2
    cfg, ras, oracle = _array_cfg(tmp_path, H, W, res)
    got = run_inference(dict(cfg, write_confidence=True))[TASK + "_confidence"].data
    oracle.eval()
    bounds = tuple(ras.bounds)
    canvas = np.zeros_like(got)
    for t in slice_tiles(bounds, bounds, patch, margin, res):
        x = ras.read_bounds([1, 2, 3], t["box"], patch).astype(np.float64)
        for c in range(3):
            x[c] = (x[c] - MEANS[c]) / STDS[c]
        with torch.no_grad():
            logits = oracle(torch.tensor(x[None], dtype=torch.float32))[0].numpy()
        z = logits[:, margin:patch - margin, margin:patch - margin].astype(np.float64)
        e = np.exp(z - z.max(0, keepdims=True))
        p = np.rint(255.0 * (e / e.sum(0, keepdims=True)).max(0)).astype(np.uint8)[None]
        col, row, w, h, skip = write_window(t["left"], t["top"], bounds, res, p.shape[-2], p.shape[-1])
        if not skip:
            canvas[:, row:row + h, col:col + w] = p[:, :h, :w]
    diff = np.abs(got.astype(int) - canvas.astype(int))
    print("confidence raster vs float64 oracle: max diff", diff.max(), "share", (diff > 0).mean())
    assert diff.max() <= 1
    assert got.any()


def test_write_confidence_is_validated(cuda, tmp_path):
    from flair_zonal_detection.inference import run_inference
    cfg, _, _ = _array_cfg(tmp_path, 100, 90, 0.2)
    with pytest.raises(ValueError):
        run_inference(dict(copy.deepcopy(cfg), write_confidence=True, output_type="class_prob"))
    with pytest.raises(ValueError):
        run_inference(dict(copy.deepcopy(cfg), write_confidence="yes"))


def test_sharded_in_memory_runs_merge_the_confidence_raster(cuda, tmp_path):
    from flair_zonal_detection.inference import merge_shard_outputs, run_inference
    cfg, _, _ = _array_cfg(tmp_path, 300, 410, 0.2)
    cfg["write_confidence"] = True
    whole = run_inference(copy.deepcopy(cfg))
    merged = merge_shard_outputs([run_inference(copy.deepcopy(cfg), shard=(r, 3)) for r in range(3)])
    for key in (TASK, TASK + "_confidence"):
        assert np.array_equal(merged[key].data, whole[key].data)


# ---- polygons ---------------------------------------------------------------------------------------------------------

def _rings(gdf):
    return [(int(c), [g.exterior] + list(g.interiors)) for c, g in zip(gdf["class_id"], gdf["geometry"])]


def _same_polygons(a, b):
    ra, rb = _rings(a), _rings(b)
    return len(ra) == len(rb) and all(ca == cb and len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y))
                                      for (ca, x), (cb, y) in zip(ra, rb))


def test_raster_to_polygons_with_confidence_on_run_inference_outputs(cuda, tmp_path):
    from flair_zonal_detection.inference import raster_to_polygons, run_inference
    from flair_zonal_detection.raster import ArrayRaster
    cfg, _, _ = _array_cfg(tmp_path, 300, 410, 0.2)
    outputs = run_inference(dict(cfg, write_confidence=True))
    plain = raster_to_polygons(outputs, n_jobs=4)           # the class raster is still found among two entries
    assert list(plain.columns) == ["class_id", "geometry"]
    gdf = raster_to_polygons(outputs, n_jobs=4, confidence=True)
    assert list(gdf.columns) == ["class_id", "confidence", "pixels", "geometry"]
    assert gdf["confidence"].dtype == np.float64 and gdf["pixels"].dtype == np.int64
    assert len(gdf) > 0 and list(gdf["class_id"]) == list(plain["class_id"]) and _same_polygons(gdf, plain)
    cls, conf = outputs[TASK].data[0], outputs[TASK + "_confidence"].data[0]
    want = oracle_sums(cls, conf, 18, min_pixels=25)        # the defaults: background 18, 1 m^2 = 25 px of 0.2 m
    assert list(gdf["class_id"]) == [c for c, _, _, _ in want]
    pixels = np.array([m for _, _, m, _ in want], np.int64)
    sums = np.array([s for _, _, _, s in want], np.int64)
    assert np.array_equal(gdf["pixels"].to_numpy(), pixels)
    assert np.array_equal(gdf["confidence"].to_numpy(), sums / (255.0 * pixels))
    assert gdf["confidence"].min() >= 0.0 and gdf["confidence"].max() <= 1.0 and gdf["confidence"].max() > 0.0
    # the raster itself instead of True
    direct = raster_to_polygons(outputs[TASK], n_jobs=1, confidence=outputs[TASK + "_confidence"])
    assert np.array_equal(direct["confidence"].to_numpy(), gdf["confidence"].to_numpy()) and _same_polygons(direct, gdf)
    a = outputs[TASK]
    with pytest.raises(ValueError):   # wrong shape
        raster_to_polygons(a, confidence=ArrayRaster(conf[None, :-1], a.left, a.top, 0.2, a.crs))
    with pytest.raises(ValueError):   # two bands
        raster_to_polygons(a, confidence=ArrayRaster(np.stack([conf, conf]), a.left, a.top, 0.2, a.crs))
    with pytest.raises(ValueError):   # not uint8
        raster_to_polygons(a, confidence=ArrayRaster(conf[None].astype(np.uint16), a.left, a.top, 0.2, a.crs))
    with pytest.raises(ValueError):   # other bounds
        raster_to_polygons(a, confidence=ArrayRaster(conf[None], a.left + 0.2, a.top, 0.2, a.crs))
    with pytest.raises(ValueError):   # other resolution
        raster_to_polygons(a, confidence=ArrayRaster(conf[None], a.left, a.top, 0.4, a.crs))
    with pytest.raises(KeyError):     # a run without write_confidence has no such entry
        raster_to_polygons({TASK: a}, confidence=True)


def test_geopackage_carries_confidence_and_pixels(cuda, tmp_path):
    from flair_zonal_detection.inference import raster_to_polygons
    from flair_zonal_detection.raster import ArrayRaster
    g = np.random.default_rng(3)
    cls = np.repeat(np.repeat(g.integers(0, 6, (30, 40)), 5, 0), 5, 1).astype(np.uint8)
    conf = g.integers(0, 256, cls.shape).astype(np.uint8)
    ras = ArrayRaster(cls, 651992.36, 6860417.84, 0.2)
    cras = ArrayRaster(conf, 651992.36, 6860417.84, 0.2)
    gdf = raster_to_polygons(ras, confidence=cras)
    path = str(tmp_path / "conf.gpkg")
    gdf.to_file(path, driver="GPKG")
    con = sqlite3.connect(path)
    cols = [(r[1], r[2]) for r in con.execute('PRAGMA table_info("conf")')]
    rows = con.execute('SELECT class_id, confidence, pixels FROM "conf" ORDER BY fid').fetchall()
    con.close()
    assert cols == [("fid", "INTEGER"), ("geom", "POLYGON"), ("class_id", "INTEGER"), ("confidence", "REAL"),
                    ("pixels", "INTEGER")]
    assert len(rows) == len(gdf) > 0
    assert [r[0] for r in rows] == list(gdf["class_id"])
    assert [r[1] for r in rows] == gdf["confidence"].tolist() and all(isinstance(r[1], float) for r in rows)
    assert [r[2] for r in rows] == gdf["pixels"].tolist() and all(isinstance(r[2], int) for r in rows)
    plain = str(tmp_path / "plain.gpkg")
    raster_to_polygons(ras).to_file(plain, driver="GPKG")
    con = sqlite3.connect(plain)
    assert [(r[1], r[2]) for r in con.execute('PRAGMA table_info("plain")')] == cols[:3]
    con.close()


def test_vectorize_segmentation_parallel_gives_each_polygon_its_own_mean(cuda):
    """two polygons of one class with different confidences: the case the reference's per-class mean gets wrong"""
    from flair_zonal_detection.inference import vectorize_segmentation_parallel
    labels = np.zeros((40, 60), np.uint8)
    labels[5:15, 5:15] = 3     # 100 px
    labels[20:35, 30:50] = 3   # 300 px
    labels[2:4, 50:58] = 7     # 16 px
    conf = np.zeros((40, 60), np.uint8)
    conf[5:15, 5:15] = 51      # 0.2
    conf[20:35, 30:50] = 204   # 0.8
    conf[20, 30] = 0
    conf[2:4, 50:58] = 255
    transform = (0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0)
    gdf = vectorize_segmentation_parallel(labels, conf, transform, simplification_tolerance=0.0)
    assert list(gdf.columns) == ["class_id", "confidence", "pixels", "geometry"] and gdf.crs == "EPSG:5490"
    assert list(gdf["class_id"]) == [3, 3, 7] and list(gdf["pixels"]) == [100, 300, 16]   # class 0 is the background
    assert gdf["confidence"].tolist() == [51 * 100 / (255.0 * 100), (204 * 299) / (255.0 * 300), 1.0]
    assert gdf["geometry"][0].bounds == (1002.5, 1992.5, 1007.5, 1997.5)
    # float confidence is quantised with rint(255 c): the same numbers
    as_float = vectorize_segmentation_parallel(labels, conf.astype(np.float32) / 255.0, transform,
                                               simplification_tolerance=0.0)
    assert as_float["confidence"].tolist() == gdf["confidence"].tolist()

    class Affine:
        a, b, c, d, e, f = transform
    assert vectorize_segmentation_parallel(labels, conf, Affine(), n_jobs=2)["pixels"].tolist() == [100, 300, 16]
    # min_area defaults to 4.0 map units^2 = 16 px here: the 16-px polygon stays, one pixel fewer goes
    labels[2, 50] = 0
    assert list(vectorize_segmentation_parallel(labels, conf, transform)["pixels"]) == [100, 300]


# ---- CLI ------------------------------------------------------------------------------------------------------------

def _file_cfg(tmp_path, seed=21):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    cfg, ras, _ = _array_cfg(tmp_path, 300, 410, 0.2, seed=5)
    src_path = str(tmp_path / "mosaic.tif")
    img = np.random.default_rng(seed).integers(0, 255, (3, 300, 410)).astype(np.uint8)
    with GeoTiffWriter.like(src_path, ras, 3) as w:
        w.data[...] = img
    cfg["modalities"][MOD]["input_img_path"] = src_path
    cfg["hardware"] = {"precision": "bf16"}
    cfg["write_confidence"] = True
    return cfg


def test_cli_polygons_with_confidence_and_two_process_sharded_run(cuda, tmp_path):
    import yaml
    from flair_zonal_detection.geotiff import GeoTiffRaster
    from flair_zonal_detection.inference import raster_to_polygons
    cfg = _file_cfg(tmp_path)
    cfg["output_path"] = str(tmp_path / "one")
    one = str(tmp_path / "one.yaml")
    yaml.safe_dump(cfg, open(one, "w"))
    two_cfg = dict(copy.deepcopy(cfg), output_path=str(tmp_path / "two"))
    two = str(tmp_path / "two.yaml")
    yaml.safe_dump(two_cfg, open(two, "w"))
    pkg = os.path.join(ROOT, "flair-for-aigle_amd")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "flair_zonal_detection.main", "--config"]
    gpkg_path = str(tmp_path / "cli.gpkg")
    subprocess.run(cmd + [one, "--polygons", gpkg_path], env=env, check=True, timeout=300, cwd=pkg)
    names = [f"z_{TASK}_argmax_i.tif", f"z_{TASK}_confidence_i.tif"]
    assert sorted(os.listdir(tmp_path / "one")) == sorted(names)
    # CLI polygons == API polygons of the written rasters
    ref = raster_to_polygons(str(tmp_path / "one" / names[0]), confidence=str(tmp_path / "one" / names[1]))
    ref_path = str(tmp_path / "ref.gpkg")
    ref.to_file(ref_path, driver="GPKG")
    q = 'SELECT fid, geom, class_id, confidence, pixels FROM "{}" ORDER BY fid'
    a = sqlite3.connect(gpkg_path).execute(q.format("cli")).fetchall()
    b = sqlite3.connect(ref_path).execute(q.format("ref")).fetchall()
    assert len(a) == len(ref) > 0 and a == b
    assert [r[3] for r in a] == ref["confidence"].tolist()
    # two processes, rank 0 merges the part files of both rasters
    procs = [subprocess.Popen(cmd + [two], env=dict(env, RANK=str(r), LOCAL_RANK="0", WORLD_SIZE="2"), cwd=pkg)
             for r in range(2)]
    assert [p.wait(timeout=300) for p in procs] == [0, 0]
    for name in names:
        with GeoTiffRaster(str(tmp_path / "one" / name)) as x, GeoTiffRaster(str(tmp_path / "two" / name)) as y:
            ref_data = x.read()
            assert ref_data.any() and np.array_equal(y.read(), ref_data)
            assert x.count == 1 and x.profile["compress"] == "lzw"
    assert sorted(os.listdir(tmp_path / "two")) == sorted(names)  # part files and masks were cleaned up
