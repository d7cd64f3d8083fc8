"""The data side of training from a FLAIR-HUB dataset on disk, without a GPU: flair_dataset and pad_collate_flair
against tests/golden/train_batch.npz (the reference's own outputs, tests/golden/gen_train_batch_golden.py) from patches
written here as GeoTIFF, the CSV and GeoPackage readers, norm's error paths, and the rules of the data module -- fixed
rank shares, reproducible epoch permutations, the cache budget."""
import csv
import json
import os
import sqlite3

import numpy as np
import pytest
import torch

from helpers import ROOT

GOLD = os.path.join(ROOT, "tests", "golden")
TASK, K = "AERIAL_LABEL-COSIA", 19


def write_tif(path, arr):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    w = GeoTiffWriter(str(path), arr.shape[2], arr.shape[1], arr.shape[0], 800000.0, 6500000.0, 0.2, crs="EPSG:2154",
                      dtype=arr.dtype)
    w.data[:] = arr
    w.close()


def write_gpkg(path, dates_by_patch, extra=None):
    """a minimal GeoPackage: gpkg_contents naming one feature table with patch_id and acquisition_dates (JSON)"""
    con = sqlite3.connect(str(path))
    con.execute("CREATE TABLE gpkg_contents (table_name TEXT PRIMARY KEY, data_type TEXT NOT NULL, identifier TEXT)")
    con.execute("CREATE TABLE other (fid INTEGER PRIMARY KEY, name TEXT)")
    con.execute("INSERT INTO gpkg_contents VALUES ('other', 'attributes', 'other')")
    con.execute("CREATE TABLE mtd (fid INTEGER PRIMARY KEY, geom BLOB, patch_id TEXT, acquisition_dates TEXT)")
    con.execute("INSERT INTO gpkg_contents VALUES ('mtd', 'features', 'mtd')")
    for pid, days in {**dates_by_patch, **(extra or {})}.items():
        con.execute("INSERT INTO mtd (geom, patch_id, acquisition_dates) VALUES (?, ?, ?)",
                    (b"", pid, json.dumps({str(i): d for i, d in enumerate(days)})))
    con.commit()
    con.close()


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "train_batch.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD, "train_batch.npz"))


@pytest.fixture(scope="module")
def on_disk(gold, tmp_path_factory):
    """the golden's input patches as GeoTIFF files, the split CSV and the dates GeoPackage"""
    meta, z = gold
    root = tmp_path_factory.mktemp("flair_hub")
    for mod, files in meta["files"].items():
        for name in files:
            write_tif(root / name, z["in/" + name])
    cols = list(meta["files"])
    with open(root / "split.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(cols)
        for i in range(len(meta["areas"])):
            w.writerow([str(root / meta["files"][c][i]) for c in cols])
    write_gpkg(root / "GLOBAL_SENTINEL2_MTD_DATES.gpkg", meta["dates"], extra={"D999-2020_XX-S9-9_9-9": ["20200101"]})
    return root


def config_of(meta, setting, root):
    cfg = json.loads(json.dumps(meta["settings"][setting]["config"]))
    cfg["paths"] = {"train_csv": str(root / "split.csv"), "val_csv": str(root / "split.csv"),
                    "test_csv": str(root / "split.csv"), "global_mtd_folder": str(root) + os.sep}
    cfg["tasks"] = {"train": True, "predict": True}
    cfg["hyperparams"] = {"seed": 7, "batch_size": 2}
    return cfg


# ---- 1. the reference schema, bit for bit -------------------------------------------------------------------------------


@pytest.mark.parametrize("setting", ["dem_raw", "dem_elev", "dem_stack", "s2"])
def test_flair_dataset_and_collate_reproduce_the_reference(gold, on_disk, setting):
    from flair_hub.data.dataloader import flair_dataset
    from flair_hub.data.utils_data.padding import pad_collate_flair
    from flair_hub.data.utils_data.paths import get_datasets
    meta, z = gold
    cfg = config_of(meta, setting, on_disk)
    train, _val, _test = get_datasets(cfg)
    ds = flair_dataset(cfg, train, use_augmentations=None, device_prepare=False)
    assert len(ds) == 4
    samples = [ds[i] for i in range(4)]
    want = meta["settings"][setting]
    for i, s in enumerate(samples):
        assert list(s.keys()) == want["keys"]
        assert os.path.basename(s[f"ID_{TASK}"]) == os.path.basename(want["ids"][i])
        for k, v in s.items():
            if not torch.is_tensor(v):
                continue
            assert v.dtype == torch.float32
            if k == TASK:
                ref = np.unpackbits(z[f"{setting}/{i}/{k}"])[:K * 64 * 64].reshape(K, 64, 64).astype(np.float32)
            else:
                ref = z[f"{setting if k != 'AERIAL_RGBI' else 'dem_raw'}/{i}/{k}"]
            assert v.shape == ref.shape and np.array_equal(v.numpy(), ref), (setting, i, k)
    out = pad_collate_flair(samples)
    assert list(out.keys()) == want["collate_keys"]
    for k, v in out.items():
        if not torch.is_tensor(v):
            assert [os.path.basename(p) for p in v] == [os.path.basename(p) for p in want["ids"]]
        elif k == "AERIAL_RGBI":
            assert torch.equal(v, torch.stack([s[k] for s in samples]))
        elif k == TASK:
            ref = np.unpackbits(z[f"{setting}/collate/{k}"])[:4 * K * 64 * 64].reshape(4, K, 64, 64)
            assert np.array_equal(v.numpy(), ref.astype(np.float32))
            assert np.array_equal(v.argmax(1).numpy().astype(np.uint8), z[f"{setting}/collate/argmax_{TASK}"])
        else:
            assert np.array_equal(v.numpy(), z[f"{setting}/collate/{k}"]), (setting, k)


@pytest.mark.parametrize("setting", ["dem_raw", "dem_elev", "dem_stack"])
def test_device_prepare_yields_what_was_decoded(gold, on_disk, setting):
    """raw bands, the 2-band DEM where a kernel takes the difference, the raw label channel as uint8; and the label rule
    of the device (v < K stays, else 0) is the argmax of the reference's one-hot planes"""
    from flair_hub.data.dataloader import flair_dataset
    from flair_hub.data.utils_data.paths import get_paths
    meta, z = gold
    cfg = config_of(meta, setting, on_disk)
    ds = flair_dataset(cfg, get_paths(cfg, "train"), use_augmentations=True, device_prepare=True)
    for i in range(4):
        s = ds[i]
        f = {m: meta["files"][m][i] for m in meta["files"]}
        assert s["AERIAL_RGBI"].dtype == torch.uint8 and np.array_equal(s["AERIAL_RGBI"].numpy(), z["in/" + f["AERIAL_RGBI"]])
        dem = z["in/" + f["DEM_ELEV"]]
        want = np.stack([dem[0], dem[0] - dem[1]]) if setting == "dem_stack" else dem
        assert s["DEM_ELEV"].dtype == torch.float32 and np.array_equal(s["DEM_ELEV"].numpy(), want)
        raw = z["in/" + f[TASK]]
        assert s[TASK].dtype == torch.uint8 and np.array_equal(s[TASK].numpy(), raw[0])
        assert np.array_equal(np.where(raw[0] < K, raw[0], 0), z[f"{setting}/collate/argmax_{TASK}"][i])
        assert (raw >= K).any() and (raw == 255).any()
    nv = ds.norm_vectors()
    assert nv["AERIAL_RGBI"].shape == (2, 5) and nv["DEM_ELEV"].shape == (2, {"dem_raw": 2, "dem_elev": 1, "dem_stack": 2}[setting])
    ds.keep_dem_bands = True  # the store's filler: always both bands
    assert np.array_equal(ds[0]["DEM_ELEV"].numpy(), z["in/" + meta["files"]["DEM_ELEV"][0]])


# ---- 2. file lists and dates ---------------------------------------------------------------------------------------------


def test_get_paths_and_get_datasets(gold, on_disk):
    from flair_hub.data.utils_data.paths import extract_sentinel_patch_ids, get_datasets, get_paths
    meta, _ = gold
    cfg = config_of(meta, "s2", on_disk)
    p = get_paths(cfg, "train")
    assert [os.path.basename(x) for x in p["AERIAL_RGBI"]] == meta["files"]["AERIAL_RGBI"]
    assert [os.path.basename(x) for x in p[TASK]] == meta["files"][TASK]
    assert p["DEM_ELEV"] == [] and len(p["SENTINEL2_MSK-SC"]) == 4  # inactive: empty; the masks come with Sentinel-2
    assert extract_sentinel_patch_ids([p, None]) == set(meta["areas"])
    assert get_paths(config_of(meta, "dem_elev", on_disk), "val")["SENTINEL2_MSK-SC"] == []
    with pytest.raises(SystemExit):
        get_paths(cfg, "holdout")
    bad = config_of(meta, "s2", on_disk)
    bad["paths"]["val_csv"] = str(on_disk / "missing.csv")
    with pytest.raises(SystemExit):
        get_paths(bad, "val")
    train, val, test = get_datasets(cfg)
    assert set(train["DATES_S2"]) == set(meta["areas"]) and train["DATES_S1_ASC"] == {} and test["DATES_S2"] is train["DATES_S2"]
    cfg["tasks"] = {"train": False, "predict": True}
    train, val, test = get_datasets(cfg)
    assert train is None and val is None and len(test[TASK]) == 4


def test_prepare_sentinel_dates_reads_the_geopackage(gold, on_disk, tmp_path):
    import datetime
    from flair_hub.data.utils_data.sentinel_dates import get_sentinel_dates_mtd, prepare_sentinel_dates
    meta, _ = gold
    cfg = config_of(meta, "s2", on_disk)
    got = prepare_sentinel_dates(cfg, str(on_disk / "GLOBAL_SENTINEL2_MTD_DATES.gpkg"), set(meta["areas"][:3]))
    assert set(got) == set(meta["areas"][:3])  # the rest of the table is not asked for
    for area in meta["areas"][:3]:
        days = [datetime.datetime.strptime(d, "%Y%m%d") for d in meta["dates"][area]]
        assert list(got[area]["dates"]) == days
        assert got[area]["diff_dates"].tolist() == [(d - datetime.datetime(d.year, 5, 15)).days for d in days]
    write_gpkg(tmp_path / "odd.gpkg", {"p": ["20210230", "20210301"]})  # 30 February: logged and left out
    odd = prepare_sentinel_dates(cfg, str(tmp_path / "odd.gpkg"), {"p"})
    assert odd["p"]["diff_dates"].tolist() == [(datetime.datetime(2021, 3, 1) - datetime.datetime(2021, 5, 15)).days]
    s2, s1a, s1d = get_sentinel_dates_mtd(cfg, set(meta["areas"]))
    assert set(s2) == set(meta["areas"]) and s1a == {} and s1d == {}
    assert get_sentinel_dates_mtd(config_of(meta, "dem_raw", on_disk), set()) == ({}, {}, {})
    con = sqlite3.connect(str(tmp_path / "none.gpkg"))
    con.execute("CREATE TABLE gpkg_contents (table_name TEXT, data_type TEXT, identifier TEXT)")
    con.commit()
    con.close()
    with pytest.raises(ValueError):
        prepare_sentinel_dates(cfg, str(tmp_path / "none.gpkg"), {"p"})


def test_read_patch_selects_one_based_channels(gold, on_disk):
    from flair_hub.data.utils_data.io import read_patch
    meta, z = gold
    name = meta["files"]["AERIAL_RGBI"][1]
    assert np.array_equal(read_patch(str(on_disk / name)), z["in/" + name])
    assert np.array_equal(read_patch(str(on_disk / name), [4, 1]), z["in/" + name][[3, 0]])
    s2 = meta["files"]["SENTINEL2_TS"][1]
    got = read_patch(str(on_disk / s2))
    assert got.dtype == np.uint16 and np.array_equal(got, z["in/" + s2])


# ---- 3. norm ---------------------------------------------------------------------------------------------------------------


def test_norm_rules_and_error_paths():
    from flair_hub.data.utils_data.norm import norm
    x = np.arange(24, dtype=np.uint8).reshape(2, 3, 4)
    got = norm(x, "custom", [1.5, 2.0], [0.5, 4.0])
    want = x.astype(np.float64)
    want[0] = (want[0] - 1.5) / 0.5
    want[1] = (want[1] - 2.0) / 4.0
    assert got.dtype == np.float64 and np.array_equal(got, want) and x.dtype == np.uint8
    assert norm(x, "without") is x
    assert np.array_equal(norm(x, "scaling"), x / 255.0)
    u16 = np.array([[[0, 65535, 100]]], dtype=np.uint16)
    assert np.array_equal(norm(u16, "scaling"), u16 / 65535.0)
    f = np.ones((1, 2, 2), dtype=np.float32)
    assert norm(f, "scaling") is f
    with pytest.raises(ValueError):
        norm(x.astype(np.int16), "scaling")  # skimage's rule for signed integers is not restated
    with pytest.raises(SystemExit):
        norm(x, "zscore")
    with pytest.raises(SystemExit):
        norm(x, None)
    with pytest.raises(SystemExit):
        norm(x, "custom", [1.0, 2.0], [1.0])


def test_elevation_and_label_helpers():
    from flair_hub.data.utils_data.elevation import calc_elevation
    from flair_hub.data.utils_data.label import reshape_label_ohe
    z = np.random.RandomState(0).randn(2, 5, 6).astype(np.float32)
    e = calc_elevation(z)
    assert e.shape == (1, 5, 6) and e.dtype == np.float32 and np.array_equal(e[0], z[0] - z[1])
    lab = np.array([[[0, 3, 4, 255], [2, 1, 5, 3]]], dtype=np.uint8)
    ohe = reshape_label_ohe(lab, 4)
    assert ohe.shape == (4, 2, 4) and ohe.dtype == bool and not ohe[:, 0, 2].any()  # 4 >= K: true in no plane
    assert np.array_equal(ohe.argmax(0), [[0, 3, 0, 0], [2, 1, 0, 3]])


def test_host_augmentation_draws_and_applies_what_the_reference_does():
    """tests/golden/augment_d4.npz holds the reference's outputs per seed, and the next rand() after the call"""
    from flair_hub.data.utils_data.augmentations import apply_numpy_augmentations
    d = np.load(os.path.join(GOLD, "augment_d4.npz"))
    keys = ["AERIAL_RGBI", "DEM_ELEV", "SENTINEL2_TS"]
    for seed, code, nxt in zip(d["seeds"], d["codes"], d["next_rand"]):
        np.random.seed(int(seed))
        out = apply_numpy_augmentations({k: d["in_" + k].copy() for k in keys + [TASK]}, keys, [TASK])
        assert np.random.rand() == nxt
        for k in keys + [TASK]:
            assert out[k].dtype == d["in_" + k].dtype and np.array_equal(out[k], d[f"out{int(code):02d}_{k}"])


# ---- 4. the data module's rules ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,world", [(8, 1), (8, 2), (10, 4), (3, 4), (17, 3)])
def test_rank_shares_are_disjoint_and_cover_the_split(n, world):
    from flair_hub.data.datamodule import rank_share
    shares = [rank_share(n, r, world) for r in range(world)]
    assert sorted(np.concatenate(shares).tolist()) == list(range(n))
    assert sum(len(s) for s in shares) == n  # disjoint
    assert all(s.tolist() == list(range(r, n, world)) for r, s in enumerate(shares))  # fixed: no seed, no epoch


def test_epoch_permutations_are_reproducible_and_differ_between_epochs():
    from flair_hub.data.datamodule import RankShareLoader, epoch_permutation
    p = epoch_permutation(50, 7, 1, 3)
    assert sorted(p.tolist()) == list(range(50))
    assert np.array_equal(p, epoch_permutation(50, 7, 1, 3))
    others = [epoch_permutation(50, 7, 1, 4), epoch_permutation(50, 7, 0, 3), epoch_permutation(50, 8, 1, 3)]
    assert all(not np.array_equal(p, o) for o in others)
    seen = []
    loader = RankShareLoader(10, 4, lambda pos: {"pos": pos.tolist()}, shuffle=True, drop_last=True, seed=7, rank=1)
    assert len(loader) == 2 and loader.rank_sharded
    for epoch in (0, 1, 0):
        loader.set_epoch(epoch)
        seen.append([b["pos"] for b in loader])
    assert seen[0] == seen[2] != seen[1]
    assert sum(seen[0], []) == epoch_permutation(10, 7, 1, 0)[:8].tolist()
    val = RankShareLoader(10, 4, lambda pos: {"pos": pos.tolist()}, shuffle=False, drop_last=False)
    assert [b["pos"] for b in val] == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9]] and len(val) == 3


def _data_module(meta, root, **kw):
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    cfg = config_of(meta, "dem_elev", root)
    train, val, test = get_datasets(cfg)
    return cfg, FlairDataModule(cfg, train, val, test, num_workers=0, batch_size=2, drop_last=True,
                                use_augmentations=False, **kw)


def test_cache_budget_rule_falls_back_when_the_store_does_not_fit(gold, on_disk, monkeypatch, caplog):
    """the store is all or nothing: 8 patches (4 train + 4 validation) of 5 * 64 * 64 + 2 * 16 * 16 * 4 + 64 * 64 bytes;
    the default budget is 60 % of what the device reports free.  The device is mocked: mem_get_info answers here, and
    the store is allocated on the host."""
    from flairhip.sample_store import SampleStore
    meta, z = gold
    per_patch = 5 * 64 * 64 + 2 * 16 * 16 * 4 + 64 * 64
    need = 8 * per_patch
    # an explicit budget one byte short
    _, dm = _data_module(meta, on_disk, cache="device", cache_bytes=need - 1, device="cpu")
    with caplog.at_level("INFO", logger="flair_hub.data.datamodule"):
        dm.setup("fit")
    assert dm.store is None and "falling back" in caplog.text
    batch = next(iter(dm.train_dataloader()))
    assert "INDEX" not in batch and batch["AERIAL_RGBI"].dtype == torch.uint8  # the streamed raw schema
    assert batch["AERIAL_RGBI_NORM"].shape == (2, 5) and batch["DEM_ELEV_NORM"].shape == (2, 1) and "RAW_LABELS" in batch
    assert batch["DEM_ELEV"].shape == (2, 2, 16, 16) and batch[TASK].dtype == torch.uint8 and len(batch[f"ID_{TASK}"]) == 2
    # the default budget: 60 % of the free device memory at that moment
    for free, fits in ((int(need / 0.6) + 2, True), (int(need / 0.6) - 2, False)):
        monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None, free=free: (free, 4 * free))
        _, dm = _data_module(meta, on_disk, cache="device", device="cpu")
        dm.setup("fit")
        assert (dm.store is not None) == fits
    # exactly enough: the store is built and holds what was decoded, train share first, then validation
    _, dm = _data_module(meta, on_disk, cache="device", cache_bytes=need, device="cpu")
    dm.setup("fit")
    assert isinstance(dm.store, SampleStore) and dm.store.bytes == need and dm.store.fits(need) and not dm.store.fits(need - 1)
    assert dm.store.n == 8 and dm.store.filled == 8 and dm.input_img_sizes() == {"AERIAL_RGBI": 64, "DEM_ELEV": 16}
    for slot in range(8):
        i = slot % 4
        assert np.array_equal(dm.store.inputs["AERIAL_RGBI"][slot].numpy(), z["in/" + meta["files"]["AERIAL_RGBI"][i]])
        assert np.array_equal(dm.store.inputs["DEM_ELEV"][slot].numpy(), z["in/" + meta["files"]["DEM_ELEV"][i]])
        assert np.array_equal(dm.store.labels[TASK][slot].numpy(), z["in/" + meta["files"][TASK][i]][0])
    assert dm.store.channels("DEM_ELEV") == 1 and dm.store.norm["DEM_ELEV"].shape == (2, 1)
    train = list(dm.train_dataloader())
    assert len(train) == 2 and all(set(b) == {"INDEX", f"ID_{TASK}"} for b in train)
    assert all(b["INDEX"].dtype == torch.int32 and b["INDEX"].shape == (2,) for b in train)
    assert sorted(torch.cat([b["INDEX"] for b in train]).tolist()) == [0, 1, 2, 3]
    val = list(dm.val_dataloader())
    assert torch.cat([b["INDEX"] for b in val]).tolist() == [4, 5, 6, 7]  # ascending, behind the training share
    for b in train + val:
        assert [os.path.basename(p) for p in b[f"ID_{TASK}"]] == [meta["files"][TASK][int(i) % 4] for i in b["INDEX"]]
    from flair_hub.tasks.module_setup import get_input_img_sizes
    assert get_input_img_sizes(dm.config, dm, "fit") == {"AERIAL_RGBI": 64, "DEM_ELEV": 16}
    assert get_input_img_sizes(dm.config, dm, "predict") == {"AERIAL_RGBI": 64, "DEM_ELEV": 16}


@pytest.mark.parametrize("rank", [0, 1])
def test_each_rank_stores_its_fixed_share_before_a_process_group_exists(gold, on_disk, monkeypatch, rank):
    """the entry point sets the data module up before the trainer creates the process group: rank and world then come
    from the launcher's RANK / WORLD_SIZE.  A world of 2: the store holds the share rank::2 of each split and nothing
    else, the budget is applied to that share, and the loaders stay inside it."""
    monkeypatch.setenv("RANK", str(rank))
    monkeypatch.setenv("WORLD_SIZE", "2")
    meta, z = gold
    per_patch = 5 * 64 * 64 + 2 * 16 * 16 * 4 + 64 * 64
    _, dm = _data_module(meta, on_disk, cache="device", cache_bytes=4 * per_patch, device="cpu")  # half of 8 patches
    dm.setup("fit")
    assert dm.store is not None and dm.store.n == 4 and dm.store.bytes == 4 * per_patch
    own = [rank, rank + 2]  # of the 4 patches of a split
    names = [meta["files"][TASK][i] for i in own]
    assert [os.path.basename(p) for p in dm.store.ids[TASK]] == names + names  # train share, then validation share
    for slot, i in enumerate(own + own):
        assert np.array_equal(dm.store.inputs["AERIAL_RGBI"][slot].numpy(), z["in/" + meta["files"]["AERIAL_RGBI"][i]])
    for epoch in (0, 1):
        loader = dm.train_dataloader()
        loader.set_epoch(epoch)
        batches = list(loader)
        assert len(batches) == 1 and sorted(batches[0]["INDEX"].tolist()) == [0, 1]
    assert dm.train_dataloader().rank == rank
    assert [b["INDEX"].tolist() for b in dm.val_dataloader()] == [[2, 3]]
    dm.setup("fit")  # the trainer's own setup: the store is not rebuilt
    assert dm.store.n == 4
    # the streamed raw loaders shard by the same rule
    _, raw = _data_module(meta, on_disk, cache="none", device_prepare=True)
    raw.setup("fit")
    ids = [os.path.basename(p) for b in raw.val_dataloader() for p in b[f"ID_{TASK}"]]
    assert ids == names
    raw.teardown()
    monkeypatch.setenv("RANK", "2")
    with pytest.raises(RuntimeError):
        _data_module(meta, on_disk, cache="device", cache_bytes=1 << 30, device="cpu")[1].setup("fit")


def test_streamed_raw_dem_without_norm_vectors_still_takes_the_kernel_route(gold, on_disk):
    """norm_type 'without' (and 'scaling' of the float32 DEM) have no mean / std, but the raw 2-band DEM of calc_elevation
    is differenced by the layout kernel, which the model chooses by DEM_ELEV_NORM: the collate supplies the identity"""
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    meta, _ = gold
    for norm_type, aerial in (("without", None), ("scaling", [[0.0] * 5, [255.0] * 5])):
        cfg = config_of(meta, "dem_elev", on_disk)
        cfg["modalities"]["normalization"] = {"norm_type": norm_type}
        train, val, test = get_datasets(cfg)
        dm = FlairDataModule(cfg, train, val, test, num_workers=2, batch_size=2, cache="none", device_prepare=True,
                             use_augmentations=False)
        dm.setup("fit")
        first = dm.train_dataloader()
        assert dm.train_dataloader().ahead is first.ahead is not None  # one pool per module, shared by its loaders
        batch = next(iter(first))
        assert batch["DEM_ELEV"].shape == (2, 2, 16, 16) and batch["DEM_ELEV_NORM"].tolist() == [[0.0], [1.0]]
        if aerial is None:
            assert "AERIAL_RGBI_NORM" not in batch
        else:
            assert batch["AERIAL_RGBI_NORM"].tolist() == aerial
        assert len(list(dm.val_dataloader())) == 2  # decode-ahead hands over every batch, in order
        dm.teardown()
        assert dm._pool is None


def test_time_series_never_enter_the_store(gold, on_disk, caplog):
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    from flairhip.sample_store import SampleStore
    meta, _ = gold
    cfg = config_of(meta, "s2", on_disk)
    train, val, test = get_datasets(cfg)
    dm = FlairDataModule(cfg, train, val, test, num_workers=0, batch_size=2, cache="device", cache_bytes=1 << 30,
                         device="cpu", use_augmentations=False)
    with caplog.at_level("INFO", logger="flair_hub.data.datamodule"):
        dm.setup("fit")
    assert dm.store is None and "time series" in caplog.text
    with pytest.raises(ValueError):
        SampleStore(2, {"SENTINEL2_TS": ((3, 10, 10), np.uint16)}, {}, {}, device="cpu")
    with pytest.raises(ValueError):
        FlairDataModule(cfg, train, val, test, cache="host")


def test_build_data_module_reads_the_optional_config_keys(gold, on_disk):
    from flair_hub.tasks.module_setup import build_data_module
    meta, _ = gold
    cfg = config_of(meta, "dem_elev", on_disk)
    cfg["hardware"] = {"num_workers": 0}
    dm = build_data_module(cfg)
    assert dm.cache == "none" and dm.cache_bytes is None and dm.device_prepare is False and dm.batch_size == 2
    cfg["hardware"].update(sample_cache="device", sample_cache_bytes=12345)
    dm = build_data_module(cfg)
    assert dm.cache == "device" and dm.cache_bytes == 12345 and dm.device_prepare is True


def test_read_config_merges_a_directory_by_top_level_key(tmp_path):
    import argparse
    from flair_hub.utils.config_io import read_config, setup_environment
    (tmp_path / "a.yaml").write_text("paths:\n  out_folder: %s\n  out_model_name: run1\n" % (tmp_path / "out"))
    (tmp_path / "b.yaml").write_text("tasks:\n  train: true\nhardware:\n  sample_cache: device\n")
    (tmp_path / "notes.txt").write_text("ignored")
    cfg = read_config(str(tmp_path))
    assert set(cfg) == {"paths", "tasks", "hardware"} and cfg["hardware"]["sample_cache"] == "device"
    assert read_config(str(tmp_path / "b.yaml")) == {"tasks": {"train": True}, "hardware": {"sample_cache": "device"}}
    with pytest.raises(ValueError):
        read_config(str(tmp_path / "notes.txt"))
    cfg, out_dir = setup_environment(argparse.Namespace(config=str(tmp_path)))
    assert out_dir == tmp_path / "out" / "run1" and out_dir.is_dir()
