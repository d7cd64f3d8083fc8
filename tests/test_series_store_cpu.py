"""Sentinel time series in the device sample store, without a GPU (stores on device="cpu"): the C ABI of
include/flairhip_series.h against flairhip.lib.SERIES_SIGNATURES, the ragged SeriesStore built by the data module from
the golden dataset (tests/golden/train_batch.*, setting s2: lengths 3, 5, 2, 4, channels [2, 3, 8]) with and without
cloud filtering and monthly averaging, the numpy definition of the gathered batch, the budget and fall-back rules, the
batch keys of the index loader and the host-side validation of ops.gather_series."""
import json
import os
import re
import shutil

import numpy as np
import pytest
import torch

import test_abi_cpu as abi
from helpers import ROOT
from test_data_module_cpu import TASK, config_of, gold, on_disk, write_tif  # noqa: F401  (gold, on_disk: fixtures)
from flairhip import lib as L

SERIES_HEADER = os.path.join(ROOT, "include", "flairhip_series.h")
LENGTHS = [3, 5, 2, 4]
FILTER = {"filter_sentinel2": True, "filter_sentinel2_max_cloud": 50, "filter_sentinel2_max_snow": 50,
          "filter_sentinel2_max_frac_cover": 0.72}


# ---- 1. ABI ------------------------------------------------------------------------------------------------------------


def series_header_text():
    text = re.sub(r"/\*.*?\*/", " ", open(SERIES_HEADER).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def series_header_signatures(monkeypatch):
    monkeypatch.setattr(abi, "header_text", series_header_text)
    return abi.header_signatures()


def test_series_table_equals_the_series_header(monkeypatch):
    header = series_header_signatures(monkeypatch)
    assert len(header) == len(re.findall(r"\bffa_\w+\s*\(", series_header_text())), "the parser missed a prototype"
    assert sorted(header) == ["ffa_gather_series"]
    assert abi.mismatches(header, L.SERIES_SIGNATURES) == []
    assert not set(L.SERIES_SIGNATURES) & (set(L.SIGNATURES) | set(L.EVAL_SIGNATURES) | set(L.GATHER_SIGNATURES))


def test_a_planted_series_mismatch_is_reported(monkeypatch):
    header = series_header_signatures(monkeypatch)
    ret, args = L.SERIES_SIGNATURES["ffa_gather_series"]
    i = 15  # float fill
    assert args[i] is abi.C.c_float
    wrong = {"ffa_gather_series": (ret, args[:i] + [abi.C.c_int] + args[i + 1:])}
    assert abi.mismatches(header, wrong) == ["ffa_gather_series: argument 15 is c_float, table says c_int"]
    assert abi.mismatches(header, {}) == ["ffa_gather_series: declared in include/flairhip.h, no ctypes signature"]


def test_the_main_header_includes_the_series_header_after_the_gather_header():
    main = open(os.path.join(ROOT, "include", "flairhip.h")).read()
    assert re.search(r'^#include "flairhip_series\.h"$', main, flags=re.M)
    at = main.index('#include "flairhip_series.h"')
    assert main.index('extern "C" {') < main.index('#include "flairhip_gather.h"') < at < main.rindex("#ifdef __cplusplus")


# ---- 2. the store built from the golden dataset ----------------------------------------------------------------------------


def s2_module(meta, root, pre=None, **kw):
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    cfg = config_of(meta, "s2", root)
    cfg["modalities"]["pre_processings"].update(pre or {})
    train, val, test = get_datasets(cfg)
    kw.setdefault("cache_bytes", 1 << 30)
    kw.setdefault("batch_size", 4)
    return cfg, (train, val, test), FlairDataModule(cfg, train, val, test, num_workers=0, drop_last=True,
                                                    use_augmentations=False, cache="device", device="cpu", **kw)


@pytest.fixture(scope="module")
def resident(gold, on_disk):
    meta, _ = gold
    _cfg, _paths, dm = s2_module(meta, on_disk, series_cache=True)
    dm.setup("fit")
    return dm


def test_the_series_store_holds_what_the_dataset_yields(gold, resident):
    from flairhip.sample_store import SampleStore, SeriesStore
    meta, z = gold
    assert isinstance(resident.store, SampleStore) and list(resident.store.series) == ["SENTINEL2_TS"]
    st = resident.store.series["SENTINEL2_TS"]
    assert isinstance(st, SeriesStore) and st.n == 8 and st.filled == 8  # train share, then the validation share
    assert st.offsets_host.tolist() == [0, 3, 8, 10, 14, 17, 22, 24, 28] and st.offsets_host.dtype == np.int32
    assert st.offsets.dtype == torch.int32 and st.offsets.tolist() == st.offsets_host.tolist()
    assert st.offsets_host[:5].tolist() == [0, 3, 8, 10, 14] and st.lengths.tolist() == LENGTHS * 2
    assert st.data.dtype == torch.uint16 and tuple(st.data.shape) == (28, 3, 10, 10) and st.data.is_contiguous()
    assert st.is_pad.dtype == torch.uint8 and tuple(st.is_pad.shape) == (28,) and not st.is_pad.any()
    assert st.dates.dtype == np.float32 and st.dates.shape == (28,)
    off = st.offsets_host
    for slot in range(8):
        i = slot % 4
        got = st.data[off[slot]:off[slot + 1]].numpy().astype(np.float32)
        assert np.array_equal(got, z[f"s2/{i}/SENTINEL2_TS"])
        assert np.array_equal(st.dates[off[slot]:off[slot + 1]], z[f"s2/{i}/SENTINEL2_DATES"])
    assert resident.input_img_sizes() == {"AERIAL_RGBI": 64, "SENTINEL2_TS": 10}
    assert resident.store.inputs.keys() == {"AERIAL_RGBI"}  # inputs= still holds no time series


def test_the_batch_reference_reproduces_the_reference_collate(gold, resident):
    from flairhip.sample_store import series_batch_reference
    _, z = gold
    st = resident.store.series["SENTINEL2_TS"]
    out, pad = series_batch_reference(st, [0, 1, 2, 3])
    want = z["s2/collate/SENTINEL2_TS"]  # [4, 5, 3, 10, 10]
    assert out.dtype == np.float32 and out.shape == (20, 10, 10, 16) and pad.dtype == np.uint8
    assert np.array_equal(out[..., :3], want.reshape(20, 3, 10, 10).transpose(0, 2, 3, 1)) and not out[..., 3:].any()
    lengths = np.array(LENGTHS)
    assert np.array_equal(pad.reshape(4, 5), (np.arange(5)[None] >= lengths[:, None]).astype(np.uint8))
    # pad_value -1: a padded date holds the 0 it was padded with and is not flagged, as on the streamed path
    assert not series_batch_reference(st, [0, 1, 2, 3], pad_value=-1.0)[1].any()
    out7, pad7 = series_batch_reference(st, torch.tensor([2, 2, 0], dtype=torch.int32), T=7, cp=8)
    assert out7.shape == (21, 10, 10, 8) and pad7.reshape(3, 7).sum(1).tolist() == [5, 5, 4]
    assert np.array_equal(out7[:7], out7[7:14]) and np.array_equal(out7[14:17], out[0:3, ..., :8])
    with pytest.raises(ValueError):
        series_batch_reference(st, [1], T=4)
    with pytest.raises(ValueError):
        series_batch_reference(st, [8])


def test_the_batch_reference_with_codes_is_the_augmentation_then_the_collate(gold, resident):
    from flair_hub.data.utils_data.padding import pad_collate_flair
    from flairhip.augment import apply_code
    from flairhip.sample_store import series_batch_reference
    _, z = gold
    st = resident.store.series["SENTINEL2_TS"]
    for codes in ([0, 1, 2, 3], [4, 7, 9, 14], [12, 5, 10, 15]):
        out, _ = series_batch_reference(st, [0, 1, 2, 3], codes=np.array(codes, dtype=np.uint8))
        samples = [{"SENTINEL2_TS": torch.from_numpy(apply_code(z[f"s2/{i}/SENTINEL2_TS"], c))}
                   for i, c in enumerate(codes)]
        want = pad_collate_flair(samples)["SENTINEL2_TS"].numpy()
        assert np.array_equal(out[..., :3], want.reshape(20, 3, 10, 10).transpose(0, 2, 3, 1)), codes


def test_the_index_loader_carries_the_dates_and_no_image(gold, resident):
    _, z = gold
    val = list(resident.val_dataloader())
    assert len(val) == 1 and set(val[0]) == {"INDEX", f"ID_{TASK}", "SENTINEL2_DATES"}
    assert val[0]["INDEX"].tolist() == [4, 5, 6, 7] and val[0]["SENTINEL2_DATES"].dtype == torch.float32
    assert np.array_equal(val[0]["SENTINEL2_DATES"].numpy(), z["s2/collate/SENTINEL2_DATES"])
    for b in resident.train_dataloader():
        assert set(b) == {"INDEX", f"ID_{TASK}", "SENTINEL2_DATES"}
        assert not any(torch.is_tensor(v) and v.ndim > 2 for v in b.values())
        order = [int(i) for i in b["INDEX"]]
        assert np.array_equal(b["SENTINEL2_DATES"].numpy(), z["s2/collate/SENTINEL2_DATES"][order])
    st = resident.store.series["SENTINEL2_TS"]
    two = st.dates_of(torch.tensor([2, 0], dtype=torch.int32))  # T is the longest series of the batch
    assert tuple(two.shape) == (2, 3) and two[0, 2] == 0 and np.array_equal(two[1].numpy(), z["s2/0/SENTINEL2_DATES"])


def test_the_augmented_loader_counts_the_codes_by_index(resident):
    from flair_hub.tasks.trainers import AugmentedLoader
    batch = next(iter(AugmentedLoader(resident.val_dataloader(), resident.config, seed=3)))  # [B, T] dates ride along
    assert batch["AUG"].dtype == torch.uint8 and tuple(batch["AUG"].shape) == (4,)


# ---- 3. filtering and averaging happen once, at fill time -----------------------------------------------------------------


def reference_samples(cfg, paths):
    from flair_hub.data.dataloader import flair_dataset
    ds = flair_dataset(cfg, paths[0], use_augmentations=None, device_prepare=False)
    return [ds[i] for i in range(len(ds))]


def test_filtered_series_equal_the_reference_schema(gold, on_disk):
    from flair_hub.data.utils_data.sentinel import filter_time_series, reshape_sentinel
    meta, z = gold
    kept = [int(filter_time_series(reshape_sentinel(z["in/" + name], 2), 50, 50, 0.72).sum())
            for name in meta["files"]["SENTINEL2_MSK-SC"]]
    assert all(k >= 1 for k in kept) and any(k < n for k, n in zip(kept, LENGTHS)), kept  # what the thresholds are for
    cfg, paths, dm = s2_module(meta, on_disk, FILTER, series_cache=True)
    dm.setup("fit")
    st = dm.store.series["SENTINEL2_TS"]
    assert st.lengths.tolist() == kept * 2 and st.data.dtype == torch.uint16
    off = st.offsets_host
    for i, s in enumerate(reference_samples(cfg, paths)):
        assert s["SENTINEL2_TS"].shape[0] == kept[i]
        assert np.array_equal(st.data[off[i]:off[i + 1]].numpy().astype(np.float32), s["SENTINEL2_TS"].numpy())
        assert np.array_equal(st.dates[off[i]:off[i + 1]], s["SENTINEL2_DATES"].numpy())


def test_averaged_series_are_float32_with_twelve_dates(gold, on_disk):
    meta, _ = gold
    cfg, paths, dm = s2_module(meta, on_disk, {"temporal_average_sentinel2": "monthly"}, series_cache=True)
    dm.setup("fit")
    st = dm.store.series["SENTINEL2_TS"]
    assert st.data.dtype == torch.float32 and st.lengths.tolist() == [12] * 8
    off = st.offsets_host
    ref = reference_samples(cfg, paths)
    for i, s in enumerate(ref):
        assert s["SENTINEL2_TS"].dtype == torch.float32 and s["SENTINEL2_TS"].shape[0] == 12
        assert np.array_equal(st.data[off[i]:off[i + 1]].numpy(), s["SENTINEL2_TS"].numpy())
        assert np.array_equal(st.dates[off[i]:off[i + 1]], s["SENTINEL2_DATES"].numpy())
    # months before a sample's first acquisition are all zero = constant at the pad value: flagged, like on the streamed path
    flags = st.is_pad.numpy()
    want = np.array([int(not s["SENTINEL2_TS"][t].any()) for s in ref for t in range(12)], dtype=np.uint8)
    assert np.array_equal(flags[:48], want) and flags.any() and not flags.all()
    assert all(tuple(b["SENTINEL2_DATES"].shape) == (4, 12) for b in dm.val_dataloader())  # one T: the step replays


# ---- 4. budget and fall-back ------------------------------------------------------------------------------------------------


def test_the_budget_counts_the_series(gold, on_disk, caplog):
    from flairhip.sample_store import store_bytes
    meta, _ = gold
    fixed = 8 * (5 * 64 * 64 + 64 * 64)                       # aerial uint8 + labels
    series = 28 * 3 * 10 * 10 * 2 + 4 * (8 + 1) + 28          # uint16 data + int32 offsets + uint8 pad flags
    assert store_bytes(8, {"AERIAL_RGBI": ((5, 64, 64), np.uint8)}, {TASK: (64, 64)},
                       {"SENTINEL2_TS": (28, (3, 10, 10), np.uint16)}) == fixed + series
    _, _, dm = s2_module(meta, on_disk, series_cache=True, cache_bytes=fixed + series)
    dm.setup("fit")
    assert dm.store is not None and dm.store.bytes == fixed + series
    assert dm.store.fits(fixed + series) and not dm.store.fits(fixed + series - 1)
    _, _, dm = s2_module(meta, on_disk, series_cache=True, cache_bytes=fixed + series - 1)
    with caplog.at_level("INFO", logger="flair_hub.data.datamodule"):
        dm.setup("fit")
    assert dm.store is None and "falling back to the streamed loaders (a split is never stored in part)" in caplog.text
    batch = next(iter(dm.train_dataloader()))
    assert "INDEX" not in batch and batch["SENTINEL2_TS"].dtype == torch.float32 and batch["SENTINEL2_TS"].ndim == 5
    dm.teardown()


def test_the_switch_is_off_by_default(gold, on_disk, caplog):
    from flair_hub.tasks.module_setup import build_data_module
    meta, _ = gold
    _, _, dm = s2_module(meta, on_disk)
    assert dm.series_cache is False
    with caplog.at_level("INFO", logger="flair_hub.data.datamodule"):
        dm.setup("fit")
    assert dm.store is None and "time series" in caplog.text
    cfg = config_of(meta, "s2", on_disk)
    cfg["hardware"] = {"num_workers": 0, "sample_cache": "device"}
    assert build_data_module(cfg).series_cache is False
    cfg["hardware"]["sample_cache_series"] = True
    assert build_data_module(cfg).series_cache is True


def test_a_sample_emptied_by_the_filter_keeps_the_split_streamed(gold, on_disk, tmp_path, caplog):
    meta, z = gold
    for name in os.listdir(on_disk):
        shutil.copy(on_disk / name, tmp_path / name)
    (tmp_path / "split.csv").write_text((on_disk / "split.csv").read_text().replace(str(on_disk), str(tmp_path)))
    victim = meta["files"]["SENTINEL2_MSK-SC"][2]
    write_tif(tmp_path / victim, np.full_like(z["in/" + victim], 99))  # snow and cloud everywhere, at every date
    _, _, dm = s2_module(meta, tmp_path, FILTER, series_cache=True)
    with caplog.at_level("INFO", logger="flair_hub.data.datamodule"):
        dm.setup("fit")
    assert dm.store is None and "empty after filtering" in caplog.text and "falling back" in caplog.text
    assert meta["files"][TASK][2] in caplog.text  # the log names the patch
    assert dm.train_dataset.keep_series_raw is False and dm.train_dataset.keep_dem_bands is False


def test_series_store_refuses_what_does_not_fit():
    from flairhip.sample_store import SampleStore, SeriesStore, series_dtype
    assert series_dtype(np.uint16, False) == np.uint16 and series_dtype(np.uint16, True) == np.float32
    assert series_dtype(np.int32, False) == np.float32 and series_dtype(np.float64, False) == np.float32
    st = SeriesStore(2, 3, (1, 2, 2), np.int16, pad_value=-1, device="cpu")
    a = np.arange(8, dtype=np.int16).reshape(2, 1, 2, 2)
    with pytest.raises(ValueError):
        st.fill(1, a, [0, 1])                      # samples come in order
    with pytest.raises(ValueError):
        st.fill(0, a.astype(np.uint16), [0, 1])    # the sample type is the store's
    with pytest.raises(ValueError):
        st.fill(0, a[:0], [])                      # an empty series
    st.fill(0, a, [5, 6])
    assert st.offsets is None                      # not complete yet
    st.fill(1, np.full((1, 1, 2, 2), -1, dtype=np.int16), [9])
    assert st.offsets.tolist() == [0, 2, 3] and st.is_pad.tolist() == [0, 0, 1] and st.dates.tolist() == [5, 6, 9]
    with pytest.raises(ValueError):
        SeriesStore(2, 1, (1, 2, 2), np.int16, device="cpu")   # fewer dates than samples
    with pytest.raises(ValueError):
        SeriesStore(2, 3, (1, 2, 2), np.float64, device="cpu")
    with pytest.raises(ValueError):
        SampleStore(3, {}, {}, {}, device="cpu", series={"SENTINEL2_TS": st})  # another sample count
    assert SampleStore(2, {}, {}, {}, device="cpu").series == {}
    both = SampleStore(2, {}, {}, {}, device="cpu", series={"SENTINEL2_TS": st})
    assert both.bytes == 3 * 4 * 2 + 4 * 3 + 3 and both.img_sizes() == {"SENTINEL2_TS": 2}


# ---- 5. ops.gather_series validates on the host ------------------------------------------------------------------------


def test_gather_series_validates_before_any_launch(resident, monkeypatch):
    from flairhip import ops
    from flairhip.sample_store import SeriesStore
    monkeypatch.setattr(L, "load", lambda: pytest.fail("gather_series reached the library"))
    st = resident.store.series["SENTINEL2_TS"]

    def idx(*v):
        return torch.tensor(v, dtype=torch.int32)

    with pytest.raises(ValueError, match="outside the store"):
        ops.gather_series(st, idx(0, 8), 5, torch.float32)
    with pytest.raises(ValueError, match="outside the store"):
        ops.gather_series(st, idx(-1), 5, torch.float32)
    with pytest.raises(ValueError, match="longest indexed series has 5 dates, T = 4"):
        ops.gather_series(st, idx(0, 1), 4, torch.float32)
    with pytest.raises(ValueError, match="int32"):
        ops.gather_series(st, torch.tensor([0]), 5, torch.float32)
    with pytest.raises(ValueError, match="channel pitch"):
        ops.gather_series(st, idx(0), 5, torch.float32, cp=12)
    wide = SeriesStore(1, 1, (1, 6, 10), np.uint8, device="cpu")
    wide.fill(0, np.zeros((1, 1, 6, 10), dtype=np.uint8), [0])
    with pytest.raises(ValueError, match="square planes"):
        ops.gather_series(wide, idx(0), 1, torch.float32, codes=torch.zeros(1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="on the host"):   # valid arguments, but a host store: still no launch
        ops.gather_series(st, idx(0, 1), 5, torch.float32)
