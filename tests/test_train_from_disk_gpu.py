"""Training from a FLAIR-HUB dataset on disk: an 8-patch dataset written here (64 x 64 aerial uint8 + a 2-band float32
DEM with calc_elevation, labels with values >= K), FlairDataModule with the device-resident sample store and with the
streamed raw loaders, eagerly and as a captured step.  Both paths run the same kernels on the same samples, so their
loss trajectories and weights are compared bit for bit.

The DEM patches are 32 x 32, not the 16 x 16 of the CPU golden: the ResNet-34 encoder refuses planes whose sides are
not multiples of 32 (FLAIR_HUB_Model._input_nhwc), with or without this feature."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

from helpers import TASK

pytestmark = pytest.mark.gpu
MOD, DEM, K = "AERIAL_RGBI", "DEM_ELEV", 19
STEM = f"encoders.{DEM}.seg_model.conv1.weight"


def write_tif(path, arr):
    from flair_zonal_detection.geotiff import GeoTiffWriter
    w = GeoTiffWriter(str(path), arr.shape[2], arr.shape[1], arr.shape[0], 800000.0, 6500000.0, 0.2, crs="EPSG:2154",
                      dtype=arr.dtype)
    w.data[:] = arr
    w.close()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("patches")
    r = np.random.RandomState(5)
    rows = []
    for i in range(8):
        area = f"D0{i:02d}-2021_UU-S2-{i}_{i}-{i + 1}"
        dom, rest = area.split("_", 1)
        files = {MOD: f"{area}_{MOD}.tif", DEM: f"{area}_{DEM}.tif", TASK: f"{dom}_{TASK}_{rest}.tif"}
        write_tif(root / files[MOD], r.randint(1, 256, (5, 64, 64)).astype(np.uint8))
        z = r.randn(32, 32) * 40 + 350
        write_tif(root / files[DEM], np.stack([z + np.abs(r.randn(32, 32)) * 12, z]).astype(np.float32))
        lab = r.randint(0, 22, (1, 64, 64)).astype(np.uint8)
        lab[0, 0, :2] = [K, 255]
        write_tif(root / files[TASK], lab)
        rows.append({k: str(root / v) for k, v in files.items()})
    for split in ("train", "val", "test"):
        with open(root / f"{split}.csv", "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=[MOD, DEM, TASK])
            w.writeheader()
            w.writerows(rows if split == "train" else rows[:4])
    return root


def make_config(root, out, hip_graph=False):
    from flairhip.configs import unet_resnet34_config
    cfg = unet_resnet34_config(in_channels=5, precision="fp32", batch_size=4)
    mods = cfg["modalities"]
    mods["inputs"][DEM] = True
    mods["pre_processings"].update(calc_elevation=True, calc_elevation_stack_dsm=False, use_augmentation=True)
    mods["normalization"] = {"norm_type": "custom", f"{MOD}_means": [105.08, 110.87, 101.82, 106.38, 53.26],
                             f"{MOD}_stds": [52.17, 45.38, 44.0, 39.69, 79.3], f"{DEM}_means": [9.5], f"{DEM}_stds": [7.25]}
    cfg["hyperparams"].update(num_epochs=3, scheduler=None, seed=11)
    cfg["hardware"]["hip_graph"] = hip_graph
    cfg["paths"] = {"train_csv": str(root / "train.csv"), "val_csv": str(root / "val.csv"),
                    "test_csv": str(root / "test.csv"), "out_folder": str(out), "out_model_name": "run"}
    cfg["tasks"] = {"train": True, "predict": True, "write_files": True, "georeferencing_output": False}
    return cfg


class LastEpochReversed:
    """a training loader whose batches come in reverse order in one epoch, and as the inner loader gives them otherwise"""
    rank_sharded = True

    def __init__(self, inner, epoch):
        self.inner, self.reversed_epoch, self.epoch = inner, epoch, 0

    def set_epoch(self, epoch):
        self.epoch = epoch
        self.inner.set_epoch(epoch)

    def __len__(self):
        return len(self.inner)

    def __iter__(self):
        batches = list(self.inner)
        return iter(batches[::-1] if self.epoch == self.reversed_epoch else batches)


def run(root, out, cache, hip_graph, seed=None, reverse_epoch=None):
    """6 training steps (3 epochs of 2 batches of 4) -> (losses, the DEM stem's weights, trainer, data module, config)"""
    from flair_hub.data.datamodule import FlairDataModule
    from flair_hub.data.utils_data.paths import get_datasets
    from flair_hub.tasks.module_setup import build_segmentation_module, get_input_img_sizes
    from flair_hub.tasks.trainers import train
    cfg = make_config(root, out, hip_graph)
    tr, va, te = get_datasets(cfg)
    dm = FlairDataModule(cfg, tr, va, te, num_workers=0, batch_size=4, drop_last=True, use_augmentations=True,
                         cache=cache, device_prepare=True, seed=seed)
    sizes = get_input_img_sizes(cfg, dm, "fit")
    assert sizes == {MOD: 64, DEM: 32}
    if reverse_epoch is not None:
        make = dm.train_dataloader
        dm.train_dataloader = lambda: LastEpochReversed(make(), reverse_epoch)
    assert (dm.store is not None) == (cache == "device")
    torch.manual_seed(3)
    task = build_segmentation_module(cfg, sizes, "train")
    losses, orig = [], task.on_train_batch_end
    task.on_train_batch_end = lambda loss, batch, i: (losses.append(float(loss.detach())), orig(loss, batch, i))[1]
    trainer = train(cfg, dm, task, str(out / f"ckpt_{cache}_{int(hip_graph)}"))
    weights = dict(task.model.named_parameters())[STEM].detach().cpu().clone()
    return losses, weights, trainer, dm, cfg, task


@pytest.fixture(scope="module")
def runs(cuda, dataset, tmp_path_factory):
    out = tmp_path_factory.mktemp("out")
    got = {(cache, graph): run(dataset, out, cache, graph) for cache in ("device", "none") for graph in (False, True)}
    for (cache, graph), r in got.items():
        # a hip_graph run really replays: two ordinary steps, the capture, four replays (the tests below that speak of
        # a replayed step would otherwise compare eager runs)
        did = (r[2].graph_built, r[2].graph_replays, r[2].eager_steps)
        assert did == ((True, 4, 2) if graph else (False, 0, 6)), (cache, graph, did)
    return got, out


def test_resident_and_streamed_training_are_bit_identical(runs):
    got, _ = runs
    for graph in (False, True):
        dev, none = got[("device", graph)], got[("none", graph)]
        print(f"hip_graph={graph}: resident {dev[0]}\n{'':16s}streamed {none[0]}")
        assert len(dev[0]) == 6 and all(np.isfinite(dev[0]))
        assert dev[0] == none[0], "loss trajectories differ between the resident and the streamed path"
        assert torch.equal(dev[1], none[1]), "the DEM stem's weights differ"
    assert got[("device", False)][0][:2] == got[("device", True)][0][:2]  # the two ordinary steps before the capture


def test_validation_logs_val_miou_from_the_store(runs):
    got, _ = runs
    for key, (_l, _w, trainer, dm, _c, _t) in got.items():
        assert "val_miou" in trainer.callback_metrics and 0.0 <= trainer.callback_metrics["val_miou"] <= 1.0, key
        assert trainer.best_model_path and os.path.isfile(trainer.best_model_path)
    assert got[("device", True)][2].callback_metrics["val_miou"] == got[("none", True)][2].callback_metrics["val_miou"]


def test_a_replayed_step_follows_new_indices(cuda, dataset, runs, tmp_path):
    """Steps 0 and 1 run eagerly, the step is captured at step 2 and replayed from there on.  The same run with the two
    batches of the last epoch (steps 4 and 5) exchanged: same weights, codes and batches up to step 3, so the losses
    agree exactly up to there; step 4 is a replay that differs from the base run in nothing but the values of INDEX.  A
    replay that ignored its indices would repeat the base run's loss."""
    got, _ = runs
    base = got[("device", True)]
    moved = run(dataset, tmp_path, "device", True, reverse_epoch=2)
    print(f"base  {base[0]}\nmoved {moved[0]}")
    assert len(moved[0]) == 6 and moved[0][:4] == base[0][:4]
    assert moved[0][4] != base[0][4]
    loader = base[3].train_dataloader()
    loader.set_epoch(2)
    first, second = [b["INDEX"].tolist() for b in loader]
    assert sorted(first) != sorted(second)  # the two batches hold different patches


def test_the_trajectory_moves_with_the_permutation_seed(cuda, dataset, runs, tmp_path):
    got, _ = runs
    base = got[("device", True)]
    moved = run(dataset, tmp_path, "device", True, seed=12)
    order = lambda dm: [b["INDEX"].tolist() for b in dm.train_dataloader()]
    assert order(moved[3]) != order(base[3])
    assert moved[0] != base[0] and not torch.equal(moved[1], base[1])


def test_predict_stage_writes_rasters_and_metrics(runs, dataset):
    from flair_hub.tasks.stages import predict_stage
    got, out = runs
    _l, _w, trainer, dm, cfg, task = got[("device", False)]
    state = torch.load(trainer.best_model_path, map_location="cpu")["state_dict"]
    pred_dir = out / "results_run"
    predict_stage(cfg, dm, pred_dir, state)
    rasters = sorted(glob.glob(str(pred_dir / "**" / "PRED_*"), recursive=True))
    with open(dataset / "test.csv") as f:
        labels = [os.path.basename(r[TASK]) for r in csv.DictReader(f)]
    assert [os.path.basename(p) for p in rasters] == sorted("PRED_" + n for n in labels)
    assert glob.glob(str(pred_dir / "**" / "metrics.json"), recursive=True)
    assert get_sizes(cfg, dm) == {MOD: 64, DEM: 32}


def get_sizes(cfg, dm):
    from flair_hub.tasks.module_setup import get_input_img_sizes
    return get_input_img_sizes(cfg, dm, "predict")


def test_a_two_band_dem_without_calc_elevation_is_still_refused(runs, cuda):
    got, _ = runs
    task = got[("none", False)][5]
    x = torch.rand(2, 5, 64, 64, device=cuda)
    dem = torch.rand(2, 2, 32, 32, device=cuda)
    norm = torch.tensor([[9.5], [7.25]], device=cuda)
    task.eval()
    with torch.no_grad():
        with pytest.raises(ValueError):  # no <MOD>_NORM: not the raw route
            task.model({MOD: x, DEM: dem})
        task.model({MOD: x, DEM: dem, DEM + "_NORM": norm})  # the raw route: calc_elevation in the layout pass
        pp = task.model.config["modalities"]["pre_processings"]
        pp["calc_elevation"] = False
        try:
            with pytest.raises(ValueError):
                task.model({MOD: x, DEM: dem, DEM + "_NORM": norm})
        finally:
            pp["calc_elevation"] = True
