"""The evaluation stage on a resnet34-unet at 64 x 64 with seeded weights.

Validation (flair_hub/tasks/tasks_module.py): HipTrainer.validate over three host batches of 2, 2 and 1 samples logs
every val_loss_class_* and val_iou_* key of the reference.  Each per-class loss is held against F.cross_entropy in
float64 on the step's own logits -- the batch-size-weighted mean of the batches' class means, 0 where a batch has no
pixel of the class -- within REL * sum (|lse| + |z_t|) / count (tests/insitu.py), carried through the same mean; the
per-class IoU equals that of a bincount confusion matrix exactly; val_loss and val_miou keep their bits.

Test stage (flair_hub/writer, trainers.predict): label GeoTIFFs in tmp_path, two tasks, the second with its labels in
band 2, values >= K present; batches of 2, so sample 1 of a batch is covered.
"""
import csv
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import MOD, TASK, make_pair
from insitu import REL

pytestmark = pytest.mark.gpu

F64 = torch.float64
LPIS, DEM = "ALL_LABEL-LPIS", "DEM_ELEV"


# ---- validation --------------------------------------------------------------------------------------------------------

def _val_batches():
    g = torch.Generator().manual_seed(11)
    out = []
    for B, hi in ((2, 19), (2, 19), (1, 10)):  # the last batch has no pixel of classes 10..18
        out.append({MOD: torch.randn(B, 5, 64, 64, generator=g), TASK: torch.randint(0, hi, (B, 64, 64), generator=g)})
    return out


def test_validation_logs_per_class_loss_and_iou(cuda):
    from flair_hub.tasks.trainers import HipTrainer
    task, _, cfg = make_pair(precision="bf16", seed=5)
    names = cfg["labels_configs"][TASK]["value_name"]
    K = len(names)
    trainer = HipTrainer()

    # a run without the per-class logging: the state update of the parent commit, nothing logged per class
    real_update, real_log = task._update_class_stats, task._log_per_class
    task._update_class_stats = lambda key, logits, preds, targets: task.val_iou[key].update(preds, targets)
    task._log_per_class = lambda key: None
    plain = dict(trainer.validate(task, dataloaders=_val_batches())[0])
    assert not [k for k in plain if k.startswith(("val_loss_class_", "val_iou_"))]

    seen = []

    def recording(key, logits, preds, targets):
        seen.append((logits._ffa_nhwc[..., :K].to(F64).clone(), preds.clone(), targets.clone()))
        return real_update(key, logits, preds, targets)

    task._update_class_stats, task._log_per_class = recording, real_log
    task._logged.clear()
    trainer.callback_metrics.clear()
    logged = dict(trainer.validate(task, dataloaders=_val_batches())[0])
    assert len(seen) == 3

    for k in ("val_loss", "val_miou", "val_miou_COSIA"):  # bit for bit
        assert logged[k] == plain[k], k

    total, tol, weight = torch.zeros(K, dtype=F64), torch.zeros(K, dtype=F64), 0
    cm = torch.zeros(K, K, dtype=torch.int64)
    for z, preds, targets in seen:
        z, t = z.cpu(), targets.cpu().long()
        B = z.shape[0]
        nll = F.cross_entropy(z.permute(0, 3, 1, 2), t, reduction="none")
        mag = torch.logsumexp(z, -1).abs() + z.gather(-1, t[..., None])[..., 0].abs()
        for c in range(K):
            m = t == c
            if m.any():
                total[c] += B * nll[m].mean()
                tol[c] += B * REL * mag[m].sum() / m.sum()
        weight += B
        cm += torch.bincount(t.reshape(-1) * K + preds.cpu().long().reshape(-1), minlength=K * K).reshape(K, K)
    assert weight == 5
    want_loss, tol = total / weight, tol / weight
    cmf = cm.float()
    tp = cmf.diag()
    want_iou = torch.nan_to_num(tp / (cmf.sum(0) + cmf.sum(1) - tp), nan=0.0)
    for i in range(K):
        got = logged[f"val_loss_class_COSIA_{i}_{names[i]}"]
        print(f"class {i}: loss {got:.9f} reference {want_loss[i].item():.9f} bound {tol[i].item():.3e}")
        assert abs(got - want_loss[i].item()) <= tol[i].item(), (i, got, want_loss[i].item(), tol[i].item())
        assert logged[f"val_iou_COSIA_{i}_{names[i]}"] == float(want_iou[i]), i
    assert len([k for k in logged if k.startswith("val_loss_class_")]) == K
    assert len([k for k in logged if k.startswith("val_iou_")]) == K
    # the state is reset for the next epoch
    assert not bool(task.val_iou[TASK].confmat.any()) and task.val_class_loss[TASK].count.item() == 0


# ---- test stage --------------------------------------------------------------------------------------------------------

N_SAMPLES, SIZE = 3, 64
ORIGIN, RES, CRS = (650000.0, 6860000.0), 0.2, "EPSG:2154"


def _fusion_task():
    from flairhip.configs import fusion_unet_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from oracle.seeded_weights import fill_state_dict
    cfg = fusion_unet_config(precision="bf16")
    cfg["labels_configs"][LPIS]["label_channel_nomenclature"] = 2
    task = build_segmentation_module(cfg, {MOD: SIZE, DEM: SIZE // 2}, "train")
    task.model.load_state_dict(fill_state_dict(task.model.state_dict()))
    return task.cuda().eval(), cfg


class _DataModule:
    def __init__(self, batches):
        self.batches = batches

    def setup(self, stage):
        assert stage == "predict"

    def predict_dataloader(self):
        return self.batches


def _write_labels(folder):
    """-> ({task: [path per sample]}, {task: [uint8 label band per sample, as the writer must read it]})"""
    from flair_zonal_detection.geotiff import GeoTiffWriter
    rng = np.random.default_rng(3)
    paths, bands = {TASK: [], LPIS: []}, {TASK: [], LPIS: []}
    for j in range(N_SAMPLES):
        left, top = ORIGIN[0] + 12.8 * j, ORIGIN[1] - 12.8 * j
        cosia = rng.integers(0, 19, (SIZE, SIZE)).astype(np.uint8)
        cosia[rng.random((SIZE, SIZE)) < 0.05] = 200                      # a value >= K: counts nowhere
        p = os.path.join(folder, f"COSIA_{j}.tif")
        w = GeoTiffWriter(p, SIZE, SIZE, 1, left, top, RES, crs=CRS)
        w.data[0] = cosia
        w.close()
        paths[TASK].append(p)
        bands[TASK].append(cosia)
        lpis = rng.integers(0, 23, (SIZE, SIZE)).astype(np.uint16)
        lpis[rng.random((SIZE, SIZE)) < 0.05] = 300                       # above 255: read as 255
        lpis[0, :4] = 25                                                  # >= K but a valid byte
        p = os.path.join(folder, f"LPIS_{j}.tif")
        w = GeoTiffWriter(p, SIZE, SIZE, 2, left, top, RES, crs=CRS, dtype=np.uint16)
        w.data[0] = rng.integers(0, 23, (SIZE, SIZE))                     # band 1 is not the nomenclature
        w.data[1] = lpis
        w.close()
        paths[LPIS].append(p)
        bands[LPIS].append(np.minimum(lpis, 255).astype(np.uint8))
    return paths, bands


@pytest.fixture(scope="module")
def stage(tmp_path_factory):
    """one georeferenced test-stage run, shared: its inputs, the labels predict_step gives, and the output folder"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    from flair_hub.tasks import trainers
    root = str(tmp_path_factory.mktemp("stage"))
    os.makedirs(os.path.join(root, "labels"))
    paths, bands = _write_labels(os.path.join(root, "labels"))
    csv_path = os.path.join(root, "test.csv")
    with open(csv_path, "w", newline="") as f:
        wr = csv.writer(f)
        wr.writerow([MOD, TASK, LPIS])
        for j in range(N_SAMPLES):
            wr.writerow([f"img_{j}.tif", paths[TASK][j], paths[LPIS][j]])
    task, cfg = _fusion_task()
    cfg["paths"] = {"out_model_name": "unet", "test_csv": csv_path}
    cfg["tasks"] = {"predict": True, "metrics_only": False, "write_files": True, "georeferencing_output": True}
    g = torch.Generator().manual_seed(21)
    batches = []
    for lo, hi in ((0, 2), (2, 3)):  # batch size 2, then the remainder
        B = hi - lo
        batches.append({MOD: torch.randn(B, 5, SIZE, SIZE, generator=g),
                        DEM: torch.randn(B, 2, SIZE // 2, SIZE // 2, generator=g),
                        f"ID_{TASK}": paths[TASK][lo:hi], f"ID_{LPIS}": paths[LPIS][lo:hi]})
    out_dir = os.path.join(root, "out")
    writer = trainers.predict(cfg, _DataModule(batches), task, out_dir)
    want = {TASK: [], LPIS: []}
    with torch.no_grad():
        for b in batches:
            out = task.predict_step({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()})
            for t in want:
                want[t] += list(out[f"preds_{t}"].cpu().numpy())
    return {"root": root, "out": out_dir, "paths": paths, "bands": bands, "want": want, "cfg": cfg, "task": task,
            "batches": batches, "writer": writer}


def _confmat(bands, preds, K):
    cm = np.zeros((K, K), dtype=np.int64)
    for t, p in zip(bands, preds):
        ok = t < K
        cm += np.bincount(t[ok].astype(np.int64) * K + p[ok], minlength=K * K).reshape(K, K)
    return cm


@pytest.mark.parametrize("task_name,K", [(TASK, 19), (LPIS, 23)])
def test_prediction_files_matrix_and_metrics(cuda, stage, task_name, K, tmp_path):
    from flair_hub.writer.metrics_utils import compute_and_save_metrics
    from flair_zonal_detection.geotiff import GeoTiffRaster
    pred_dir = os.path.join(stage["out"], "predictions_unet", task_name)
    assert sorted(os.listdir(pred_dir)) == sorted("PRED_" + os.path.basename(p) for p in stage["paths"][task_name])
    written = []
    for j, label_path in enumerate(stage["paths"][task_name]):
        with GeoTiffRaster(os.path.join(pred_dir, "PRED_" + os.path.basename(label_path))) as got, \
                GeoTiffRaster(label_path) as ref:
            assert got.count == 1 and got.dtypes == ("uint8",) and got.profile["compress"] == "lzw"
            assert (got.left, got.top, got.res, got.crs) == (ref.left, ref.top, ref.res, ref.crs)
            assert got.crs == CRS and got.res == (RES, RES)
            arr = got.read(1)
        assert np.array_equal(arr, stage["want"][task_name][j]), j  # sample 1 of the first batch included
        written.append(arr)
    cm = _confmat(stage["bands"][task_name], written, K)
    assert cm.sum() > 0 and cm.sum() < N_SAMPLES * SIZE * SIZE  # the values >= K were left out
    folder = os.path.join(stage["out"], "metrics_unet", task_name)
    saved = np.load(os.path.join(folder, "confmat_predict.npy"))
    assert saved.shape == (K, K) and np.array_equal(saved, cm)
    assert np.array_equal(stage["writer"].accumulated_confmats[task_name].cpu().numpy(), cm)
    compute_and_save_metrics(cm, stage["cfg"], str(tmp_path), task_name, mode="predict")
    with open(os.path.join(folder, "metrics.json")) as f, \
            open(tmp_path / "metrics_unet" / task_name / "metrics.json") as g:
        assert f.read() == g.read()


def test_metrics_only_scores_the_written_files(cuda, stage, tmp_path):
    import shutil
    from flair_hub.tasks import trainers
    cfg = dict(stage["cfg"], tasks=dict(stage["cfg"]["tasks"], predict=False, metrics_only=True))
    out = str(tmp_path / "out")
    shutil.copytree(stage["out"], out)  # the shared run stays as it is
    os.remove(os.path.join(out, "predictions_unet", LPIS, "PRED_LPIS_2.tif"))  # one prediction goes missing
    writer = trainers.predict(cfg, None, None, out)
    for task_name, K in ((TASK, 19), (LPIS, 23)):
        folder = os.path.join(out, "metrics_unet", task_name)
        n = N_SAMPLES - (task_name == LPIS)
        cm = _confmat(stage["bands"][task_name][:n], stage["want"][task_name][:n], K)
        assert np.array_equal(np.load(os.path.join(folder, "confmat_metrics_only.npy")), cm)
        assert np.array_equal(writer.accumulated_confmats[task_name].cpu().numpy(), cm)
        if task_name == TASK:  # all files there: the matrix of the predict run
            assert np.array_equal(cm, np.load(os.path.join(folder, "confmat_predict.npy")))
        with open(os.path.join(folder, "metrics.json")) as f:
            assert json.load(f)["classes"]


def test_plain_tiff_output_reads_back_through_pillow(cuda, stage, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from flair_hub.tasks.trainers import HipTrainer
    from flair_hub.writer.prediction_writer import PredictionWriter
    cfg = dict(stage["cfg"], tasks=dict(stage["cfg"]["tasks"], georeferencing_output=False))
    writer = PredictionWriter(cfg, str(tmp_path))
    trainer = HipTrainer(callbacks=[writer])
    assert trainer.predict(stage["task"], dataloaders=stage["batches"], return_predictions=False) == []
    for task_name in (TASK, LPIS):
        for j, label_path in enumerate(stage["paths"][task_name]):
            path = tmp_path / "predictions_unet" / task_name / ("PRED_" + os.path.basename(label_path))
            with Image.open(path) as im:
                assert im.mode == "L" and im.size == (SIZE, SIZE)
                assert np.array_equal(np.array(im), stage["want"][task_name][j])
    # and the trainer without callbacks behaves as before: the predictions, nothing written
    outs = HipTrainer().predict(stage["task"], dataloaders=stage["batches"][:1])
    assert torch.equal(outs[0][f"preds_{TASK}"].cpu(), torch.from_numpy(np.stack(stage["want"][TASK][:2])))
