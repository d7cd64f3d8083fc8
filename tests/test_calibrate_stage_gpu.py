"""The calibration stage and the zonal run that applies its file, at toy size.

Stage (flair_hub.tasks.stages.calibrate_stage) on the resnet34-unet of tests/test_eval_stage_gpu.py at 64 x 64 with
seeded weights, three host batches of 2, 2 and 1 samples: the thresholds of the written best_thresholds.yaml equal
flairhip.calibration.best_thresholds of a histogram rebuilt in numpy from the model's own 'class_prob' bytes, and its
iou_thresholded the IoU of the confusion matrix of the label rule applied in numpy to those bytes and logits.

Zonal run (setup of tests/test_tta_zonal_gpu.py: patch 128, margin 16, a 200 x 260 raster, graded logits): with a
threshold file the label raster equals the rule applied in numpy to the class-probability raster of a second run
(output_type: class_prob).  The raster holds the bytes, not the logits the rule orders by.  A byte is monotone in its
logit, so the chosen class holds the largest passing byte: where one passing class holds it (at least 90 % of the
pixels, asserted) the label is that class, exactly; where several do, the label is one of them; the confidence is that
byte everywhere.  With the file absent the outputs are those of a run without the key.
"""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

from helpers import MOD, ROOT, TASK, make_pair, oracle_to_product_keys

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
K = 19


def rule(score, q, thr, fallback):
    """score, q: [K, ...]; the label rule of include/flairhip_calib.h in numpy -> uint8 labels"""
    ok = q >= np.asarray(thr, dtype=np.uint8).reshape((-1,) + (1,) * (q.ndim - 1))
    return np.where(ok.any(0), np.where(ok, score, -np.inf).argmax(0), fallback).astype(np.uint8)


# ---- the stage ---------------------------------------------------------------------------------------------------------

class _ValModule:
    def __init__(self, batches):
        self.batches = batches

    def setup(self, stage):
        assert stage == "validate"

    def val_dataloader(self):
        return self.batches


def _val_batches(task=None):
    """three host batches of 2, 2 and 1 samples; with ``task``, the labels are the model's own predictions with 30 % of
    the pixels redrawn at random, so that a class's pixels sit at its high scores and every class has support"""
    g = torch.Generator().manual_seed(11)
    out = []
    for B in (2, 2, 1):
        x = torch.randn(B, 5, 64, 64, generator=g)
        labels = torch.randint(0, K, (B, 64, 64), generator=g)
        if task is not None:
            with torch.no_grad():
                _, preds, _ = task.step({MOD: x.cuda(), TASK: labels.cuda()}, training=False)
            labels = torch.where(torch.rand(labels.shape, generator=g) < 0.3, labels, preds[TASK].cpu().long())
        out.append({MOD: x, TASK: labels})
    return out


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """one stage run, shared: the file it wrote and, per batch, the model's class_prob bytes, logits and targets"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU in this environment")
    from flairhip import ops
    from flair_hub.tasks.stages import calibrate_stage
    out_dir = str(tmp_path_factory.mktemp("calibrate"))
    task, _, cfg = make_pair(precision="bf16", seed=5)
    task.eval()
    cfg["tasks"] = {"calibrate": True}
    batches = _val_batches(task)
    path = calibrate_stage(cfg, _ValModule(batches), out_dir, seg_module=task)
    seen = []
    with torch.no_grad():
        for b in batches:
            logits = {}
            _, _, targets = task.step({k: v.cuda() for k, v in b.items()}, training=False, logits_out=logits)
            nhwc = logits[TASK]._ffa_nhwc
            q = ops.predict_u8(nhwc, K, "class_prob").cpu().numpy()        # [B, K, H, W]
            z = nhwc[..., :K].float().cpu().numpy().transpose(0, 3, 1, 2)  # [B, K, H, W]
            seen.append((q, z, targets[TASK].cpu().numpy()))
    return {"path": path, "out_dir": out_dir, "seen": seen, "cfg": cfg}


def test_stage_writes_the_thresholds_of_the_rebuilt_histogram(cuda, staged):
    from flairhip import calibration as cal
    assert staged["path"] == os.path.join(staged["out_dir"], "checkpoints", "best_thresholds.yaml")
    doc = yaml.safe_load(open(staged["path"]))
    assert list(doc) == [TASK]
    entry = doc[TASK]
    hist = np.zeros((K, 2, 256), dtype=np.int64)
    cm = np.zeros((K, K), dtype=np.int64)
    for q, z, t in staged["seen"]:
        for k in range(K):
            for side in (0, 1):
                hist[k, side] += np.bincount(q[:, k][(t == k) == bool(side)], minlength=256)
        cm += np.bincount(t.reshape(-1).astype(np.int64) * K + z.argmax(1).reshape(-1), minlength=K * K).reshape(K, K)
    assert np.count_nonzero(hist.sum((0, 1))) > 50, "scores between 0 and 255 occur"
    thr = cal.best_thresholds(hist, "iou")
    assert entry["thresholds_u8"] == thr.tolist() and min(entry["thresholds_u8"]) >= 1
    assert entry["thresholds"] == [t / 255.0 for t in thr.tolist()]
    assert entry["objective"] == "iou" and entry["fallback"] == 18
    names = staged["cfg"]["labels_configs"][TASK]["value_name"]
    assert entry["class_names"] == [names[i] for i in range(K)]
    assert entry["support"] == hist[:, 1].sum(1).tolist()
    assert entry["ece"] == cal.expected_calibration_error(hist).tolist()
    assert entry["iou_argmax"] == cal.iou_from_confmat(cm).tolist()
    assert entry["iou_one_vs_rest"] == cal.sweep(hist)["iou"][np.arange(K), thr].tolist()
    assert np.array_equal(cal.read_thresholds(staged["path"], K, task=TASK)["thresholds_u8"], thr)


def test_stage_reports_the_iou_of_the_label_rule(cuda, staged):
    from flairhip import calibration as cal
    entry = yaml.safe_load(open(staged["path"]))[TASK]
    thr = entry["thresholds_u8"]
    cm = np.zeros((K, K), dtype=np.int64)
    changed = 0
    for q, z, t in staged["seen"]:
        for b in range(q.shape[0]):
            label = rule(z[b], q[b], thr, 18)
            changed += int((label != z[b].argmax(0)).sum())
            cm += np.bincount(t[b].reshape(-1).astype(np.int64) * K + label.reshape(-1), minlength=K * K).reshape(K, K)
    print(f"{changed} labels moved by the thresholds")
    assert changed > 0, "the thresholds move some labels"  # about 250 of 20 480 on the float32 oracle of this network
    assert entry["iou_thresholded"] == cal.iou_from_confmat(cm).tolist()


def test_stage_without_the_second_pass(cuda, tmp_path):
    from flair_hub.tasks.stages import calibrate_stage
    task, _, cfg = make_pair(precision="bf16", seed=5)
    cfg["tasks"] = {"calibrate": True, "calibrate_verify": False, "calibrate_objective": "f1"}
    path = calibrate_stage(cfg, _ValModule(_val_batches()[:1]), str(tmp_path), seg_module=task)
    entry = yaml.safe_load(open(path))[TASK]
    assert "iou_thresholded" not in entry and entry["objective"] == "f1" and len(entry["thresholds_u8"]) == K
    cfg["tasks"]["calibrate_objective"] = "accuracy"
    with pytest.raises(ValueError):
        calibrate_stage(cfg, _ValModule([]), str(tmp_path), seg_module=task)


# ---- the zonal run ------------------------------------------------------------------------------------------------------

PATCH, MARGIN, RES, H, W = 128, 16, 0.2, 200, 260


@pytest.fixture(scope="module")
def base_cfg(tmp_path_factory):
    from flair_zonal_detection.raster import ArrayRaster
    from oracle.seeded_weights import fill_state_dict
    from oracle.unet_resnet34 import UnetResNet34
    tmp = tmp_path_factory.mktemp("thr_zonal")
    img = np.random.default_rng(3).integers(0, 255, (3, H, W)).astype(np.uint8)
    ras = ArrayRaster(img, 651992.36, 6860417.84, RES)
    cfg = yaml.safe_load(open(os.path.join(GOLD, "zonal_config.yaml")))
    cfg.update({"output_path": str(tmp), "output_name": "z", "img_pixels_detection": PATCH, "margin": MARGIN,
                "output_px_meters": RES, "output_type": "argmax", "batch_size": 4, "num_worker": 0,
                "hardware": {"precision": "fp32"}})
    cfg["modalities"][MOD].update({"input_img_path": ras, "channels": [1, 2, 3],
                                   "normalization": {"type": "custom", "means": [105.66, 111.35, 102.18],
                                                     "stds": [52.23, 45.62, 44.30]}})
    cfg["tasks"] = [{"name": TASK, "active": True, "class_names": {i: f"c{i}" for i in range(K)}}]
    oracle = UnetResNet34(3, K)
    state = fill_state_dict(oracle.state_dict(), seed=77)
    for key in ("segmentation_head.0.weight", "segmentation_head.0.bias"):  # graded probabilities, as in test_tta_zonal_gpu
        state[key] = state[key] * 2.0 ** -8
    oracle.load_state_dict(state)
    cfg["model_weights"] = str(tmp / "w.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in oracle_to_product_keys(oracle.state_dict()).items()}},
               cfg["model_weights"])
    from flairhip.calibration import write_thresholds
    # this model's winners are classes 1, 9, 6 with top scores of 50..140: 80 on the odd classes rejects most of them,
    # 45 on the even ones lets a runner-up in (float32 oracle of the network: about 11 % runner-up and 34 % fallback,
    # 12 % and 61 % under the four flips)
    cfg["_thr"] = [45 if k % 2 == 0 else 80 for k in range(K)]
    cfg["_file"] = write_thresholds(str(tmp / "best_thresholds.yaml"), cfg["_thr"], task=TASK)
    return cfg


def run(base_cfg, **keys):
    from flair_zonal_detection.inference import run_inference
    cfg = copy.deepcopy({k: v for k, v in base_cfg.items() if not k.startswith("_")})
    cfg.update(keys)
    return {k: o.data.copy() for k, o in run_inference(cfg).items()}


@pytest.mark.parametrize("fallback,tta", [(18, "none"), (200, "none"), (18, "flips")])
def test_zonal_labels_follow_the_rule_on_the_class_prob_raster(cuda, base_cfg, fallback, tta):
    thr = np.asarray(base_cfg["_thr"], np.uint8)[:, None, None]
    probs = run(base_cfg, output_type="class_prob", tta=tta)[TASK]  # [K, H, W]
    plain = run(base_cfg, tta=tta)[TASK][0]
    ok = probs >= thr
    fell = ~ok.any(0)
    top = np.where(ok, probs.astype(np.int16), -1).max(0)  # the largest passing byte
    among = ok & (probs == top[None])                # the passing classes that hold it
    unique = among.sum(0) == 1
    want = np.where(fell, fallback, among.argmax(0)).astype(np.uint8)
    moved = unique & (want != plain)
    print(f"one top byte or none {(unique | fell).mean():.3f}, runner-up {moved.mean():.3f}, fallback {fell.mean():.3f}")
    # on the oracle, before comparing
    assert (unique | fell).mean() >= 0.9 and moved.mean() >= 0.05 and fell.mean() >= 0.05 and unique.mean() >= 0.05
    out = run(base_cfg, model_threshold_filepath=base_cfg["_file"], threshold_fallback=fallback, tta=tta)
    assert list(out) == [TASK]
    got = out[TASK][0]
    assert np.array_equal(got[unique | fell], want[unique | fell])
    tied = ~(unique | fell)
    assert np.take_along_axis(among, np.minimum(got, K - 1)[None].astype(np.int64), 0)[0][tied].all()
    assert (got[tied] < K).all()
    # with the confidence raster: the same labels, and the byte of the chosen class
    conf = run(base_cfg, model_threshold_filepath=base_cfg["_file"], threshold_fallback=fallback, tta=tta,
               write_confidence=True)
    assert np.array_equal(conf[TASK][0], got)
    assert np.array_equal(conf[TASK + "_confidence"][0], np.where(fell, 0, top).astype(np.uint8))


def test_an_absent_file_changes_nothing(cuda, base_cfg, caplog):
    import logging
    plain = run(base_cfg, write_confidence=True)
    with caplog.at_level(logging.WARNING):
        out = run(base_cfg, write_confidence=True, model_threshold_filepath=base_cfg["_file"] + ".nowhere")
    assert "does not exist" in caplog.text
    assert sorted(out) == sorted(plain) and all(np.array_equal(out[k], plain[k]) for k in plain)
    caplog.clear()
    probs = run(base_cfg, output_type="class_prob")
    with caplog.at_level(logging.WARNING):
        out = run(base_cfg, output_type="class_prob", model_threshold_filepath=base_cfg["_file"])
    assert "label output" in caplog.text
    assert np.array_equal(out[TASK], probs[TASK])
