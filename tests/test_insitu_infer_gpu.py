"""Every kernel call of the bf16 zonal inference step, checked in situ against float64 (tests/insitu.py).

In eval mode the program differs from the training step in the places the training in-situ tests never reach:
nn._eval_folded folds gamma / sqrt(running_var + eps) into the packed bf16 operand of every layout (ring16, thin, stem,
igemm and the two-source conv2d_upcat), the shift goes in as the conv bias, the residual add and the ReLU happen in the
conv epilogue, and the outputs come from predict_u8 or -- under test-time augmentation -- from d4_layout,
tta_accumulate_ and tta_predict_u8.  Here the eval forward and the whole zonal tile loop run under a Recorder: each conv
call against the float64 convolution with bf16(w * scale) as the packer forms it (the scale vector itself against
float64 as bn_eval_params' output), each uint8 output against the float64 softmax of the call's own logits.

The model state is not the initial one: two eager training steps with the product's optimizer move gamma, beta and the
running statistics before task.eval().
"""
import time

import numpy as np
import pytest
import torch

from helpers import MOD, TASK, make_pair
from insitu import OPEN_MAX_SHARE, Recorder
from test_insitu_gpu import GRID_CAPS, _assert_default_switches, _families
from test_tta_zonal_gpu import base_cfg, run  # noqa: F401  (base_cfg: the module-scoped fixture of the zonal TTA tests)

pytestmark = pytest.mark.gpu

CLASSES = 19
# ops functions and families that belong to a training step: none of them may run in eval mode
TRAINING_OPS = {"conv2d_bn_stats", "conv2d_upcat_bn_stats", "conv2d_pro_bn_stats", "conv2d_pro", "bn_stats", "bn_apply",
                "bn_bwd", "bn_bwd_partials", "conv2d_bnbwd", "conv_wgrad", "conv_wgrad_upcat", "conv_wgrad_pro",
                "conv2d_dgrad_upcat", "softmax_ce", "scale_inplace", "channel_sums", "maxpool3x3s2_bwd",
                "upsample2x_concat_bwd", "bilinear_bwd"}
HEAD = f"main_decoders.{TASK}.seg_model.segmentation_head.0"


def trained_task(precision):
    """the task after two eager training steps (2 x 128 x 128), in eval mode"""
    from flairhip.optim import HipAdamW
    task, _, _ = make_pair(precision=precision)
    task.train()
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    assert isinstance(opt, HipAdamW), type(opt)
    before = {k: v.clone() for k, v in task.model.state_dict().items() if "running_" in k}
    g = torch.Generator().manual_seed(43)
    for step in range(2):
        batch = {MOD: torch.randn(2, 5, 128, 128, generator=g).cuda(),
                 TASK: torch.randint(0, CLASSES, (2, 128, 128), generator=g).to(torch.uint8).cuda()}
        loss = task.training_step(batch, step)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    after = task.model.state_dict()
    still = [k for k, v in before.items() if torch.equal(v, after[k])]
    assert before and not still, f"running statistics the two steps did not move: {still[:5]}"
    task.eval()
    return task


@pytest.fixture(scope="module")
def trained(cuda):
    return trained_task("bf16")


def _eval_forward(task, B, H, W, seed, after=None):
    """the eval forward under a Recorder; after(logits): further ops calls on the logits inside the same recording"""
    x = torch.randn(B, 5, H, W, generator=torch.Generator().manual_seed(seed)).cuda()
    with Recorder(task.model, mode="full", chunk=1) as rec, torch.no_grad():
        logits, _ = task.model({MOD: x})
        if after is not None:
            after(logits[TASK])
        torch.cuda.synchronize()
    assert tuple(logits[TASK].shape) == (B, CLASSES, H, W)
    return rec


def _report(rec, t0):
    print(f"\n{rec.table()}\nchecked calls: {len(rec.calls)}; wall time {time.perf_counter() - t0:.1f} s")
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    fails = rec.failures()
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])
    for kind, (n_open, n) in rec.open.items():
        assert n_open <= OPEN_MAX_SHARE * n, (kind, n_open, n)


def _assert_eval_coverage(rec, layouts=("ring16", "thin", "stem")):
    """layouts: the operand layouts of the 3x3 / 7x7 convs of the step (bf16: ring16, thin and stem; f32: igemm alone)"""
    calls = rec.calls
    training = sorted({c["op"] for c in calls if c["op"] in TRAINING_OPS or c.get("stats")
                       or str(c.get("family", "")).startswith(("dgrad", "bn_bwd", "wgrad", "upcat_dgrad", "upcat_wgrad"))})
    assert not training, f"training-family calls in the eval step: {training}"

    def seen(family, layout=None, **flags):
        return any(c.get("family") == family and (layout is None or c.get("layout") == layout)
                   and all(c.get(k) == v for k, v in flags.items()) for c in calls)

    required = {f"fwd:{lay} bias+relu": seen("fwd", lay, folded=True, bias=True, relu=True, residual=False)
                for lay in layouts}
    required.update({
        f"fwd:{layouts[0]} residual+relu": seen("fwd", layouts[0], folded=True, bias=True, relu=True, residual=True),
        "fwd:igemm 1x1 stride-2 bias, no relu": seen("fwd", "igemm", folded=True, kernel="1x1", stride=2, bias=True,
                                                     relu=False, residual=False),
        "upcat_fwd bias+relu": seen("upcat_fwd", folded=True, bias=True, relu=True),
        "bn_eval_params": seen("bn_eval_params"),
    })
    missing = sorted(k for k, ok in required.items() if not ok)
    assert not missing, f"the eval step no longer reaches {missing} (routing moved: update the list and the checks); " \
                        f"families seen: {sorted(_families(rec))}"
    # one checked scale / shift pair per folded layer: ResNet-34 has 36 BatchNorms, the five decoder blocks two each
    folded = {c["module"] for c in calls if c.get("folded")}
    assert len(folded) == sum(1 for c in calls if c.get("family") == "bn_eval_params") == 46, sorted(folded)


def test_every_kernel_of_the_bf16_eval_forward_at_3x96x160_matches_float64(trained):
    """non-square: the bottleneck is 3 x 5, the ring and thin tiles have ragged ends"""
    t0 = time.perf_counter()
    _assert_default_switches()
    rec = _eval_forward(trained, 3, 96, 160, seed=47)
    _report(rec, t0)
    _assert_eval_coverage(rec)


def test_every_kernel_of_the_bf16_eval_forward_at_2x256_with_low_grid_caps_matches_float64(trained, monkeypatch):
    """forced caps of 8 blocks: every ring, thin and stem launch walks many tiles per block"""
    t0 = time.perf_counter()
    for k in GRID_CAPS:
        monkeypatch.setenv(k, "8")
    _assert_default_switches(allowed_env=GRID_CAPS)
    rec = _eval_forward(trained, 2, 256, 256, seed=53)
    _report(rec, t0)
    _assert_eval_coverage(rec)


# ---- the zonal tile loop ---------------------------------------------------------------------------------------------------

OUTPUTS = {"argmax": {"output_type": "argmax"}, "class_prob": {"output_type": "class_prob"},
           "confidence": {"write_confidence": True}}


@pytest.fixture(scope="module")
def frequent_class(cuda, base_cfg):
    """the label this model writes most often on this raster (one plain bf16 run): the class to duplicate when a tie of
    the top two has to be planted -- a copy of a class that never wins ties only below the top"""
    label = run(base_cfg, hardware={"precision": "bf16"}, hip_graph=False)[TASK].data
    return int(np.bincount(label.ravel(), minlength=CLASSES).argmax())


def _recorded_run(base_cfg, monkeypatch, keys, plant=None):
    """run_inference under a Recorder; the model it builds is handed to the recorder (module names).  plant: the class
    whose head weights and bias are copied onto the next class, so that the two tie exactly in every pixel and view."""
    from flair_zonal_detection import inference
    build = inference.build_inference_model
    rec = Recorder(None, mode="full", chunk=1)

    def build_and_adopt(config, patch_sizes):
        model = build(config, patch_sizes)
        if plant is not None:
            params = dict(model.named_parameters())
            with torch.no_grad():
                for leaf in ("weight", "bias"):
                    params[f"{HEAD}.{leaf}"][(plant + 1) % CLASSES] = params[f"{HEAD}.{leaf}"][plant]
        rec.adopt(model)
        return model

    with monkeypatch.context() as m, rec:
        m.setattr(inference, "build_inference_model", build_and_adopt)
        out = run(base_cfg, hardware={"precision": "bf16"}, hip_graph=False, **keys)
        torch.cuda.synchronize()
    return rec, out


@pytest.mark.parametrize("output", sorted(OUTPUTS))
@pytest.mark.parametrize("tta", ["none", "d4"])
def test_every_kernel_of_the_bf16_zonal_run_matches_float64(cuda, base_cfg, frequent_class, monkeypatch, tta, output):
    """200 x 260 raster, patch 128, margin 16, batch 4: several batches, the last one partial, one forward per view.

    Ties: the label checks are exact, so they must have met an exact tie of the top two.  Without TTA the labels come
    from bf16 logits, which tie by themselves (measured: 1274 of the 82944 written pixels).  Under d4 they come from
    f32 sums of eight softmax values, which do not: there the tie is planted from the start -- the most frequent class
    is copied onto its neighbour -- and a run without TTA that met no tie is repeated with the plant."""
    t0 = time.perf_counter()
    _assert_default_switches()
    keys = dict(OUTPUTS[output], tta=tta)
    label_op = "predict_u8" if tta == "none" else "tta_predict_u8"
    rec, out = _recorded_run(base_cfg, monkeypatch, keys, plant=frequent_class if tta == "d4" else None)
    if tta == "none" and output != "class_prob" and not rec.ties[label_op]:
        rec, out = _recorded_run(base_cfg, monkeypatch, keys, plant=frequent_class)
    _report(rec, t0)
    fams = _families(rec)
    want = {"predict_u8"} if tta == "none" else {"d4_layout", "tta_accumulate_", "tta_predict_u8"}
    assert want <= fams, sorted(fams)
    assert not ({"predict_u8", "d4_layout", "tta_accumulate_", "tta_predict_u8"} - want) & fams, sorted(fams)
    assert "bn_eval_params" in fams and any(c.get("folded") for c in rec.calls)
    mode = {"argmax": "argmax", "class_prob": "class_prob", "confidence": "argmax_conf"}[output]
    finals = [c for c in rec.calls if c.get("family") == label_op]
    n = len(finals)
    assert n >= 2 and all(c["mode"] == mode for c in finals), finals
    if tta == "d4":
        views = [c for c in rec.calls if c.get("family") == "tta_accumulate_"]
        assert [c["code"] for c in views] == list(range(8)) * n and [c["first"] for c in views] == ([True] + [False] * 7) * n
        assert all(c["crop"] == (16, 16, 96, 96) for c in views) and all(c["views"] == 8 for c in finals)
        assert sum(c["logit_ties"] for c in views) > 0
    else:
        assert all(c["crop"] == (16, 16, 96, 96) for c in finals)
    if output != "class_prob":
        assert rec.ties[label_op] > 0, "no exact tie of the top two among the checked labels"
    assert out[TASK].data.any()


def test_graph_and_eager_runs_write_the_same_bytes_without_tta(cuda, base_cfg):
    keys = {"tta": "none", "write_confidence": True, "hardware": {"precision": "bf16"}}
    graphed = run(base_cfg, hip_graph=True, **keys)
    eager = run(base_cfg, hip_graph=False, **keys)
    assert set(graphed) == set(eager) == {TASK, TASK + "_confidence"}
    for key in graphed:
        assert np.array_equal(graphed[key].data, eager[key].data), key
    assert graphed[TASK].data.any() and graphed[TASK + "_confidence"].data.any()
