"""Every kernel call of the fp32 programs, checked in situ against float64 (tests/insitu.py).

``hardware.precision: fp32`` runs on kernel instantiations of its own -- conv_igemm_kernel<float> and
conv3x3_persist_kernel<float> on the f32 MFMA, the f32 configurations of conv_wgrad_kernel, the f32 templates of the
BatchNorm, pooling, loss, resampling and layout kernels -- which the per-kernel tests hold to 1e-4 against torch-CPU f32
and the whole-model tests to 1e-2 on the gradients (the avalanche through 50 BatchNorms).  Here the real steps run under
a Recorder and every call is held to

    stored activations:  |o - r| <= ulp_f32(r) + 2^-16 a        f32 sums:  |o - r| <= 2^-16 a

against float64 on the call's own inputs: two orders of magnitude above honest f32 summation, below one dropped term
of any reduction of the model, and 128 times below what a bf16 operand or a bf16 detour of the output leaves
(tests/test_insitu_checker.py has the power of these bounds, without a GPU).

The sizes are the smallest that still reach both tile geometries (output width >= 32 and < 32), ragged tile ends,
several tiles per persistent block (FFA_CONV_PERSIST_GRID=8) and both slab-count branches of the weight-gradient reduce.
The helpers are those of the bf16 files, with the precision handed in.
"""
import time

import pytest
import torch

from helpers import MOD
from insitu import AMBIG_MAX_FRACTION, PREDICT_MODES
from test_insitu_fusion_gpu import _batch as _fusion_batch
from test_insitu_fusion_gpu import _checked_step as _checked_fusion_step
from test_insitu_fusion_gpu import _report_and_assert as _report_and_assert_fusion
from test_insitu_fusion_gpu import _task as _fusion_task
from test_insitu_gpu import _assert_default_switches, _checked_step, _families, _report_and_assert
from test_insitu_infer_gpu import CLASSES, _assert_eval_coverage, _eval_forward, _report, trained_task

pytestmark = pytest.mark.gpu

PERSIST_GRID = ("FFA_CONV_PERSIST_GRID",)
# (kernel, stride) of the convolutions of ResNet-34 + U-Net: stem, body, the stride-2 entries of layers 2 to 4, their
# 1x1 shortcuts
CONV_SHAPES = {("7x7", 2), ("3x3", 1), ("3x3", 2), ("1x1", 2)}
TRAIN_FAMILIES = {"fwd:igemm", "dgrad_dil2", "dgrad_residual", "maxpool_bwd_add", "wgrad", "softmax_ce"}
CONV_FAMILIES = ("fwd", "dgrad", "upcat_fwd", "upcat_dgrad", "upcat_wgrad", "wgrad")


def _assert_f32_routing(rec):
    """every conv-family call of the step is an f32 call on a conv_igemm operand: the ring16, thin and stem layouts are
    bf16-only (ring takes f32 under FFA_RING=1 alone, which no case here sets)"""
    convs = [c for c in rec.calls if str(c.get("family", "")).startswith(CONV_FAMILIES)]
    assert convs
    wrong = [(c["op"], c.get("module"), c.get("layout"), c.get("dtype")) for c in convs
             if c.get("dtype") != "float32" or c.get("layout") not in ("igemm", "general")]
    assert not wrong, f"conv calls of the fp32 step off the f32 conv_igemm / conv_wgrad kernels: {wrong[:10]}"


def _assert_upcat_routing(rec, fused_families):
    """the two-source kernels wherever ops.upcat_supported accepts the channel split in f32, elsewhere the materialised
    upsample2x_concat_* calls (checked like any other call)"""
    from flairhip import ops
    fams = _families(rec)
    fused = [c for c in rec.calls if c.get("family") in fused_families]
    plain = [c for c in rec.calls if c.get("family") == "upsample2x_concat_fwd"]
    assert fused or plain, sorted(fams)
    refused = [(c["family"], c["c1"], c["c2"]) for c in fused if not ops.upcat_supported(c["c1"], c["c2"], torch.float32)]
    assert not refused, f"two-source calls on splits upcat_supported refuses: {refused}"
    missed = [(c["c1"], c["c2"]) for c in plain if ops.upcat_supported(c["c1"], c["c2"], torch.float32)]
    assert not missed, f"materialised concat on splits the two-source kernels take: {missed}"
    if fused:
        assert set(fused_families) <= fams, sorted(fams)
    if plain and "upcat_dgrad" in fused_families:
        assert "upsample2x_concat_bwd" in fams, sorted(fams)
    return len(fused), len(plain)


def _assert_training_coverage(rec):
    calls = rec.calls
    fams = _families(rec)
    fwd = {(c["kernel"], c["stride"]) for c in calls if c.get("family") == "fwd" and c.get("layout") == "igemm"}
    assert CONV_SHAPES <= fwd, f"forward conv shapes seen: {sorted(fwd)}"
    wgrads = {(c["kernel"], c["stride"]) for c in calls if c.get("family") == "wgrad"}
    assert CONV_SHAPES <= wgrads, f"weight-gradient shapes seen: {sorted(wgrads)}"
    persistent = {bool(c["persistent"]) for c in calls if "persistent" in c}
    assert persistent == {True, False}, f"conv3x3_persist_kernel / one-tile launches seen: {persistent}"
    n_fused, n_plain = _assert_upcat_routing(rec, ("upcat_fwd", "upcat_dgrad", "upcat_wgrad"))
    print(f"decoder inputs: {n_fused} two-source calls, {n_plain} materialised")
    _assert_f32_routing(rec)
    assert rec.ambiguous[0] <= AMBIG_MAX_FRACTION * rec.ambiguous[1], rec.ambiguous


def test_every_kernel_of_the_fp32_step_at_2x256_matches_float64(cuda):
    t0 = time.perf_counter()
    _assert_default_switches()
    task, rec, _ = _checked_step(2, "full", seed=61, chunk=1, precision="fp32", hw=(256, 256))
    _report_and_assert(task, rec, t0, required=TRAIN_FAMILIES)
    _assert_training_coverage(rec)


def test_every_kernel_of_the_fp32_step_at_3x96x160_with_a_persistent_grid_of_8_matches_float64(cuda, monkeypatch):
    """non-square, odd batch: the bottleneck is 3 x 5, the tiles have ragged ends, and a grid of 8 persistent blocks
    makes every conv3x3_persist_kernel launch walk several tiles"""
    t0 = time.perf_counter()
    monkeypatch.setenv(PERSIST_GRID[0], "8")
    _assert_default_switches(allowed_env=PERSIST_GRID)
    task, rec, _ = _checked_step(3, "full", seed=67, chunk=1, precision="fp32", hw=(96, 160))
    _report_and_assert(task, rec, t0, required=TRAIN_FAMILIES)
    _assert_training_coverage(rec)


def test_every_kernel_of_the_fp32_eval_forward_and_its_uint8_outputs_match_float64(cuda):
    """the eval forward at 3 x 96 x 160 after two eager fp32 training steps (the running statistics have moved): folded
    f32 operands (w * scale in f32), the shift as the bias, residual + ReLU in the epilogue; then predict_u8 in its three
    modes on the f32 logits and a two-view test-time augmentation on their square left part"""
    from flairhip import ops
    t0 = time.perf_counter()
    _assert_default_switches()
    task = trained_task("fp32")

    def outputs(logits):
        nhwc, k = logits._ffa_nhwc, logits._ffa_classes
        assert nhwc.dtype == torch.float32 and k == CLASSES
        for mode in PREDICT_MODES:
            ops.predict_u8(nhwc, k, mode, crop=(5, 7, 80, 140))
        sq = nhwc[:, :, :96].contiguous()  # rotations need square tiles
        acc = ops.tta_buffer(sq.shape[0], k, 64, 64, sq.device, cp=sq.shape[-1])
        ops.tta_accumulate_(acc, sq, k, 0, crop=(16, 16, 64, 64), first=True)
        ops.tta_accumulate_(acc, sq, k, 4, crop=(16, 16, 64, 64))
        for mode in PREDICT_MODES:
            ops.tta_predict_u8(acc, mode, 2)

    rec = _eval_forward(task, 3, 96, 160, seed=71, after=outputs)
    _report(rec, t0)
    _assert_eval_coverage(rec, layouts=("igemm",))
    _assert_f32_routing(rec)
    _assert_upcat_routing(rec, ("upcat_fwd",))
    by_family = {}
    for c in rec.calls:
        by_family.setdefault(c.get("family"), []).append(c)
    assert [c["mode"] for c in by_family["predict_u8"]] == list(PREDICT_MODES)
    assert [(c["code"], c["first"]) for c in by_family["tta_accumulate_"]] == [(0, True), (4, False)]
    assert [(c["mode"], c["views"]) for c in by_family["tta_predict_u8"]] == [(m, 2) for m in PREDICT_MODES]
    assert set(rec.open) == {"band", "confidence"}


def test_every_kernel_of_the_fp32_fusion_step_96_64_with_a_persistent_grid_of_8_matches_float64(cuda, monkeypatch):
    """aerial 96 px, DEM 64 px, batch 3: what the U-Net step does not reach in f32 -- the column blocks of the fusion
    1x1 weight, the f32 bilinear forward and backward at ratio 1.5 (checked against the coordinate the kernel takes), two
    loss nodes with an upstream gradient other than 1"""
    from test_insitu_fusion_gpu import DEM
    t0 = time.perf_counter()
    monkeypatch.setenv(PERSIST_GRID[0], "8")
    _assert_default_switches(allowed_env=PERSIST_GRID)
    task = _fusion_task(precision="fp32", sizes={MOD: 96, DEM: 64}, aux_loss=True, lpis_weight=0.5)
    rec, _ = _checked_fusion_step(task, _fusion_batch(3, 96, 64, seed=79))
    _report_and_assert_fusion(task, rec, t0, 96, 64, True, 0.5)
    _assert_f32_routing(rec)
    assert rec.ambiguous[0] <= AMBIG_MAX_FRACTION * rec.ambiguous[1], rec.ambiguous
