"""Every kernel call of the bf16 two-modality fusion step, checked in situ against float64 (tests/insitu.py).

flairhip.configs.fusion_unet_config: two mono-temporal encoders (aerial 5 channels, DEM 2 channels) fused per stage, two
task decoders with task weights and an auxiliary aerial decoder.  Code that runs nowhere else: the 1x1 fusion conv as a
chain of per-source convs over column blocks of one weight (bias on the first link, the chain through the residual
input, per-block wgrads concatenated), the bilinear alignment of the DEM stages at ratios 2 and 1.5 in both directions,
two softmax-CE nodes in one backward with upstream gradients other than 1 (the rescale of dlogits and the loss sums
times the task weight as the head's bias gradient), and with augmentation the flip / rotation layout kernels of both
modalities.

The cases are small on purpose: what is specific to the fusion path does not depend on the workload's size.  No
BatchNorm sees fewer than 16 values per channel (the deepest DEM maps are 2 x 2 at batch 4); should an honest bn_stats /
bn_bwd check exceed its bound there through cancellation in the variance, the remedy is a larger batch here, never a
wider bound.

The auxiliary decoder runs forward only: as in the reference its logits never reach the loss (tasks_module.py
_compute_aux_loss), so a step has one softmax-CE node per task and the aux decoders' parameters stay without a
gradient -- the `unused_parameters` list of tests/golden/fusion_two_mod.json, which every aux-on case asserts.
"""
import json
import os
import time

import pytest
import torch

from helpers import MOD, ROOT, TASK
from insitu import Recorder
from test_insitu_gpu import GRID_CAPS, _assert_default_switches, _families

pytestmark = pytest.mark.gpu

LPIS, DEM = "ALL_LABEL-LPIS", "DEM_ELEV"
GOLD = os.path.join(ROOT, "tests", "golden", "fusion_two_mod.json")


def _task(precision="bf16", **cfg_kw):
    from flairhip.configs import fusion_unet_config
    from flair_hub.tasks.module_setup import build_segmentation_module
    from oracle.seeded_weights import fill_state_dict
    sizes = cfg_kw.pop("sizes")
    cfg = fusion_unet_config(precision=precision, **cfg_kw)
    task = build_segmentation_module(cfg, sizes, "train")
    task.model.load_state_dict(fill_state_dict(task.model.state_dict()))
    return task.cuda()


def _batch(n, aerial, dem, seed, codes=None):
    g = torch.Generator().manual_seed(seed)
    b = {MOD: torch.randn(n, 5, aerial, aerial, generator=g).cuda(),
         DEM: torch.randn(n, 2, dem, dem, generator=g).cuda(),
         TASK: torch.randint(0, 19, (n, aerial, aerial), generator=g).to(torch.uint8).cuda(),
         LPIS: torch.randint(0, 23, (n, aerial, aerial), generator=g).to(torch.uint8).cuda()}
    if codes is not None:
        b["AUG"] = torch.tensor(codes, dtype=torch.uint8).cuda()
    return b


def _checked_step(task, batch, chunk=2):
    """step 1 eager with the product's own optimizer (operands re-packed afterwards), step 2 recorded and checked"""
    from flairhip.optim import HipAdamW
    task.train()
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    assert isinstance(opt, HipAdamW), type(opt)
    loss = task.training_step(batch, 0)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    del loss
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    with Recorder(task.model, mode="full", chunk=chunk) as rec:
        loss = task.training_step(batch, 1)
        loss.backward()
        torch.cuda.synchronize()
    return rec, loss


def _report_and_assert(task, rec, t0, aerial, dem, aux, lpis_weight, codes=None):
    # the grad-source rules first: rule (b) adds its own results to the report
    named = list(task.model.named_parameters())
    orphans = rec.grad_orphans(named)
    print(f"\n{rec.table()}\nchecked calls: {len(rec.calls)}; wall time {time.perf_counter() - t0:.1f} s")
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    fails = rec.failures()
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])
    assert not orphans, f"gradients not produced by a checked call: {orphans[:10]}"

    fams = _families(rec)
    calls = rec.calls
    model = task.model
    # the alignment runs in both directions whenever the modalities differ in size (an identity resize launches nothing)
    resized = aerial != dem
    assert ("bilinear_fwd" in fams) == resized and ("bilinear_bwd" in fams) == resized, sorted(fams)
    if resized:
        ratios = {c["ratio"] for c in calls if c.get("family") in ("bilinear_fwd", "bilinear_bwd")}
        assert ratios == {dem / aerial}, ratios
    # the fusion chain: per mixed stage one forward link per source, the later ones through the residual input
    stages = model.fusion_handler.stage_channels
    mixed = range(1, len(stages[MOD]))
    links = [c for c in calls if c.get("fusion") and c.get("family") == "fwd"]
    assert all(c["kernel"] == "1x1" for c in links)
    assert sum(1 for c in links if c["residual"]) == len(mixed) and sum(1 for c in links if not c["residual"]) == len(mixed)
    dlinks = [c for c in calls if c.get("fusion") and c.get("family", "").startswith("dgrad")]
    assert len(dlinks) == 2 * len(mixed), len(dlinks)
    # 1x1 wgrad calls for every source of every mixed stage
    w11 = [(c["co"], c["ci"], c["hw"]) for c in calls if c.get("family") == "wgrad" and c["kernel"] == "1x1"]
    for s in mixed:
        hw = (aerial >> s, aerial >> s)
        for m in (MOD, DEM):
            want = (model.fusion_handler.conv_f[s].out_channels, stages[m][s], hw)
            assert want in w11, f"no 1x1 wgrad for {m} at stage {s}: {want} not among {w11}"
    # one softmax-CE node per task (the aux logits never reach the loss, see the module docstring), each followed by
    # the rescale of its dlogits; the task weight makes at least one of the scales differ from 1
    n_ce = sum(1 for c in calls if c.get("family") == "softmax_ce")
    assert n_ce == 2, n_ce
    scales = sorted(c["scale"] for c in calls if c.get("family") == "scale_inplace")
    assert scales == sorted([1.0, lpis_weight]), scales
    heads = {k: v["scale"] for k, v in rec.head_bias.items()}
    assert heads == {f"main_decoders.{TASK}.seg_model.segmentation_head.0": 1.0,
                     f"main_decoders.{LPIS}.seg_model.segmentation_head.0": lpis_weight}, heads
    # parameters without a gradient: the reference's own list
    unused = sorted(k for k, p in named if p.grad is None)
    if aux:
        assert unused == json.load(open(GOLD))["unused_parameters"]
    else:
        assert unused and all(k.startswith("fusion_handler.conv_f.0.") for k in unused), unused
    if codes is not None:
        seen = set()
        for c in calls:
            if c.get("family") == "d4_layout":
                seen |= set(c["codes"])
        n_layout = sum(1 for c in calls if c.get("family") == "d4_layout")
        assert n_layout == 2 and seen == set(range(8)), (n_layout, seen)
        assert sum(1 for c in calls if c.get("family") == "d4_labels") == 2


def test_fusion_step_128_64_ratio_2_matches_float64(cuda):
    """case A: integer ratio 2 at every stage, aux decoder on, LPIS weight 0.5"""
    t0 = time.perf_counter()
    _assert_default_switches()
    task = _task(sizes={MOD: 128, DEM: 64}, aux_loss=True, lpis_weight=0.5)
    rec, _ = _checked_step(task, _batch(4, 128, 64, seed=51))
    _report_and_assert(task, rec, t0, 128, 64, True, 0.5)


def test_fusion_step_96_64_ratio_1_5_with_low_grid_caps_matches_float64(cuda, monkeypatch):
    """case B: ratio 1.5 (48 <-> 32 down to 3 <-> 2), odd batch, forced grid caps so that the small layers walk many
    tiles per block.  The deepest DEM maps are 2 x 2 x 3 = 12 values per channel for BatchNorm."""
    t0 = time.perf_counter()
    for k in GRID_CAPS:
        monkeypatch.setenv(k, "8")
    _assert_default_switches(allowed_env=GRID_CAPS)
    task = _task(sizes={MOD: 96, DEM: 64}, aux_loss=True, lpis_weight=0.5)
    rec, _ = _checked_step(task, _batch(3, 96, 64, seed=53))
    _report_and_assert(task, rec, t0, 96, 64, True, 0.5)


def test_fusion_step_96_96_same_size_upstream_gradient_2_matches_float64(cuda):
    """case C: same-size modalities (the identity resize launches no kernel), no aux decoder, LPIS weight 2"""
    t0 = time.perf_counter()
    _assert_default_switches()
    task = _task(sizes={MOD: 96, DEM: 96}, aux_loss=False, lpis_weight=2.0)
    rec, _ = _checked_step(task, _batch(4, 96, 96, seed=57))
    _report_and_assert(task, rec, t0, 96, 96, False, 2.0)


def test_fusion_step_with_all_eight_flips_and_rotations_matches_float64(cuda):
    """case D: as A at batch 8 with batch['AUG'] holding the eight transforms of the square: both modalities go through
    d4_layout, both label maps through d4_labels"""
    t0 = time.perf_counter()
    _assert_default_switches()
    task = _task(sizes={MOD: 128, DEM: 64}, aux_loss=True, lpis_weight=0.5)
    task.config["modalities"]["pre_processings"]["use_augmentation"] = True
    codes = [5, 0, 7, 2, 4, 1, 6, 3]
    rec, _ = _checked_step(task, _batch(8, 128, 64, seed=59, codes=codes))
    _report_and_assert(task, rec, t0, 128, 64, True, 0.5, codes=codes)


def test_fusion_recorder_checks_the_ops_the_step_does_not_reach_on_direct_calls(cuda):
    """mean_stack (several time-series branches), nhwc_to_nchw (generic logits) and the normalising layout kernels of
    raw raster samples have references too; fusion_unet_config calls none of them, so they are called here"""
    import numpy as np
    from flairhip import ops
    t0 = time.perf_counter()
    rs = np.random.RandomState(61)
    g = torch.Generator().manual_seed(61)
    B, C, H, W = 3, 5, 40, 24
    mean = (torch.rand(C, generator=g) * 100 + 50).cuda()
    std = (torch.rand(C, generator=g) * 40 + 20).cuda()
    maps = [torch.randn(B, H, W, 32, generator=g).to(torch.bfloat16).cuda() for _ in range(3)]
    codes = torch.tensor([4, 3, 7, 0, 6, 1], dtype=torch.uint8).cuda()
    with Recorder(torch.nn.Module(), mode="full", chunk=2) as rec:
        ops.u8_nchw_to_nhwc(torch.from_numpy(rs.randint(0, 256, (B, C, H, W)).astype(np.uint8)).cuda(), torch.bfloat16,
                            mean, std, 16)
        for np_t, lo, hi in ((np.uint8, 0, 256), (np.uint16, 0, 65536), (np.int16, -32768, 32768)):
            raw = torch.from_numpy(rs.randint(lo, hi, (B, C, H, W)).astype(np_t)).cuda()
            ops.raw_nchw_to_nhwc(raw, torch.bfloat16, mean, std, 16)
        ops.raw_nchw_to_nhwc(torch.randn(B, C, H, W, generator=g).cuda() * 80 + 90, torch.float32, mean, std, 8)
        sq = torch.from_numpy(rs.randint(0, 65536, (12, C, 24, 24)).astype(np.uint16)).cuda()
        ops.d4_layout(sq, torch.bfloat16, codes, mean, std, 16, group=2)
        ops.mean_stack(maps)
        ops.mean_stack(maps[:1], divisor=3)
        ops.nhwc_to_nchw(maps[0], 19)
        torch.cuda.synchronize()
    print(f"\n{rec.table()}\nchecked calls: {len(rec.calls)}; wall time {time.perf_counter() - t0:.1f} s")
    assert not rec.unchecked, dict(rec.unchecked)
    fails = rec.failures()
    assert not fails, "\n".join(r.line() for r in fails)
    assert [c["family"] for c in rec.calls] == ["layout_norm"] * 5 + ["d4_layout", "mean_stack", "mean_stack",
                                                                     "nhwc_to_nchw"]


def test_graph_replay_of_the_fusion_step_equals_the_checked_eager_step(cuda):
    """GraphedTrainStep (what tools/bench_fusion.py times) replays case A's batch from the same state with the loss and
    parameter gradients of the eager step, bit for bit: the in-situ checks of the eager step speak for the replay"""
    from flairhip import nn as hnn
    from flairhip.graph import GraphedTrainStep
    t0 = time.perf_counter()
    _assert_default_switches()
    task = _task(sizes={MOD: 128, DEM: 64}, aux_loss=True, lpis_weight=0.5)
    task.train()
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    batch = _batch(4, 128, 64, seed=51)
    state = {k: v.clone() for k, v in task.state_dict().items()}
    stepper = GraphedTrainStep(task, opt, batch, warmup_steps=2)
    task.load_state_dict(state)
    hnn.bump_state_epoch()
    loss_g = stepper(stepper.static_batch).detach().clone()
    torch.cuda.synchronize()
    grads_g = {n: p.grad.detach().clone() for n, p in task.model.named_parameters() if p.grad is not None}
    task.load_state_dict(state)
    hnn.bump_state_epoch()
    opt.zero_grad(set_to_none=True)
    loss_e = task.training_step(stepper.static_batch, 0)
    loss_e.backward()
    torch.cuda.synchronize()
    grads_e = {n: p.grad.detach() for n, p in task.model.named_parameters() if p.grad is not None}
    print(f"\ngraph replay vs eager, fusion step at 4 x 128 / 64: loss {loss_g.item():.6f} / {loss_e.item():.6f}, "
          f"{len(grads_e)} gradients; wall time {time.perf_counter() - t0:.1f} s")
    assert torch.equal(loss_g.reshape(()), loss_e.detach().reshape(()))
    assert grads_g.keys() == grads_e.keys() and len(grads_e) > 200
    diff = [n for n in grads_e if not torch.equal(grads_g[n], grads_e[n])]
    assert not diff, f"{len(diff)} gradients differ between replay and eager step, e.g. {diff[:5]}"
