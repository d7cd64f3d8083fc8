"""Every kernel call of the U-TAE training step and of its evaluation forward, checked in situ against float64.

flairhip/utae.py holds arithmetic of its own between the kernels of csrc/temporal.hip (tests/test_temporal_kernels_gpu.py
calls them one by one, on arguments of its own) and the whole-step comparison with the reference's gradients
(tests/test_utae_gpu.py: one shape, both dropouts off, a gradient-norm ratio within (0.7, 1.4) in bf16): the input
gradient of a reflect-padded conv as a pad-2 conv with the transposed operand and out_hw, ConvTranspose2d(3, 1, 1) as a
pad-1 conv on a transposed operand with the roles of x and dy exchanged in its weight gradient, conv1 over
cat([up, skip]) as two convs over column slices of one weight chained through the residual input, the class-score layer
at the logits pitch with padded BatchNorm vectors, bias gradients as column sums, the attention gradient that every
temporal_aggregate_bwd sends to ltae_attention_bwd, mask_images_ as its own backward, both dropouts as multiplies,
evaluation-mode BatchNorm folded through HipUTAE._packed.  Here the real step runs under tests/insitu.py's Recorder with
both dropouts at their defaults (0.2 and 0.1): every flairhip.ops call is held, on its own inputs (padded dates, dropout
masks, the saved prob and dattn_ext among them), to a float64 restatement of the reference's formula within
ulp_stored(r) + 2^-16 a, f32 outputs within 2^-16 a, copies and flags exactly; every operand of HipUTAE._packed is known
to the checker with its master weight, column slice, transpose flag and -- in eval mode -- the product's own checked
bn_eval_params scale; and every parameter gradient must be the output of a checked call, or one of the views, slices
and concatenations Recorder.grad_orphans admits.  Three rules tie calls together: dattn_ext must be the sum of the dattn
of every temporal_aggregate_bwd call, a bias gradient counts only as the column sums of a tensor that a conv_wgrad call
of the same node read, and the weight gradient of a ConvTranspose2d must take the node's output gradient as its x.

What one MI355X run of this module measured: the largest error as a fraction of its bound, per op and output, over all
cases of the storage type (the tables of tests/test_temporal_kernels_gpu.py give the same kernels on their own).
  op (family)              output          fp32 storage  bf16 storage
  reflect_pad1             padded copy     exact         exact
  reflect_pad1_bwd         dx              0.0089        0.499
  group_norm               y               0.0082        0.498
  group_norm_bwd           dx              0.0094        0.498
                           dgamma          0.0031        0.0035
                           dbeta           0.0065        0.00086
  group_norm_seq           y               0.0079        0.498
  group_norm_seq_bwd       dx              0.0088        0.498
                           dgamma          0.0033        0.0039
                           dbeta           0.0038        0.00090
  positional_encoding      encoding        0.0060        (f32 only)
  add_rowvec_              x + vec         0.0039        0.499
  detect_pad_images        pad flags       exact         (f32 only)
  mask_images_             masked copy     exact         exact
  mul                      x * m           0.0039        0.499
  ltae_attention           out             0.0042        0.497
                           attn            0.0056        0.0059
  ltae_attention_train     out             0.0048        0.497
                           attn            0.0066        0.0088
                           prob            0.0058        0.0064
  ltae_attention_bwd       dk              0.0067        0.496
                           dv              0.0075        0.499
                           dQ              0.00019       0.00017
                           dattn_ext       0.333         0.333      (= the sum of the aggregators' dattn)
  temporal_aggregate       out             0.0092        0.499
  temporal_aggregate_bwd   dx              0.0039        0.499
                           dattn           0.0100        0.0074
  column_sums              column sums     0.0091        0.0044
  conv2d, forward operand  out             0.026         0.498      (utae_fwd: sliced pairs and folded operands too)
  conv2d, ConvTranspose2d  out             0.018         0.497      (utae_conv_transpose)
  conv2d, input gradient   dx              0.056         0.498      (utae_dgrad: out_hw calls, sliced pairs, 1x1)
  conv_wgrad               dW              0.037         0.025
  HipUTAE._packed          bias vector     0.499         0.499      (eval mode: shift + scale * bias within 2 ulp_f32)
The bf16-stored outputs sit at one half of their bound because the bound's first term is one bf16 ulp and round to
nearest errs by half of it; what the f32 arithmetic adds stays, as in the f32 column, below 0.06 of REL * a.  No kernel
was found to round an intermediate to bf16, so no 2^-8 term appears in any bound.

No bound was moved and no product defect was found.  Two defects of the checker itself were mended in tests/insitu.py:
the record of a rescaled dlogits buffer was matched by address against a later, unrelated conv input once the buffer
had been consumed by a BatchNorm backward (the U-TAE's class-score layer) and freed, which failed three fp32 cases on
the first run; and bn_bwd would have counted the zero pad channels of that layer (dy = 0, where the mask decides
nothing) as open ReLU masks.

Tried by hand, not committed: _Aggregate.backward returning None for dattn fails every training case here at
"dattn_ext = sum of the aggregators' dattn"; _bias_grad(dy) in place of _bias_grad(d0) in _ConvGN.backward fails every
training case at the gradient-source rule (column sums of a tensor no conv_wgrad call of the node read).
"""
import json
import os
import time

import pytest
import torch

from helpers import MOD, ROOT, TASK
from insitu import Recorder
from test_insitu_gpu import _assert_default_switches
from test_oracle_goldens import _utae_state_shapes
from test_utae_gpu import PARAMS

pytestmark = pytest.mark.gpu

S2, S2_DATES = "SENTINEL2_TS", "SENTINEL2_DATES"
TRAIN_OPS = {"reflect_pad1", "reflect_pad1_bwd", "group_norm", "group_norm_bwd", "group_norm_seq", "group_norm_seq_bwd",
             "positional_encoding", "add_rowvec_", "detect_pad_images", "mask_images_", "mul", "ltae_attention_train",
             "ltae_attention_bwd", "temporal_aggregate", "temporal_aggregate_bwd", "column_sums"}
EVAL_OPS = {"reflect_pad1", "group_norm", "group_norm_seq", "positional_encoding", "add_rowvec_", "detect_pad_images",
            "mask_images_", "ltae_attention", "temporal_aggregate"}
ALL_OPS = TRAIN_OPS | EVAL_OPS
# B, T, H, W, padded dates of sample 0, flip / rotation codes
CASES = {"10x10": (2, 4, 10, 10, 2, None), "5x7": (2, 4, 5, 7, 2, None), "T1": (2, 1, 10, 10, 0, None),
         "aug": (2, 4, 10, 10, 2, [5, 2])}
CASE = pytest.mark.parametrize("case", sorted(CASES))
PRECISION = pytest.mark.parametrize("precision", ["bf16", "fp32"])

# The BatchNorm layers of the decoder see 2 x 10 x 10 x 32 = 6400 values or fewer, where the cap on ReLU masks the
# reference leaves open (AMBIG_MAX_FRACTION = 1e-4 of the elements) admits not one: the seed is one at which no
# pre-activation with a non-zero gradient lies within AMBIG_REL of zero in any case, decided on the float64 side alone
# (as GN2D_SEED of tests/test_temporal_kernels_gpu.py).  The run is reproducible: every kernel sums in a fixed order.
TRAIN_SEED = 63
FUSED_SEED = 73

_seen = set()      # ops names counted by the recorders of this module
_measured = {}     # (op, what, storage) -> worst error / bound


def _model(precision):
    from flairhip.utae import HipUTAE
    from oracle.seeded_weights import fill_utae_state_dict
    net = HipUTAE(10, precision=precision, **PARAMS)
    net.load_state_dict(fill_utae_state_dict({k: torch.zeros(s) for k, s in _utae_state_shapes().items()}))
    assert (net.mlp_dropout, net.attn_dropout) == (0.2, 0.1)
    return net.cuda()


def _inputs(case, seed):
    B, T, H, W, npad, codes = CASES[case]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, 10, H, W, generator=g)
    if npad:
        x[0, T - npad:] = float(PARAMS["pad_value"])   # sample 0 loses its last dates, sample 1 keeps all
    pos = torch.sort(torch.randint(0, 365, (B, T), generator=g), dim=1).values.float()
    target = torch.randint(0, 19, (B, H, W), generator=g)
    aug = None if codes is None else torch.tensor(codes, dtype=torch.uint8).cuda()
    return x.cuda(), pos.cuda(), target.cuda(), aug


def _note(rec, storage):
    _seen.update(rec.counts)
    for r in rec.results:
        key = (r.get("family", r["op"]), r["what"], storage)
        _measured[key] = max(_measured.get(key, 0.0), r["worst"])


def _report(rec, t0):
    print(f"\n{rec.table()}\nchecked calls: {len(rec.calls)}; wall time {time.perf_counter() - t0:.1f} s")
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    fails = rec.failures()
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])


def _assert_conv_forms(rec, training):
    """the recorded conv calls include the forms that are this model's own"""
    convs = [c for c in rec.calls if c.get("utae")]
    assert convs and all(c["layout"] == "igemm" for c in convs)
    assert any(c["family"] == "utae_conv_transpose" and c["kernel"] == "3x3" and c["bias"] for c in convs)
    pair = [c for c in convs if c["sliced"] and c["family"] == "utae_fwd"]
    assert any(c["residual"] and c["cols"][0] > 0 for c in pair) and any(not c["residual"] and c["cols"][0] == 0 for c in pair)
    assert all(c["folded"] != training for c in convs if c["family"] == "utae_fwd" and c["tag"] != "inconv" and
               c["tag"] != "fc1_k" and not c["tag"].startswith(("in", "d")))
    if training:
        assert any(c["out_hw"] and c["family"] == "utae_dgrad" and c["kernel"] == "3x3" for c in convs)
        assert any(c["sliced"] and c["family"] == "utae_dgrad" for c in convs)
        assert any(c["family"] == "utae_dgrad" and c["kernel"] == "1x1" for c in convs)


def _train_step(net, crit, x, pos, target, aug):
    from flairhip import nn as hnn
    logits_nhwc, _, _ = net.forward_nhwc(x, pos, aug=aug)
    loss = crit(hnn.logits_view(logits_nhwc, 19), target)
    loss.backward()
    return loss


def _checked_training_step(case, precision, seed):
    """step 1 eager, then the product's optimizer (the operands are re-packed), step 2 recorded -> (net, recorder, aug)"""
    from flairhip import nn as hnn
    from flairhip.optim import HipAdamW
    torch.manual_seed(seed)   # the dropout masks are drawn on the device
    net = _model(precision).train()
    crit = hnn.HipCrossEntropyLoss(num_classes=19).cuda()
    opt = HipAdamW(net.parameters(), lr=1e-3)
    x, pos, target, aug = _inputs(case, seed)
    _train_step(net, crit, x, pos, target, aug)
    opt.step()
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    with Recorder(net, mode="full", chunk=2) as rec:
        _train_step(net, crit, x, pos, target, aug)
        torch.cuda.synchronize()
    return net, rec, aug


@PRECISION
@CASE
def test_every_kernel_call_of_the_utae_training_step_matches_float64(cuda, case, precision):
    t0 = time.perf_counter()
    _assert_default_switches()
    net, rec, aug = _checked_training_step(case, precision, TRAIN_SEED)
    named = list(net.named_parameters())
    orphans = rec.grad_orphans(named)
    _note(rec, precision)
    _report(rec, t0)
    assert not orphans, f"gradients not produced by a checked call: {orphans[:10]}"
    without = [k for k, p in named if p.grad is None]
    assert not without, f"parameters without a gradient: {without[:10]}"
    missing = TRAIN_OPS - set(rec.counts)
    assert not missing, f"the training step no longer reaches {sorted(missing)}"
    _assert_conv_forms(rec, training=True)
    T = CASES[case][1]
    assert {c["T"] for c in rec.calls if c["op"] == "group_norm_seq"} == {1, T}
    bwd = [c for c in rec.calls if c["op"] == "ltae_attention_bwd"]
    assert len(bwd) == 1 and bwd[0]["drop"] and bwd[0]["dattn_ext"] and bwd[0]["T"] == T and bwd[0]["aggregators"] == 3
    assert sum(1 for c in rec.calls if c["op"] == "mul") == 2 and sum(1 for c in rec.calls if c["op"] == "mask_images_") == 8
    assert sum(1 for c in rec.calls if c.get("conv_transpose")) == len(net.up_blocks) == 3  # their wgrads, roles checked
    layouts = [c for c in rec.calls if c["op"] == "d4_layout"]
    assert len(layouts) == (0 if aug is None else 1) and all(c["codes"] == sorted(CASES[case][5]) for c in layouts)


@PRECISION
@CASE
def test_every_kernel_call_of_the_utae_evaluation_forward_matches_float64(cuda, case, precision):
    t0 = time.perf_counter()
    _assert_default_switches()
    net = _model(precision).eval()
    x, pos, _, aug = _inputs(case, seed=67)
    with torch.no_grad(), Recorder(net, mode="full", chunk=2) as rec:
        if aug is None:
            logits, maps = net(x, batch_positions=pos)   # the return_maps path: every decoder map goes back to NCHW
            assert logits.shape == (x.shape[0], 19) + tuple(x.shape[-2:]) and len(maps) == 4
        else:
            net.forward_nhwc(x, pos, aug=aug)
        torch.cuda.synchronize()
    _note(rec, precision)
    _report(rec, t0)
    missing = EVAL_OPS - set(rec.counts)
    assert not missing, f"the evaluation forward no longer reaches {sorted(missing)}"
    assert not (set(rec.counts) & (TRAIN_OPS - EVAL_OPS))
    _assert_conv_forms(rec, training=False)
    assert rec.counts["bn_eval_params"] >= 12 and (rec.counts["nhwc_to_nchw"] == 5) == (aug is None)


def test_every_kernel_call_of_the_aerial_plus_sentinel_training_step_matches_float64(cuda):
    """FLAIR_HUB_Model with AERIAL_RGBI + SENTINEL2_TS in bf16: the U-TAE maps go through the per-stage fusion and back.
    Aerial 64 x 64 at B = 4 leaves the deepest BatchNorms 2 x 2 x 4 = 16 values per channel."""
    from flairhip.configs import unet_resnet34_config
    from flairhip.optim import HipAdamW
    from flair_hub.tasks.module_setup import build_segmentation_module
    from test_sentinel_gpu import _fill
    t0 = time.perf_counter()
    _assert_default_switches()
    cfg = unet_resnet34_config(in_channels=5, precision="bf16")
    cfg["modalities"]["inputs"][S2] = True
    cfg["modalities"]["inputs_channels"][S2] = list(range(1, 11))
    task = build_segmentation_module(cfg, {MOD: 64, S2: 10}, "train")
    task.model.load_state_dict(_fill(task.model.state_dict()))
    task = task.cuda().train()
    utae = task.model.encoders[S2]
    assert (utae.mlp_dropout, utae.attn_dropout) == (0.2, 0.1)
    B, T = 4, 3
    torch.manual_seed(FUSED_SEED)   # the dropout masks are drawn on the device
    g = torch.Generator().manual_seed(FUSED_SEED)
    s2 = torch.randn(B, T, 10, 10, 10, generator=g)
    s2[1, T - 1] = 0.0                                         # one padded date
    batch = {MOD: torch.randn(B, 5, 64, 64, generator=g).cuda(), S2: s2.cuda(),
             S2_DATES: torch.sort(torch.randint(0, 365, (B, T), generator=g), dim=1).values.float().cuda(),
             TASK: torch.randint(0, 19, (B, 64, 64), generator=g).to(torch.uint8).cuda()}
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    assert isinstance(opt, HipAdamW), type(opt)
    loss, _, _ = task.step(batch, training=True)
    loss.backward()
    opt.step()
    del loss
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    with Recorder(task.model, mode="full", chunk=2) as rec:
        loss, _, _ = task.step(batch, training=True)
        loss.backward()
        torch.cuda.synchronize()
    named = list(task.model.named_parameters())
    orphans = rec.grad_orphans(named)
    _note(rec, "bf16")
    _report(rec, t0)
    assert not orphans, f"gradients not produced by a checked call: {orphans[:10]}"
    missing = TRAIN_OPS - set(rec.counts)
    assert not missing, f"the fused training step no longer reaches {sorted(missing)}"
    _assert_conv_forms(rec, training=True)
    # the class scores of the U-TAE never reach the loss of the fused model: the reference's own list of parameters
    # without a gradient (tests/golden/sentinel.json, s2_train)
    info = json.load(open(os.path.join(ROOT, "tests", "golden", "sentinel.json")))["s2_train"]
    assert sorted(k for k, p in named if p.grad is None) == info["unused_parameters"]
    assert any(c.get("fusion") for c in rec.calls)
    bwd = [c for c in rec.calls if c["op"] == "ltae_attention_bwd"]
    assert len(bwd) == 1 and bwd[0]["dattn_ext"] and bwd[0]["aggregators"] == len(utae.up_blocks) == 5


def test_the_cases_of_this_module_reach_every_temporal_op(cuda):
    """last: the union of what the recorders above counted, so that a refactor that drops an op from the step is noticed"""
    rows = {}
    for (op, what, storage), worst in _measured.items():
        rows.setdefault((op, what), {})[storage] = worst
    print("\n  op / family                output                      fp32 storage   bf16 storage")
    for (op, what), v in sorted(rows.items()):
        cells = "".join(f"{v[s]:15.3g}" if s in v else f"{'-':>15}" for s in ("fp32", "bf16"))
        print(f"  {op:26s} {what[:26]:26s}{cells}")
    missing = ALL_OPS - _seen
    assert not missing, f"no case of this module reached {sorted(missing)}"
