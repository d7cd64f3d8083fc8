"""Every kernel call of the bf16 training step, checked in situ against float64 (tests/insitu.py).

The benchmarked program (bf16 U-Net at 512 x 512) runs on kernels the fp32 model tests never reach, at grid caps,
tile walks and re-packed operands the per-kernel tests never see.  Here the real step runs under a Recorder: every
flairhip.ops call is compared with a float64 evaluation of the same operation on the call's own inputs, so a wrong
tile, channel block or dropped partial shows up where it happens instead of drowning in the bf16 avalanche of a
whole-model comparison.  The optimizer step is no ops function and the recorder does not see it: the eager step that
precedes the recorded one snapshots p, g, exp_avg, exp_avg_sq, step and lr around HipAdamW.step() and holds every tensor to
the float64 update (Checker.adamw); those results join the table (family "adamw") and the assertions.
"""
import os
import time

import pytest
import torch

from helpers import MOD, TASK, make_pair
from insitu import Checker, Recorder

pytestmark = pytest.mark.gpu

TILE, CLASSES = 512, 19
# library switches read at launch time, and the Python-side ones: bench.py runs with none of them set
GRID_CAPS = ("FFA_RING_GRID", "FFA_THIN_GRID", "FFA_STEM_GRID")
REQUIRED_FAMILIES = {
    "fwd:ring16", "fwd:thin", "fwd:stem", "upcat_fwd", "upcat_dgrad", "upcat_wgrad", "dgrad_dil2",
    "dgrad_residual", "maxpool_bwd_add",
}


def _batch(n, seed, hw=(TILE, TILE)):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 5, *hw, generator=g)
    t = torch.randint(0, CLASSES, (n, *hw), generator=g).to(torch.uint8)
    return {MOD: x.cuda(), TASK: t.cuda()}


def _switches():
    from flairhip import ops, unet
    py = {"FUSED_BN_STATS": ops.FUSED_BN_STATS, "FUSED_UPCAT": ops.FUSED_UPCAT, "FUSED_UPCAT_BWD": ops.FUSED_UPCAT_BWD,
          "NORM_ON_LOAD": ops.NORM_ON_LOAD, "FUSED_BN_BWD": ops.FUSED_BN_BWD, "FUSED_BN_BWD_COOP": ops.FUSED_BN_BWD_COOP,
          "FUSED_FORKS": unet.FUSED_FORKS}
    env = {k: v for k, v in os.environ.items() if k.startswith("FFA_")}
    return py, env


def _assert_default_switches(allowed_env=()):
    py, env = _switches()
    print(f"switches: {py}; FFA_* environment: {env or 'none'}")
    assert py == {"FUSED_BN_STATS": True, "FUSED_UPCAT": True, "FUSED_UPCAT_BWD": True, "NORM_ON_LOAD": False,
                  "FUSED_BN_BWD": False, "FUSED_BN_BWD_COOP": False, "FUSED_FORKS": True}, py
    extra = {k: v for k, v in env.items() if k not in allowed_env}
    assert not extra, f"FFA_* switches set that bench.py does not run with: {extra}"


def _families(rec):
    fams = set()
    for c in rec.calls:
        f = c.get("family", c["op"])
        fams.add(f)
        if f == "fwd":
            fams.add(f"fwd:{c['layout']}")
        if f.startswith("dgrad"):
            if c.get("dil") == 2:
                fams.add("dgrad_dil2")
            if c.get("residual"):
                fams.add("dgrad_residual")
    return fams


def _checked_step(B, mode, seed, chunk, precision="bf16", hw=(TILE, TILE)):
    """step 1 eager with the product's own optimizer (operands re-packed by the batched packers afterwards), step 2
    recorded and checked -> (task, recorder, loss)"""
    from flairhip.optim import HipAdamW
    task, _, _ = make_pair(precision=precision)
    task.train()
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    assert isinstance(opt, HipAdamW), type(opt)
    batch = _batch(B, seed, hw)
    loss = task.training_step(batch, 0)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    adam = _checked_optimizer_step(task, opt)
    del loss
    opt.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    with Recorder(task.model, mode=mode, chunk=chunk) as rec:
        loss = task.training_step(batch, 1)
        loss.backward()
        torch.cuda.synchronize()
    rec.results.extend(adam.results)  # the optimizer is no ops function: its checks join the table and the assertions here
    return task, rec, loss


def _checked_optimizer_step(task, opt):
    """opt.step() of the product's HipAdamW on the step's own gradients, every tensor against float64 (Checker.adamw):
    p, g, exp_avg, exp_avg_sq, step and lr snapshotted around the call -> the checker holding the results"""
    names = {id(p): n for n, p in task.model.named_parameters()}
    before = []
    for gi, grp in enumerate(opt.param_groups):
        for p in grp["params"]:
            if p.grad is None:
                continue
            st = opt.state.get(p, {})
            before.append((gi, p, p.detach().clone(), p.grad.detach().clone(),
                           st["exp_avg"].clone() if st else torch.zeros_like(p),
                           st["exp_avg_sq"].clone() if st else torch.zeros_like(p)))
    opt.step()
    torch.cuda.synchronize()
    ck = Checker("full")
    for i, (gi, p, p0, g0, m0, v0) in enumerate(before):
        grp, st = opt.param_groups[gi], opt.state[p]
        ck.adamw({"op": "adamw", "family": "adamw", "call": f"adamw:{i}", "module": names.get(id(p), "?")}, p0, g0, m0, v0,
                 st["step"], grp["lr"], p, st["exp_avg"], st["exp_avg_sq"], grp["betas"], grp["eps"], grp["weight_decay"],
                 opt.decoupled, grp["maximize"])
    assert len(ck.results) == 3 * len(before) > 0
    return ck


def _report_and_assert(task, rec, t0, required=REQUIRED_FAMILIES):
    print(f"\n{rec.table()}\nchecked calls: {len(rec.calls)}; wall time {time.perf_counter() - t0:.1f} s")
    fails = rec.failures()
    assert not rec.unchecked, f"kernel-launching ops calls without a reference: {dict(rec.unchecked)}"
    assert not fails, f"{len(fails)} checks failed:\n" + "\n".join(r.line() for r in fails[:40])
    # (b) coverage of the kernel families the step is expected to route through
    missing = set(required) - _families(rec)
    assert not missing, f"the step no longer reaches {sorted(missing)} (routing moved: update the list and the checks)"
    # (c) every parameter gradient IS the output of a checked call (bit for bit)
    srcs = {}
    for tag, t in rec.grad_sources:
        srcs.setdefault(tuple(t.shape), []).append(t)
    orphans = []
    for name, p in task.model.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach()
        if not any(torch.equal(g, t) for t in srcs.get(tuple(g.shape), [])):
            orphans.append(name)
    assert not orphans, f"gradients not produced by a checked call: {orphans[:10]}"


def test_every_kernel_of_the_bf16_step_at_2x512_matches_float64(cuda):
    t0 = time.perf_counter()
    _assert_default_switches()
    task, rec, _ = _checked_step(2, "full", seed=31, chunk=1)
    _report_and_assert(task, rec, t0)


def test_every_kernel_of_the_bf16_step_at_2x512_with_low_grid_caps_matches_float64(cuda, monkeypatch):
    """at B = 2 the default caps leave the small layers at about one tile per block: forced caps make every ring, thin
    and stem launch walk many tiles, ragged ends included"""
    t0 = time.perf_counter()
    for k in GRID_CAPS:
        monkeypatch.setenv(k, "8")
    _assert_default_switches(allowed_env=GRID_CAPS)
    task, rec, _ = _checked_step(2, "full", seed=37, chunk=1)
    _report_and_assert(task, rec, t0)


def test_every_kernel_of_the_bf16_step_at_3x96x160_matches_float64(cuda):
    """non-square, odd batch: the maps are 48 x 80, 24 x 40, 12 x 20, 6 x 10 and 3 x 5, so every ring16, thin, stem and
    weight-gradient launch has ragged tiles and the deepest levels are smaller than one tile (the fp32 step has this
    case in tests/test_insitu_fp32_gpu.py; at 512 x 512 every map is a power of two and every tile is full)"""
    t0 = time.perf_counter()
    _assert_default_switches()
    task, rec, _ = _checked_step(3, "full", seed=43, chunk=1, hw=(96, 160))
    _report_and_assert(task, rec, t0)


def test_every_kernel_of_the_bf16_step_at_32x512_matches_float64_projected(cuda):
    t0 = time.perf_counter()
    _assert_default_switches()
    task, rec, _ = _checked_step(32, "proj", seed=41, chunk=4)
    _report_and_assert(task, rec, t0)


def test_graph_replay_at_32x512_equals_the_checked_eager_step(cuda):
    """GraphedTrainStep (what bench.py times) replays the same batch from the same state with the loss and parameter
    gradients of the eager step, bit for bit: the in-situ checks of the eager step speak for the replay"""
    from flairhip import nn as hnn
    from flairhip.graph import GraphedTrainStep
    t0 = time.perf_counter()
    _assert_default_switches()
    task, _, _ = make_pair(precision="bf16")
    task.train()
    opt = task.configure_optimizers()
    opt = opt["optimizer"] if isinstance(opt, dict) else opt
    batch = _batch(32, seed=41)
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
    print(f"\ngraph replay vs eager at 32 x 512: loss {loss_g.item():.6f} / {loss_e.item():.6f}, "
          f"{len(grads_e)} gradients; wall time {time.perf_counter() - t0:.1f} s")
    assert torch.equal(loss_g.reshape(()), loss_e.detach().reshape(()))
    assert grads_g.keys() == grads_e.keys() and len(grads_e) > 100
    diff = [n for n in grads_e if not torch.equal(grads_g[n], grads_e[n])]
    assert not diff, f"{len(diff)} gradients differ between replay and eager step, e.g. {diff[:5]}"
