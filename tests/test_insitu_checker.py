"""Power of the in-situ comparator (tests/insitu.py), without a GPU.

"Product" outputs are made with torch at small shapes: f32 arithmetic in another summation order than the float64
references, rounded to bf16 where the kernels store bf16.  In both modes (elementwise and projected) the comparator
must pass these honest results and flag each planted fault that applies to the mode -- the subtle ways a kernel of the
training step goes wrong in situ: a halo shift of one tile, a channel block with its neighbour's weights, a dropped
split-K partial, a lost tile of a BatchNorm reduction, swapped parity planes of a stride-2 dgrad, a nonzero pad
channel, a max-pool gradient routed to the wrong tap, a biased running variance.

The same calls are made with f32 tensors for the fp32 programs, whose rounding unit is ulp_f32: there a bf16 operand, a
bf16 detour of an output, one dropped channel group of one tap, a lost statistics tile, BatchNorm-backward sums from
bf16-rounded gradients and a one-tap shift of the resize must be flagged as well, and one test recomputes the rule
that was applied to every activation before (ulp_bf16) to show what it let through.

The references of the eval step (zonal inference) follow at the end of the file, with the ways that path goes wrong: a
BatchNorm scale folded along the wrong axis or in another precision than the packer's, a shift left out, a residual
added after the ReLU, a zeroed row of a ragged tile, the higher label at an exact tie, a band off by one, a crop origin
off by one, a quarter-turn view taken back with the forward code, a first view added where it should overwrite, a view
count off by one.

Last, the optimizer (Checker.adamw): an f32 emulation of ffa_adamw_multi must sit inside the bound at steps 1 .. 1e5 and
gradient scales 1e-9 .. 10, and seven mutants must fail it: no bias correction of v or of m, beta1 as the lerp weight,
decoupled and L2 decay exchanged, eps inside the square root, maximize ignored, another tensor's step count.
"""
import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import insitu
from insitu import Checker

B, H, W = 2, 32, 48
CI, CO, CO_PITCH, C2 = 48, 72, 80, 64  # stride-1 layer 48 -> 72 (stored pitch 80), stride-2 layer 48 -> 64
MOM, EPS = 0.1, 1e-5


def _bf(t):
    return t.to(torch.bfloat16).float()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _store(t_nchw, pitch=None, dtype=torch.bfloat16):
    """f32 NCHW result -> NHWC tensor stored as `dtype` (pad channels zero)"""
    o = _nhwc(t_nchw).to(dtype)
    if pitch is not None and pitch > o.shape[-1]:
        o = F.pad(o, (0, pitch - o.shape[-1]))
    return o


def _build_case(seed, dt):
    """the calls of one layer with activations stored as `dt`: bf16 values throughout for torch.bfloat16 (the bf16
    step), plain f32 values -- weights, activations and gradients -- for torch.float32 (the fp32 step)"""
    g = torch.Generator().manual_seed(seed)
    c = {"dt": dt}
    q = _bf if dt == torch.bfloat16 else (lambda t: t)
    x = q(torch.randn(B, CI, H, W, generator=g))
    w1 = q(torch.randn(CO, CI, 3, 3, generator=g) / 20)
    w2 = q(torch.randn(C2, CI, 3, 3, generator=g) / 20)
    c.update(x=x, w1=w1, w2=w2)
    # stride-1 forward (pitch 80 for 72 real channels)
    c["y1"] = _store(F.conv2d(x, w1, padding=1), CO_PITCH, dt)
    # stride-2 forward + BatchNorm statistics of its stored output
    y0 = _store(F.conv2d(x, w2, stride=2, padding=1), None, dt)
    v = y0.float().reshape(-1, C2)
    n = v.shape[0]
    mean, var = v.mean(0), v.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    gamma = torch.rand(C2, generator=g) * 0.5 + 0.75
    beta = torch.randn(C2, generator=g) * 0.1
    rm0, rv0 = torch.randn(C2, generator=g) * 0.1, torch.rand(C2, generator=g) + 0.5
    scale = gamma * rstd
    shift = beta - mean * scale
    c.update(y0=y0, gamma=gamma, beta=beta, rm0=rm0, rv0=rv0, mean=mean, rstd=rstd, scale=scale, shift=shift,
             rm1=(1 - MOM) * rm0 + MOM * mean, rv1=(1 - MOM) * rv0 + MOM * var * n / (n - 1), var=var, n=n)
    # BatchNorm + ReLU backward, mask recomputed from the pre-activation (mode 2)
    dy = q(torch.randn(B, H // 2, W // 2, C2, generator=g) * 0.1).to(dt)
    xf = y0.float()
    gm = torch.where(xf * scale + shift > 0, dy.float(), torch.zeros(()))
    xh = (xf - mean) * rstd
    dbeta = gm.reshape(-1, C2).sum(0)
    dgamma = (gm * xh).reshape(-1, C2).sum(0)
    dx = (gamma * rstd * (gm - dbeta / n - xh * dgamma / n)).to(dt)
    c.update(bdy=dy, bdx=dx, dgamma=dgamma, dbeta=dbeta, gm=gm, xh=xh)
    # stride-2 dgrad (the zero-insertion call) and stride-1 weight gradient
    d2 = q(torch.randn(B, C2, H // 2, W // 2, generator=g) * 0.1)
    c.update(d2=_nhwc(d2).to(dt), dx2=_store(conv2d_input((B, CI, H, W), w2, d2, stride=2, padding=1), None, dt))
    d1 = q(torch.randn(B, CO, H, W, generator=g) * 0.1)
    c.update(d1=F.pad(_nhwc(d1), (0, CO_PITCH - CO)).to(dt),
             dw1=conv2d_weight(x, w1.shape, d1, padding=1), d1_nchw=d1)
    # max-pool 3x3 s2 p1 forward (first maximal tap in row-major order) and backward with an `add` input
    xp = torch.randn(B, H, W, 32, generator=g).to(dt)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    pad = F.pad(xp.float(), (0, 0, 1, 1, 1, 1), value=float("-inf"))
    taps = torch.stack([pad[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r in range(3) for s in range(3)])
    best = taps.max(0).values
    idx = torch.argmax((taps == best).to(torch.int8), dim=0).to(torch.uint8)
    pdy = torch.randn(B, Ho, Wo, 32, generator=g).to(dt)
    add = torch.randn(B, H, W, 32, generator=g).to(dt)
    c.update(px=xp, pidx=idx, pdy=pdy, padd=add, pdx=_route(pdy, idx, add, H, W).to(dt))
    return c


@pytest.fixture(scope="module")
def case():
    return _build_case(5, torch.bfloat16)


@pytest.fixture(scope="module")
def case32():
    return _build_case(35, torch.float32)


def _route(dy, idx, add, H, W):
    """the routed gradient sums + add, in f32 (the caller rounds them to the stored type)"""
    Bn, Ho, Wo, C = dy.shape
    acc = torch.zeros(Bn, 2 * Ho + 1, 2 * Wo + 1, C)
    for t in range(9):
        r, s = divmod(t, 3)
        acc[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += torch.where(idx == t, dy.float(), torch.zeros(()))
    return acc[:, 1:1 + H, 1:1 + W] + add.float()


def _f64(t):
    return t.to(torch.float64)


# --------------------------------------------------------------------------------------------------
# one entry per checked kernel call: run(checker, case, fault) -> results of that call

def run_fwd(ck, c, fault):
    dt = c["dt"]
    y = c["y1"].clone()
    if fault == "halo":  # one 16x16 tile of the last image read one pixel off
        ys = _store(F.conv2d(torch.roll(c["x"], 1, dims=3), c["w1"], padding=1), CO_PITCH, dt)
        y[-1, 16:32, 16:32] = ys[-1, 16:32, 16:32]
    elif fault == "channel_block":  # output channels 16..31 computed with the weights of 32..47
        w = c["w1"].clone()
        w[16:32] = w[32:48]
        y[..., 16:32] = _store(F.conv2d(c["x"], w, padding=1), CO_PITCH, dt)[..., 16:32]
    elif fault == "pad_channel":
        y[0, 3, 5, CO + 3] = 1e-3
    elif fault == "out_bf16":  # f32 in name only: the result takes a detour through bf16
        y = _bf(y)
    elif fault == "w_bf16":  # f32 in name only: the operand was packed as bf16
        y = _store(F.conv2d(c["x"], _bf(c["w1"]), padding=1), CO_PITCH, dt)
    elif fault == "tap_group":  # last row of the ragged tile (columns 32..47 of 48) of the last image: the 8 input
        wz = torch.zeros_like(c["w1"])  # channels 8..15 of tap (0, 2) never reach the sum
        wz[:, 8:16, 0, 2] = c["w1"][:, 8:16, 0, 2]
        y[-1, H - 1, 32:, :CO] -= _nhwc(F.conv2d(c["x"], wz, padding=1))[-1, H - 1, 32:].to(dt)
    ck.conv_forward({"op": "conv2d"}, _nhwc(c["x"]).to(dt), _f64(c["w1"]), 1, 1, y)


def run_dgrad_s2(ck, c, fault):
    dx = c["dx2"].clone()
    if fault == "parity":  # even and odd rows of the zero-insertion dgrad exchanged
        dx = torch.stack([dx[:, 1::2], dx[:, 0::2]], dim=2).reshape(dx.shape)
    ck.conv_dgrad({"op": "conv2d"}, c["d2"], _f64(c["w2"]), 2, 1, dx)


def run_wgrad(ck, c, fault):
    dw = c["dw1"].clone()
    if fault == "split_k":  # image 1 (one split-K slab) missing from one 16 x 16 (out x in) channel block
        part = conv2d_weight(c["x"][1:], c["w1"].shape, c["d1_nchw"][1:], padding=1)
        dw[0:16, 16:32] -= part[0:16, 16:32]
    ck.conv_wgrad({"op": "conv_wgrad"}, _nhwc(c["x"]).to(c["dt"]), c["d1"], 3, 3, 1, 1, dw)


def run_bn_stats(ck, c, fault):
    k = dict(c)
    if fault == "biased_var":
        k["rv1"] = (1 - MOM) * c["rv0"] + MOM * c["var"]
    elif fault == "lost_tile":  # channel 5: the partial sums of one 16 x 16 tile never reach the reduction
        v, t = c["y0"].float()[..., 5], c["y0"].float()[0, 0:16, 0:16, 5]
        n = c["n"]
        mean, var = c["mean"].clone(), c["var"].clone()
        mean[5] = (v.sum() - t.sum()) / n
        var[5] = ((v * v).sum() - (t * t).sum()) / n - mean[5] ** 2
        rstd = 1.0 / torch.sqrt(var + EPS)
        scale = c["gamma"] * rstd
        k.update(mean=mean, rstd=rstd, scale=scale, shift=c["beta"] - mean * scale,
                 rm1=(1 - MOM) * c["rm0"] + MOM * mean, rv1=(1 - MOM) * c["rv0"] + MOM * var * n / (n - 1))
    ck.bn_stats({"op": "conv2d_bn_stats"}, c["y0"], c["gamma"], c["beta"], c["rm0"], c["rv0"], k["rm1"], k["rv1"], MOM,
                EPS, k["scale"], k["shift"], k["mean"], k["rstd"])


def run_bn_bwd(ck, c, fault):
    dgamma, dx = c["dgamma"].clone(), c["bdx"]
    if fault == "dgamma_tile":  # channel 5 misses the partial sum of one 16 x 16 tile
        dgamma[5] -= (c["gm"][0, 0:16, 0:16, 5] * c["xh"][0, 0:16, 0:16, 5]).sum()
    elif fault == "dbeta_from_bf16":  # the sums inside dx taken from bf16-rounded dy; the dbeta handed out is the honest one
        low = _bf(c["gm"]).reshape(-1, C2).sum(0)
        dx = (c["gamma"] * c["rstd"] * (c["gm"] - low / c["n"] - c["xh"] * c["dgamma"] / c["n"])).to(c["dt"])
    ck.bn_bwd({"op": "bn_bwd"}, c["y0"], c["bdy"], None, c["gamma"], c["beta"], c["mean"], c["rstd"], True, dx,
              None, dgamma, c["dbeta"])


def run_maxpool_bwd(ck, c, fault):
    dx = c["pdx"]
    if fault == "route":  # one pixel's gradient sent to another tap of its window
        idx = c["pidx"].clone()
        idx[1, 5, 7, 3] = (int(idx[1, 5, 7, 3]) + 4) % 9
        dx = _route(c["pdy"], idx, c["padd"], H, W).to(c["dt"])
    elif fault == "sum_bf16":  # the gradient sum rounded to bf16 on its way to an f32 tensor
        dx = _bf(dx)
    ck.maxpool_bwd({"op": "maxpool3x3s2_bwd"}, c["pdy"], c["pidx"], (H, W), c["padd"], dx)


CALLS = {"fwd": run_fwd, "dgrad_s2": run_dgrad_s2, "wgrad": run_wgrad, "bn_stats": run_bn_stats, "bn_bwd": run_bn_bwd,
         "maxpool_bwd": run_maxpool_bwd}
# fault -> (call it lives in, modes it applies to)
FAULTS = {
    "halo": ("fwd", ("full", "proj")),
    "channel_block": ("fwd", ("full", "proj")),
    "split_k": ("wgrad", ("full", "proj")),
    "dgamma_tile": ("bn_bwd", ("full", "proj")),
    "parity": ("dgrad_s2", ("full", "proj")),
    "pad_channel": ("fwd", ("full", "proj")),
    "route": ("maxpool_bwd", ("full",)),
    "biased_var": ("bn_stats", ("full", "proj")),
}
# what only the f32 bounds can see (for bf16 tensors the first, second and fifth ARE the honest result), and two more
# that the bf16 cases do not plant.  A projection sums the independent roundings of the channels: they grow with the
# root of the channel count, the bound with the count itself, so the margin over the two bf16 detours of a forward conv
# shrinks as the layers widen: those two are asserted for the elementwise mode, which the fp32 GPU cases run in.  The
# projected mode is asserted on the faults that are whole terms of the sum.
F32_FAULTS = {
    "out_bf16": ("fwd", ("full",)),
    "w_bf16": ("fwd", ("full",)),
    "tap_group": ("fwd", ("full", "proj")),
    "lost_tile": ("bn_stats", ("full", "proj")),
    "dbeta_from_bf16": ("bn_bwd", ("full", "proj")),
    "sum_bf16": ("maxpool_bwd", ("full",)),
}


@pytest.mark.parametrize("mode", ["full", "proj"])
@pytest.mark.parametrize("call", sorted(CALLS))
def test_honest_bf16_results_pass(case, mode, call):
    ck = Checker(mode, chunk=1)
    CALLS[call](ck, case, None)
    assert ck.results
    bad = [r.line() for r in ck.results if not r.ok]
    assert not bad, bad
    if call == "bn_bwd":  # mode 2 recomputes the mask: near-ties are counted, never more than the allowed fraction
        assert ck.ambiguous[0] <= insitu.AMBIG_MAX_FRACTION * ck.ambiguous[1]


@pytest.mark.parametrize("fault,mode", [(f, m) for f in sorted(FAULTS) for m in FAULTS[f][1]])
def test_planted_fault_is_flagged(case, mode, fault):
    call = FAULTS[fault][0]
    ck = Checker(mode, chunk=1)
    CALLS[call](ck, case, fault)
    bad = [r for r in ck.results if not r.ok]
    assert bad, f"{fault} passed the {mode} comparator: " + "; ".join(r.line() for r in ck.results)


# ---- the same calls of the fp32 programs: f32 tensors, held to ulp_f32(r) + REL * a -------------------------------------

@pytest.mark.parametrize("mode", ["full", "proj"])
@pytest.mark.parametrize("call", sorted(CALLS))
def test_honest_f32_results_pass(case32, mode, call):
    ck = Checker(mode, chunk=1)
    CALLS[call](ck, case32, None)
    assert ck.results
    bad = [r.line() for r in ck.results if not r.ok]
    assert not bad, bad
    if call == "bn_bwd":
        assert ck.ambiguous[0] <= insitu.AMBIG_MAX_FRACTION * ck.ambiguous[1]


ALL_F32_FAULTS = dict(FAULTS, **F32_FAULTS)


@pytest.mark.parametrize("fault,mode", [(f, m) for f in sorted(ALL_F32_FAULTS) for m in ALL_F32_FAULTS[f][1]])
def test_planted_fault_is_flagged_in_f32(case32, mode, fault):
    call = ALL_F32_FAULTS[fault][0]
    ck = Checker(mode, chunk=1)
    CALLS[call](ck, case32, fault)
    bad = [r for r in ck.results if not r.ok]
    assert bad, f"{fault} passed the {mode} comparator: " + "; ".join(r.line() for r in ck.results)
    if fault == "tap_group" and mode == "full":  # nothing but the outputs that lost the terms
        assert all(r["where"][:2] == (B - 1, H - 1) and r["where"][2] >= 32 for r in bad), [r.line() for r in bad]
        assert sum(r["fail"] for r in bad) <= 16 * CO
    if fault == "dbeta_from_bf16":  # dbeta and dgamma themselves are the honest ones
        assert {r["what"] for r in bad} == {"dx"}, [r.line() for r in bad]


def test_the_rule_for_bf16_tensors_passes_what_the_f32_rule_flags(case32):
    """The gap the f32 rounding unit closes.  Until the unit followed the stored type, every activation was held to
    ulp_bf16(r) + REL * a.  Recomputed here, that rule passes an f32 convolution whose output went through bf16 on
    EVERY element: the detour's error is half a bf16 ulp of the value itself.  A weight operand rounded to bf16 it
    passes on most elements only.  That error does not shrink with r: over K = 432 terms of size t it is about
    sqrt(K) * 2^-9 * 0.58 t = 0.024 t, against r of about sqrt(K) t = 21 t and REL * a = 2^-16 * K * 0.64 t = 0.004 t,
    so the old rule gives way only where ulp_bf16(r) falls below that, at |r| under a quarter of its spread: a share
    P(|N(0, 1)| < 0.25) = 0.2 of the outputs at most, the rest passes.  ulp_f32(r) + REL * a has no such room and fails
    both faults on more than half of the outputs."""
    MISS_OLD, HIT_NEW = 0.2, 0.5
    c = case32
    x64, w64 = _f64(_nhwc(c["x"])), _f64(c["w1"])
    r = insitu.conv_gather(x64, w64, 1, 1, H, W)
    a = insitu.conv_gather(x64.abs(), w64.abs(), 1, 1, H, W)
    old, new = insitu.ulp_bf16(r) + insitu.REL * a, insitu.ulp_f32(r) + insitu.REL * a
    honest = (_f64(c["y1"][..., :CO]) - r).abs()
    assert bool((honest <= new).all())
    shares = {}
    for fault in ("out_bf16", "w_bf16"):
        y = _bf(c["y1"]) if fault == "out_bf16" else _store(F.conv2d(c["x"], _bf(c["w1"]), padding=1), CO_PITCH, c["dt"])
        err = (_f64(y[..., :CO]) - r).abs()
        shares[fault] = (float((err > old).double().mean()), float((err > new).double().mean()))
        ck = Checker("full", chunk=1)
        run_fwd(ck, c, fault)
        assert [r_.ok for r_ in ck.results if r_["what"] == "out"] == [False]
    print(f"\nshare of outputs outside (old rule, f32 rule): {shares}")
    assert shares["out_bf16"][0] == 0.0 and shares["w_bf16"][0] <= MISS_OLD, shares
    assert min(s[1] for s in shares.values()) > HIT_NEW, shares


def test_failure_report_locates_the_fault(case):
    """the worst element and the worst 16x16x16 block name the planted tile"""
    ck = Checker("full", chunk=1)
    run_fwd(ck, case, "halo")
    bad = [r for r in ck.results if not r.ok]
    assert len(bad) == 1
    r = bad[0]
    b, y, x, _ = r["where"]
    assert b == B - 1 and 16 <= y < 32 and 16 <= x < 32, r.line()
    assert r["block"][:3] == (B - 1, 16, 16), r.line()


def test_ulp_units():
    t = torch.tensor([1.0, 1.5, 2.0, -3.0, 0.0], dtype=torch.float64)
    assert insitu.ulp_bf16(t).tolist()[:4] == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]
    assert insitu.ulp_f32(t).tolist()[:3] == [2.0 ** -23, 2.0 ** -23, 2.0 ** -22]


def test_honest_elementwise_and_loss_results_pass():
    """the remaining references of the step: max-pool forward, bn_apply, softmax-CE (loss, dlogits, pred, sums),
    the dlogits rescale, the input layout change and the confusion-matrix update"""
    g = torch.Generator().manual_seed(9)
    ck = Checker("full", chunk=1)
    x = torch.randn(B, H, W, 32, generator=g).to(torch.bfloat16)
    x[0, 0, 0, 0] = x[0, 0, 1, 0]  # a tie inside a window
    pad = F.pad(x.float(), (0, 0, 1, 1, 1, 1), value=float("-inf"))
    Ho, Wo = H // 2, W // 2
    taps = torch.stack([pad[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r in range(3) for s in range(3)])
    y = taps.max(0).values.to(torch.bfloat16)
    idx = torch.argmax((taps == taps.max(0).values).to(torch.int8), dim=0).to(torch.uint8)
    ck.maxpool_fwd({"op": "maxpool3x3s2_fwd"}, x, y, idx)
    sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    res = torch.randn(B, H, W, 32, generator=g).to(torch.bfloat16)
    ck.bn_apply({"op": "bn_apply"}, x, sc, sh, res, True, torch.relu(x.float() * sc + sh + res.float()).to(torch.bfloat16))
    K, Cp = 19, 32
    logits = F.pad(torch.randn(B, H, W, K, generator=g) * 3, (0, Cp - K)).to(torch.bfloat16)
    t = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    cw = torch.tensor([1.0] * 15 + [0.0] * 4)
    z = logits.float()[..., :K]
    wp = cw[t.long()]
    wsum = wp.sum()
    loss = (wp * (torch.logsumexp(z, -1) - torch.gather(z, -1, t.long().unsqueeze(-1)).squeeze(-1))).sum() / wsum
    d = F.pad((wp / wsum).unsqueeze(-1) * (torch.softmax(z, -1) - F.one_hot(t.long(), K)), (0, Cp - K)).to(torch.bfloat16)
    pred = z.argmax(-1).to(torch.uint8)
    sums = d.float().reshape(-1, Cp).sum(0)
    ck.softmax_ce({"op": "softmax_ce"}, logits, t, cw, K, None, (loss.reshape(1), wsum.reshape(1), d, pred, sums))
    ck.scale_inplace({"op": "scale_inplace"}, d, torch.ones(1), d.clone())
    xin = torch.randn(B, 5, H, W, generator=g)
    ck.nchw_to_nhwc({"op": "nchw_to_nhwc"}, xin, F.pad(_nhwc(xin), (0, 11)).to(torch.bfloat16))
    cm = torch.randint(0, 5, (K, K), generator=g)
    after = cm + torch.bincount(t.reshape(-1).long() * K + pred.reshape(-1).long(), minlength=K * K).view(K, K)
    ck.confusion({"op": "confusion"}, cm, after, pred, t)
    bad = [r.line() for r in ck.results if not r.ok]
    assert len(ck.results) >= 13 and not bad, bad
    # and each of them notices a wrong value
    for corrupt in ("y", "loss", "pred", "dlogits_zero_weight", "sums"):
        ck = Checker("full", chunk=1)
        y2, loss2, pred2, d2, sums2 = y.clone(), loss.clone(), pred.clone(), d.clone(), sums.clone()
        if corrupt == "y":
            y2[1, 3, 4, 5] = y2[1, 3, 4, 6]
            ck.maxpool_fwd({"op": "maxpool3x3s2_fwd"}, x, y2, idx)
        else:
            if corrupt == "loss":
                loss2 = loss2 * (1 + 1e-4)
            elif corrupt == "pred":
                k = int(torch.nonzero(z[0, 0, 0] < z[0, 0, 0].max())[0])
                pred2[0, 0, 0] = k
            elif corrupt == "dlogits_zero_weight":
                p = torch.nonzero(wp == 0)[0]
                d2[p[0], p[1], p[2], 0] = 2.0 ** -20
            else:
                sums2[3] += 1e-3 * sums2.abs().max()
            ck.softmax_ce({"op": "softmax_ce"}, logits, t, cw, K, None, (loss2.reshape(1), wsum.reshape(1), d2, pred2, sums2))
        assert any(not r.ok for r in ck.results), corrupt


# --------------------------------------------------------------------------------------------------
# the references of the two-modality fusion step: 1x1 conv chains over column blocks of one weight, the bilinear
# alignment at ratio 1.5, mean_stack, the head bias gradient handed over from the loss, the layout kernels

FB, FH, FW, FHO, FWO = 2, 12, 8, 18, 12   # maps 12 x 8 -> 18 x 12 (ratio 1.5)
FC0, FC1, FO, FPITCH = 5, 6, 12, 16       # two sources of 5 and 6 real channels, 12 outputs, pitch 16
FK = 11                                   # classes of the head (pitch 16)
SQ = 12                                   # square planes for the flips and rotations


def _taps(n_in, n_out, align=False, clamp=True, coord="f32", shift_from=None):
    """f32 taps of one axis; align: the align_corners=True source index.  coord: "f32" the coordinate in plain f32
    arithmetic, "fma" as the kernel takes it (insitu.source_coordinate_f32), "f64" taken in float64 and the weights
    rounded to f32; shift_from: destination indices from this one on read one source index further (a one-tap shift)"""
    dst = torch.arange(n_out, dtype=torch.float32)
    if align:
        src = dst * torch.tensor((n_in - 1) / (n_out - 1), dtype=torch.float32)
    elif coord == "fma":
        src = insitu.source_coordinate_f32(n_in, n_out).float()
    elif coord == "f64":
        src = ((dst.double() + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    else:
        src = ((dst + 0.5) * torch.tensor(n_in / n_out, dtype=torch.float32) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    l1 = (src - i0.to(src.dtype)).float()
    if shift_from is not None:
        i0[shift_from:] = (i0[shift_from:] + 1).clamp(max=n_in - 1)
    i1 = i0 + 1
    if clamp:
        i1 = i1.clamp(max=n_in - 1)
    return i0, i1, 1 - l1, l1


def _bilinear_f32(x, ho, wo, align=False, clamp_rows=True, coord="f32", shift_from=None):
    """gather form in f32, rows of two column-interpolated taps; clamp_rows=False: the second tap of the last row reads
    row H, which in memory is row 0 of the next image (zeros past the last one)"""
    Bn, H, W, C = x.shape
    xf = x.float()
    if not clamp_rows:
        xf = torch.cat([xf, torch.cat([xf[1:, :1], torch.zeros(1, 1, W, C)])], dim=1)
    y0, y1, ly0, ly1 = _taps(H, ho, align, clamp_rows, coord, shift_from)
    x0, x1, lx0, lx1 = _taps(W, wo, align, coord=coord)

    def row(yi):
        r = xf[:, yi]
        return lx0[None, None, :, None] * r[:, :, x0] + lx1[None, None, :, None] * r[:, :, x1]

    return ly0[None, :, None, None] * row(y0) + ly1[None, :, None, None] * row(y1)


def _tap_matrix(n_in, n_out, coord="f32"):
    i0, i1, l0, l1 = _taps(n_in, n_out, coord=coord)
    m = torch.zeros(n_out, n_in)
    m.scatter_add_(1, i0[:, None], l0[:, None])
    m.scatter_add_(1, i1[:, None], l1[:, None])
    return m


@pytest.fixture(scope="module")
def fcase():
    g = torch.Generator().manual_seed(17)
    c = {}

    def padded(real, *shape):
        t = torch.randn(*shape, real, generator=g)
        return F.pad(t, (0, FPITCH - real)).to(torch.bfloat16)

    c["xa"], c["xb"] = padded(FC0, FB, FH, FW), padded(FC1, FB, FH, FW)
    c["w"] = _bf(torch.randn(FO, FC0 + FC1, 1, 1, generator=g) / 3)
    c["bias"] = F.pad(torch.randn(FO, generator=g), (0, FPITCH - FO))
    c["x"] = padded(10, FB, FH, FW)                   # the map the alignment resizes
    c["dy"] = padded(10, FB, FHO, FWO)
    c["g"] = padded(10, FB, FH, FW)
    d = F.pad(torch.randn(FB, FH, FW, FK, generator=g) * 0.01, (0, FPITCH - FK)).to(torch.bfloat16)
    c["dlogits"] = d
    c["sums"] = d.float().reshape(-1, FPITCH).sum(0)  # what the loss kernel hands over: for an upstream gradient of 1
    c["u8"] = torch.randint(0, 256, (FB, 3, SQ, SQ), generator=g).to(torch.uint8)
    c["mean"], c["std"] = torch.tensor([105.0, 110.5, 101.25]), torch.tensor([52.0, 45.5, 44.0])
    c["labels"] = torch.randint(0, 19, (FB, SQ, SQ), generator=g).to(torch.uint8)
    return c


def _link(x, w, real, extra):
    """one link of the chain in f32: 1x1 conv of the real channels + (bias and / or the chain so far), stored bf16"""
    y = _nhwc(F.conv2d(_nchw(x[..., :real].float()), w)) + extra
    return F.pad(y, (0, FPITCH - FO)).to(torch.bfloat16)


def run_fusion(ck, c, fault):
    w, b = c["w"], c["bias"][:FO]
    y0 = _link(c["xa"], w[:, :FC0], FC0, b)
    w1 = w[:, FC0:FC0 + FC1]
    if fault == "slice_padded_offset":  # the second block starts at the first source's PITCH: past the weight's columns
        w1 = w[:, FPITCH:FPITCH + FC1]
        w1 = F.pad(w1, (0, 0, 0, 0, 0, FC1 - w1.shape[1]))
    y1 = _link(c["xb"], w1, FC1, y0[..., :FO].float() + (b if fault == "bias_twice" else 0.0))
    w64 = _f64(w)
    ck.conv_forward({"op": "conv2d", "link": 0}, c["xa"], w64[:, :FC0], 1, 0, y0, bias=c["bias"])
    ck.conv_forward({"op": "conv2d", "link": 1}, c["xb"], w64[:, FC0:FC0 + FC1], 1, 0, y1, residual=y0)


def run_bilinear_fwd(ck, c, fault):
    y = _bilinear_f32(c["x"], FHO, FWO, align=fault == "align_corners", clamp_rows=fault != "no_clamp")
    ck.bilinear({"op": "bilinear_fwd"}, c["x"], y.to(torch.bfloat16), False)


BWD_SRC_ROW, BWD_DST_ROW = 5, 9  # destination rows 7, 8 and 9 reach source row 5 at ratio 1.5


def run_bilinear_bwd(ck, c, fault):
    my, mx = _tap_matrix(FH, FHO), _tap_matrix(FW, FWO)
    if fault == "missing_row":  # the gather of one source row stops one destination row early
        assert my[BWD_DST_ROW, BWD_SRC_ROW] > 0 and my[BWD_DST_ROW + 1, BWD_SRC_ROW] == 0
        my[BWD_DST_ROW, BWD_SRC_ROW] = 0
    dx = torch.einsum("px,bypc->byxc", mx, torch.einsum("oy,bopc->bypc", my, c["dy"].float()))
    ck.bilinear({"op": "bilinear_bwd"}, c["dy"], dx.to(torch.bfloat16), True)


def run_mean_stack(ck, c, fault):
    ck.mean_stack({"op": "mean_stack", "dir": "fwd"}, [c["x"], c["g"]], None,
                  ((c["g"].float() + c["x"].float()) / 2).to(torch.bfloat16))
    gi = (c["g"].float() / (1 if fault == "divisor_one" else 2)).to(torch.bfloat16)
    ck.mean_stack({"op": "mean_stack", "dir": "bwd"}, [c["g"]], 2, gi)


def run_head_bias(ck, c, fault):
    gs = 0.5
    final = (c["dlogits"].float() * gs).to(torch.bfloat16)  # the buffer after scale_inplace
    db = (c["sums"] * (1.0 if fault == "no_task_weight" else gs))[:FK]
    ck.head_bias_grad({"op": "head_bias_grad"}, _f64(final).reshape(-1, FPITCH).sum(0),
                      _f64(c["dlogits"]).abs().reshape(-1, FPITCH).sum(0) * gs, db)


def run_layouts(ck, c, fault):
    from flairhip.augment import VFLIP, apply_code, make_code
    codes = [make_code(False, False, 1), make_code(True, True, 0)]  # a quarter turn (transpose + flip), both flips

    def product(x, used):
        t = torch.stack([torch.from_numpy(apply_code(x[b].numpy(), k)) for b, k in enumerate(used)])
        v = (t.float() - c["mean"][None, :, None, None]) / c["std"][None, :, None, None]
        return F.pad(_nhwc(v), (0, 5)).to(torch.bfloat16)

    used = [VFLIP, codes[1]] if fault == "transpose_as_flip" else codes
    ck.layout_norm({"op": "d4_layout"}, c["u8"], c["mean"], c["std"], product(c["u8"], used), codes=codes)
    ck.layout_norm({"op": "u8_nchw_to_nhwc"}, c["u8"], c["mean"], c["std"], product(c["u8"], [0, 0]))
    xf = torch.randn(FB, 2, SQ, SQ, generator=torch.Generator().manual_seed(3))
    t = torch.stack([torch.from_numpy(apply_code(xf[b].numpy(), k)) for b, k in enumerate(codes)])
    ck.layout_norm({"op": "d4_layout"}, xf, None, None, F.pad(_nhwc(t), (0, 6)).to(torch.bfloat16), codes=codes)
    lab = torch.stack([torch.from_numpy(apply_code(c["labels"][b].numpy(), k)) for b, k in enumerate(codes)])
    ck.d4_labels({"op": "d4_labels"}, c["labels"], codes, lab)
    ck.nhwc_to_nchw({"op": "nhwc_to_nchw"}, c["x"], 10, _nchw(c["x"][..., :10].float()))


FCALLS = {"fusion": run_fusion, "bilinear_fwd": run_bilinear_fwd, "bilinear_bwd": run_bilinear_bwd,
          "mean_stack": run_mean_stack, "head_bias": run_head_bias, "layouts": run_layouts}
# fault -> (call it lives in, modes, what the failing results must say)
FFAULTS = {
    "slice_padded_offset": ("fusion", ("full", "proj"), lambda r: r["link"] == 1),
    "bias_twice": ("fusion", ("full", "proj"), lambda r: r["link"] == 1),
    "align_corners": ("bilinear_fwd", ("full",), lambda r: r["op"] == "bilinear_fwd"),
    "no_clamp": ("bilinear_fwd", ("full",), lambda r: r["where"][1] == FHO - 1 and r["fail"] <= FB * FWO * 10),
    "missing_row": ("bilinear_bwd", ("full",), lambda r: r["where"][1] == BWD_SRC_ROW and r["fail"] <= FB * FW * 10),
    "divisor_one": ("mean_stack", ("full",), lambda r: r["dir"] == "bwd"),
    "no_task_weight": ("head_bias", ("full",), lambda r: r["what"] == "bias gradient from the loss sums"),
    "transpose_as_flip": ("layouts", ("full",), lambda r: r["op"] == "d4_layout" and r["where"][0] == 0),
}


@pytest.mark.parametrize("mode", ["full", "proj"])
@pytest.mark.parametrize("call", sorted(FCALLS))
def test_honest_fusion_results_pass(fcase, mode, call):
    ck = Checker(mode, chunk=1)
    FCALLS[call](ck, fcase, None)
    assert ck.results
    bad = [r.line() for r in ck.results if not r.ok]
    assert not bad, bad


@pytest.mark.parametrize("fault,mode", [(f, m) for f in sorted(FFAULTS) for m in FFAULTS[f][1]])
def test_planted_fusion_fault_is_flagged_in_the_right_place(fcase, mode, fault):
    call, _, right_place = FFAULTS[fault]
    ck = Checker(mode, chunk=1)
    FCALLS[call](ck, fcase, fault)
    bad = [r for r in ck.results if not r.ok]
    assert bad, f"{fault} passed the {mode} comparator: " + "; ".join(r.line() for r in ck.results)
    assert all(right_place(r) for r in bad), [r.line() for r in bad]


def test_bilinear_matrix_is_the_aten_resize():
    """the float64 taps against F.interpolate (f32) at the sizes of the fusion stages, both directions"""
    for n_in, n_out in ((2, 3), (3, 2), (32, 48), (48, 32), (8, 12), (1, 8), (13, 40)):
        x = torch.randn(1, 1, n_in, 1, generator=torch.Generator().manual_seed(n_in))
        ref = F.interpolate(x, size=(n_out, 1), mode="bilinear", align_corners=False)[0, 0, :, 0]
        got = insitu.bilinear_matrix(n_in, n_out) @ _f64(x[0, 0, :, 0])
        # ATen takes the source coordinate in f32: a few ulps of a number up to n_in, times the step between the taps
        assert (got - _f64(ref)).abs().max().item() <= 8 * n_in * 2.0 ** -24 * 2 * x.abs().max().item()
        assert torch.allclose(insitu.bilinear_matrix(n_in, n_out).sum(1), torch.ones(n_out, dtype=torch.float64))


# ---- f32 tensors of the fp32 programs: bilinear against the coordinate the kernel takes, bn_apply, the loss gradient ----

def _f32_maps(seed):
    g = torch.Generator().manual_seed(seed)
    x = F.pad(torch.randn(FB, FH, FW, 10, generator=g), (0, FPITCH - 10))
    dy = F.pad(torch.randn(FB, FHO, FWO, 10, generator=g), (0, FPITCH - 10))
    return x, dy


@pytest.mark.parametrize("coord", ["fma", "f64"])
def test_f32_bilinear_passes_with_the_kernels_coordinate_and_tolerates_the_float64_one(coord):
    """12 x 8 <-> 18 x 12, scale 2 / 3: the f32 coordinate is off the float64 one by an f32 ulp or two, and the tap
    weights with it.  The reference takes the kernel's coordinate; a product that took the float64 one is no fault and
    must pass too on these maps: the fractions are 1 / 6, 1 / 2 and 5 / 6, so no tap nearly cancels and a is at least a
    sixth of |v0| + |v1|, the error at most a few 1e-7 of it."""
    x, dy = _f32_maps(71)
    ck = Checker("full", chunk=1)
    ck.bilinear({"op": "bilinear_fwd"}, x, _bilinear_f32(x, FHO, FWO, coord=coord), False)
    my, mx = _tap_matrix(FH, FHO, coord), _tap_matrix(FW, FWO, coord)
    dx = torch.einsum("px,bypc->byxc", mx, torch.einsum("oy,bopc->bypc", my, dy))
    ck.bilinear({"op": "bilinear_bwd"}, dy, dx, True)
    assert len(ck.results) == 4 and all(r.ok for r in ck.results), [r.line() for r in ck.results if not r.ok]
    assert not torch.equal(_tap_matrix(FH, FHO, "fma"), _tap_matrix(FH, FHO, "f64"))  # the two do differ here


def test_f32_bilinear_flags_a_one_tap_shift_and_a_bf16_detour():
    x, _ = _f32_maps(71)
    for fault in ("shift", "bf16"):
        y = _bilinear_f32(x, FHO, FWO, coord="fma", shift_from=FHO - 4 if fault == "shift" else None)
        ck = Checker("full", chunk=1)
        ck.bilinear({"op": "bilinear_fwd"}, x, _bf(y) if fault == "bf16" else y, False)
        bad = [r for r in ck.results if not r.ok]
        assert bad and all(r["what"] == "y" for r in bad), (fault, [r.line() for r in ck.results])
        if fault == "shift":
            assert bad[0]["where"][1] >= FHO - 4, bad[0].line()


def test_f32_coordinate_matrix():
    """rows sum to one; where the scale is an f32 number (ratios 2 and 1.5 downwards) both coordinates are the same
    number and so are the matrices; elsewhere they differ by f32 roundings of a coordinate below n_in"""
    for n_in, n_out in ((2, 3), (3, 2), (32, 48), (48, 32), (8, 12), (64, 32), (13, 40)):
        m32, m64 = insitu.bilinear_matrix(n_in, n_out, f32_coordinate=True), insitu.bilinear_matrix(n_in, n_out)
        assert torch.allclose(m32.sum(1), torch.ones(n_out, dtype=torch.float64))
        assert (m32 - m64).abs().max().item() <= 4 * n_in * 2.0 ** -24
        if (n_in, n_out) in ((3, 2), (48, 32), (64, 32)):
            assert torch.equal(m32, m64)
    c = insitu.source_coordinate_f32(32, 48)
    assert torch.equal(c, c.float().double()) and c[0] == 0 and bool((c[1:] > c[:-1]).all())


def test_f32_elementwise_and_loss_results():
    """bn_apply and the loss gradient with f32 tensors: honest f32 arithmetic passes, a bf16 detour of the stored
    values is flagged (for bf16 tensors it is the honest result)"""
    g = torch.Generator().manual_seed(73)
    x = torch.randn(B, H, W, 32, generator=g)
    sc, sh = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g)
    res = torch.randn(B, H, W, 32, generator=g)
    y = torch.relu(x * sc + sh + res)
    K, Cp = 19, 32
    logits = F.pad(torch.randn(B, H, W, K, generator=g) * 3, (0, Cp - K))
    t = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    cw = torch.tensor([1.0] * 15 + [0.0] * 4)
    z = logits[..., :K]
    wp = cw[t.long()]
    wsum = wp.sum()
    loss = (wp * (torch.logsumexp(z, -1) - torch.gather(z, -1, t.long().unsqueeze(-1)).squeeze(-1))).sum() / wsum
    d = F.pad((wp / wsum).unsqueeze(-1) * (torch.softmax(z, -1) - F.one_hot(t.long(), K)), (0, Cp - K))
    pred = z.argmax(-1).to(torch.uint8)
    for fault in (None, "y_bf16", "dlogits_bf16"):
        ck = Checker("full", chunk=1)
        ck.bn_apply({"op": "bn_apply"}, x, sc, sh, res, True, _bf(y) if fault == "y_bf16" else y)
        d2 = _bf(d) if fault == "dlogits_bf16" else d
        ck.softmax_ce({"op": "softmax_ce"}, logits, t, cw, K, None,
                      (loss.reshape(1), wsum.reshape(1), d2, pred, d2.reshape(-1, Cp).sum(0)))
        bad = {(r["op"], r["what"]) for r in ck.results if not r.ok}
        want = {None: set(), "y_bf16": {("bn_apply", "y")}, "dlogits_bf16": {("softmax_ce", "dlogits")}}[fault]
        assert bad == want, (fault, [r.line() for r in ck.results if not r.ok])


def test_grad_source_rules():
    """a parameter gradient is accounted for bit for bit, (a) as the dim=1 concatenation of consecutive checked wgrads
    or (b) -- a head's bias -- against the rescaled buffer its node consumed; nothing else"""
    g = torch.Generator().manual_seed(23)
    rec = insitu.Recorder(torch.nn.Module(), "full")
    a, b, other = (torch.randn(FO, n, 1, 1, generator=g) for n in (FC0, FC1, FC1))
    rec.grad_sources += [("dW", a), ("dW", other), ("dW", b)]
    P = torch.nn.Parameter

    def with_grad(t):
        p = P(torch.zeros_like(t))
        p.grad = t.clone()
        return p

    assert rec.grad_orphans([("plain.weight", with_grad(a))]) == []
    assert rec.grad_orphans([("fused.weight", with_grad(torch.cat([a, other], 1)))]) == []
    assert rec.grad_orphans([("fused.weight", with_grad(torch.cat([a, b], 1)))]) == ["fused.weight"]  # not consecutive
    assert rec.grad_orphans([("fused.weight", with_grad(torch.cat([other, a], 1)))]) == ["fused.weight"]  # wrong order
    s = torch.randn(FPITCH, generator=g)
    rec.sum_sources.append(s)
    assert rec.grad_orphans([("conv_f.bias", with_grad(s[:FO]))]) == []
    assert rec.grad_orphans([("conv_f.bias", with_grad(s[1:FO + 1]))]) == ["conv_f.bias"]
    sums = torch.randn(FPITCH, generator=g, dtype=torch.float64)
    rec.head_bias["head"] = {"call": 7, "scale": 0.5, "sums": sums * 0.5, "abs_sums": sums.abs() * 40 * 0.5}
    assert rec.grad_orphans([("head.bias", with_grad((sums.float() * 0.5)[:FK]))]) == []
    assert rec.grad_orphans([("head.bias", with_grad(sums.float()[:FK]))]) == ["head.bias"]
    assert [r["module"] for r in rec.failures()] == ["head"]


# --------------------------------------------------------------------------------------------------
# the references of the eval step (zonal inference): convs on operands with the BatchNorm scale folded in, shift as the
# bias, residual + ReLU in the epilogue; bn_eval_params; the uint8 outputs with and without test-time augmentation

EB, EH, EW, EC = 2, 20, 24, 48           # 20 x 24: ragged against 16 x 16 and 8 x 32 tiles; 48 -> 48 so that a fold over
                                          # the input channels has the shape of the right one
PK, PCP, PN = 19, 24, 40                  # classes, logit pitch, square tile
PCROP = (3, 5, 17, 30)                    # y0, x0, h, w
TIE = (0, 4, 9)                           # image, row, column (tile frame, inside the crop) of the planted exact tie
VIEWS = 8


def _bf16_once(t64):
    """float64 -> the nearest bf16 value (ties to even) in ONE rounding (a cast goes through f32 first)"""
    m, e = torch.frexp(t64)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def _double_rounding_pairs(g, want):
    """(w, s) f32 pairs whose product rounds to another bf16 value in one step (float64) than in two (f32, then bf16):
    the exact product lies just beside a bf16 tie and the f32 rounding lands on it"""
    w = torch.randn(1 << 22, generator=g) / 20
    s = torch.rand(1 << 22, generator=g) * 0.5 + 0.75
    two = (w * s).to(torch.bfloat16).double()
    hit = torch.nonzero(two != _bf16_once(w.double() * s.double())).flatten()[:want]
    assert hit.numel() == want, f"only {hit.numel()} double-rounding pairs among {w.numel()}"
    return w[hit], s[hit]


@pytest.fixture(scope="module")
def ecase():
    g = torch.Generator().manual_seed(29)
    c = {}
    x = _bf(torch.randn(EB, EC, EH, EW, generator=g))
    w = torch.randn(EC, EC, 3, 3, generator=g) / 20                      # f32 master weight: not bf16 values
    gamma, beta = torch.rand(EC, generator=g) * 0.5 + 0.75, torch.randn(EC, generator=g) * 0.1
    rm, rv = torch.randn(EC, generator=g) * 0.1, torch.rand(EC, generator=g) * 0.5 + 0.75
    scale = gamma * (1.0 / torch.sqrt(rv + EPS))                         # f32, the kernel's operation order
    shift = beta - rm * scale
    # the conv case folds a scale vector of its own: 16 output channels get a (weight, scale) pair on which the
    # float64 fold rounds differently
    pw_, ps_ = _double_rounding_pairs(g, 16)
    w[:16, 0, 0, 0] = pw_
    fscale = scale.clone()
    fscale[:16] = ps_
    res = torch.randn(EB, EH, EW, EC, generator=g).to(torch.bfloat16)
    c.update(x=x, w=w, gamma=gamma, beta=beta, rm=rm, rv=rv, scale=scale, shift=shift, fscale=fscale, res=res)
    # uint8 outputs: logits N(0, 2) in bf16 values at pitch 24 (garbage in the pad channels), one exact tie of the top two
    z = (torch.randn(EB, PN, PN, PCP, generator=g) * 2).to(torch.bfloat16)
    b, i, j = TIE
    z[b, i, j, :PK] = z[b, i, j, :PK].clamp(max=3.0)
    z[b, i, j, 3] = z[b, i, j, 7] = 4.0
    c["logits"] = z
    # an accumulator of VIEWS views
    p = torch.softmax(torch.randn(VIEWS, EB, PCROP[2], PCROP[3], PK, generator=g) * 2, dim=-1)
    acc = torch.zeros(EB, PCROP[2], PCROP[3], PCP)
    for v in range(VIEWS):
        acc[..., :PK] += p[v]
    acc[b, 1, 4, 5] = acc[b, 1, 4, 2] = acc[b, 1, 4, :PK].max() + 0.5     # an exact tie of the top two sums
    c["acc"] = acc
    return c


def _eval_conv(c, wq, fault=None):
    """the epilogue in f32 on the bf16 operand wq: relu(conv + shift + residual), stored bf16"""
    y = _nhwc(F.conv2d(c["x"], wq, padding=1))
    if fault != "no_shift":
        y = y + c["shift"]
    if fault == "residual_after_relu":
        return (torch.relu(y) + c["res"].float()).to(torch.bfloat16)
    return torch.relu(y + c["res"].float()).to(torch.bfloat16)


def run_eval_conv(ck, c, fault):
    w, s = c["w"], c["fscale"]
    wq = _bf(w * s[:, None, None, None])                                 # the packer: f32 product, then bf16
    if fault == "scale_over_inputs":
        wq = _bf(w * s[None, :, None, None])
    elif fault == "fold_in_f64":
        wq = _bf16_once(w.double() * s.double()[:, None, None, None]).float()
        c["fold_f64_differs"] = int((wq != _bf(w * s[:, None, None, None])).sum())
    y = _eval_conv(c, wq, fault)
    if fault == "last_row":  # the last row of the last (ragged) tile of the last image
        y[-1, EH - 1, 16:, :] = 0
    ck.conv_forward({"op": "conv2d"}, _nhwc(c["x"]).to(torch.bfloat16), insitu.folded_weight(w, s, True), 1, 1, y,
                    bias=c["shift"], residual=c["res"], relu=True)


def run_bn_eval(ck, c, fault):
    scale, shift = c["scale"], c["shift"]
    if fault == "no_eps":
        scale = c["gamma"] / torch.sqrt(c["rv"])
    elif fault == "shift_sign":
        shift = c["beta"] + c["rm"] * c["scale"]
    ck.bn_eval_params({"op": "bn_eval_params"}, c["gamma"], c["beta"], c["rm"], c["rv"], EPS, scale, shift)


def _u8_product(scores, p, mode, fault=None):
    """the kernels' outputs in f32: strict '>' keeps the lowest index, bands rint(p * 255)"""
    label = insitu.first_max(scores)
    bands = torch.round(p * 255.0)
    if fault == "tie_higher":
        b, i, j = TIE[0], TIE[1] - PCROP[0], TIE[2] - PCROP[1]
        assert label[b, i, j] == 3
        label[b, i, j] = 7
    if fault == "band_off":
        frac = (255.0 * p.double()) % 1.0
        far = torch.nonzero(((frac - 0.5).abs() > 0.3) & (bands < 255))[0]
        bands[tuple(far)] += 1
        if mode == "argmax_conf":  # the confidence of that pixel
            top = p.max(-1).values
            k = tuple(torch.nonzero((((255.0 * top.double()) % 1.0 - 0.5).abs() > 0.3) & (top < 0.99))[0])
            out = torch.stack([label.float(), torch.round(top * 255.0)], dim=1)
            out[k[0], 1, k[1], k[2]] += 1
            return out.to(torch.uint8)
    if mode == "argmax":
        return label.to(torch.uint8)
    if mode == "class_prob":
        return bands.permute(0, 3, 1, 2).to(torch.uint8)
    return torch.stack([label.float(), bands.max(-1).values], dim=1).to(torch.uint8)


def run_predict(mode):
    def run(ck, c, fault):
        y0, x0, h, w = PCROP
        if fault == "crop_shift":
            y0 += 1
        z = c["logits"][:, y0:y0 + h, x0:x0 + w, :PK].float()
        out = _u8_product(z, torch.softmax(z, dim=-1), mode, fault)
        ck.predict_u8({"op": "predict_u8"}, c["logits"], PK, mode, PCROP, out)
    return run


QUARTER = 4  # the forward code of a quarter turn; its inverse is code 7


def run_tta_accumulate(first):
    def run(ck, c, fault):
        from flairhip.augment import apply_code, inverse_code
        assert inverse_code(QUARTER) != QUARTER
        y0, x0, h, w = PCROP
        p = torch.softmax(c["logits"][..., :PK].float(), dim=-1).permute(0, 3, 1, 2)           # the view's frame
        back = QUARTER if fault == "forward_code" else inverse_code(QUARTER)
        p = torch.from_numpy(apply_code(p.numpy(), back)).permute(0, 2, 3, 1)[:, y0:y0 + h, x0:x0 + w]
        before = c["acc"].clone()
        after = torch.zeros_like(before)
        after[..., :PK] = p if (first and fault != "first_adds") else before[..., :PK] + p
        if fault == "pad_channel":
            after[0, 2, 3, PK] = 1e-6
        ck.tta_accumulate({"op": "tta_accumulate_"}, before, c["logits"], PK, QUARTER, PCROP, first, after)
    return run


def run_tta_predict(mode):
    def run(ck, c, fault):
        views = VIEWS - 1 if fault == "views_off_by_one" else VIEWS
        a = c["acc"][..., :PK]
        out = _u8_product(a / float(views), a / float(views), mode)
        if fault == "tie_higher":
            assert out[TIE[0], 1, 4] == 2
            out[TIE[0], 1, 4] = 5
        ck.tta_predict_u8({"op": "tta_predict_u8"}, c["acc"], mode, VIEWS, PK, out)
    return run


def run_tta_probabilities(ck, c, fault):
    views = VIEWS - 1 if fault == "views_off_by_one" else VIEWS
    out = (c["acc"][..., :PK] / float(views)).permute(0, 3, 1, 2)
    ck.tta_probabilities({"op": "tta_probabilities"}, c["acc"], VIEWS, PK, out)


ECALLS = {"eval_conv": run_eval_conv, "bn_eval": run_bn_eval, "predict_argmax": run_predict("argmax"),
          "predict_class_prob": run_predict("class_prob"), "predict_argmax_conf": run_predict("argmax_conf"),
          "tta_first": run_tta_accumulate(True), "tta_add": run_tta_accumulate(False),
          "tta_predict_argmax": run_tta_predict("argmax"), "tta_predict_class_prob": run_tta_predict("class_prob"),
          "tta_predict_argmax_conf": run_tta_predict("argmax_conf"), "tta_probabilities": run_tta_probabilities}
# (fault, call it lives in, what every failing result must be about)
EFAULTS = [
    ("scale_over_inputs", "eval_conv", "out"),       # scale folded over the input channels
    ("no_shift", "eval_conv", "out"),                # shift omitted
    ("residual_after_relu", "eval_conv", "out"),     # residual added after the ReLU
    ("last_row", "eval_conv", "out"),                # one output row of the last tile zeroed
    ("no_eps", "bn_eval", "scale"),
    ("shift_sign", "bn_eval", "shift"),
    ("tie_higher", "predict_argmax", "label"),       # the higher index at an exact tie
    ("tie_higher", "predict_argmax_conf", "label"),
    ("tie_higher", "tta_predict_argmax", "label"),
    ("band_off", "predict_class_prob", "bands"),     # a band off by one away from any half-integer
    ("band_off", "predict_argmax_conf", "confidence"),
    ("crop_shift", "predict_argmax", "label"),       # crop origin shifted by one pixel
    ("crop_shift", "predict_class_prob", "bands"),
    ("crop_shift", "predict_argmax_conf", None),
    ("forward_code", "tta_first", "accumulator"),    # a quarter turn taken back with the forward code
    ("forward_code", "tta_add", "accumulator"),
    ("first_adds", "tta_first", "accumulator"),      # first=True adding where it should overwrite
    ("pad_channel", "tta_add", "pad channels"),
    ("views_off_by_one", "tta_predict_class_prob", "bands"),
    ("views_off_by_one", "tta_predict_argmax_conf", "confidence"),
    ("views_off_by_one", "tta_probabilities", "mean probabilities"),
]


@pytest.mark.parametrize("call", sorted(ECALLS))
def test_honest_eval_results_pass(ecase, call):
    ck = Checker("full", chunk=1)
    ECALLS[call](ck, ecase, None)
    assert ck.results
    bad = [r.line() for r in ck.results if not r.ok]
    assert not bad, bad
    if call.startswith("predict") and "class_prob" not in call:
        assert ck.ties["predict_u8"] >= 1       # the planted tie was seen, and its label checked
    if call.startswith("tta_predict") and "class_prob" not in call:
        assert ck.ties["tta_predict_u8"] >= 1


@pytest.mark.parametrize("fault,call,what", EFAULTS, ids=[f"{f}-{c}" for f, c, _ in EFAULTS])
def test_planted_eval_fault_is_flagged(ecase, fault, call, what):
    ck = Checker("full", chunk=1)
    ECALLS[call](ck, ecase, fault)
    bad = [r for r in ck.results if not r.ok]
    assert bad, f"{fault} passed: " + "; ".join(r.line() for r in ck.results)
    if what is not None:
        assert all(r["what"] == what for r in bad), [r.line() for r in bad]
    if fault == "last_row":
        assert all(r["where"][:2] == (EB - 1, EH - 1) and r["where"][2] >= 16 for r in bad), [r.line() for r in bad]
    if fault in ("tie_higher", "band_off", "pad_channel"):
        assert sum(r["fail"] for r in bad) == 1, [r.line() for r in bad]


def test_a_fold_taken_in_float64_fails_the_bound_where_it_matters(ecase):
    """Scale folded in float64 and rounded once, where the packer rounds twice (f32 product, then bf16).  On the 16
    planted (weight, scale) pairs the operand then differs by one bf16 ulp of that weight, 2^-8 |w| or more, and the
    output by that times the tap's |x|.  The bound dictates: this FAILS, but only on the few outputs of those channels
    that are small against the sum of their terms -- there ulp_bf16(r) gives no room, and 2^-16 a is about 2^-8 of one
    average term for this layer's 432 taps, so a tap with an above-average |x| exceeds it (37 of 46080 outputs for this
    seed).  Where r is of the size of a, one bf16 ulp of one weight stays far inside the half ulp of r that the bound
    leaves beside the output's own rounding.  A reference that folded in float64 would therefore flag the product on
    such weights: the reference folds as the packer does (insitu.folded_weight)."""
    ck = Checker("full", chunk=1)
    run_eval_conv(ck, ecase, "fold_in_f64")
    assert ecase["fold_f64_differs"] == 16
    bad = [r for r in ck.results if not r.ok]
    assert bad and all(r["what"] == "out" and r["where"][3] < 16 for r in bad), [r.line() for r in ck.results]
    assert sum(r["fail"] for r in bad) <= 0.01 * EB * EH * EW * 16, [r.line() for r in bad]


def test_f32_eval_conv_is_checked_against_the_packers_f32_fold(ecase):
    """the fp32 eval operand is w * scale in f32, stored as it is (csrc/conv_pack.hip multiplies in f32 for both
    types): honest f32 arithmetic on it passes; the operand rounded to bf16, the scale over the wrong axis and a
    missing shift are flagged"""
    c = ecase
    w, s = c["w"], c["fscale"]
    x = c["x"] * 1.0009765625 + 2.0 ** -12       # f32 values that are no bf16 values
    res = c["res"].float() * 1.00048828125
    for fault in (None, "fold_bf16", "scale_over_inputs", "no_shift"):
        wq = w * (s[None, :, None, None] if fault == "scale_over_inputs" else s[:, None, None, None])
        if fault == "fold_bf16":
            wq = _bf(wq)
        y = _nhwc(F.conv2d(x, wq, padding=1)) + (0.0 if fault == "no_shift" else c["shift"])
        y = torch.relu(y + res)
        ck = Checker("full", chunk=1)
        ck.conv_forward({"op": "conv2d"}, _nhwc(x), insitu.folded_weight(w, s, False), 1, 1, y, bias=c["shift"],
                        residual=res, relu=True)
        assert [r.ok for r in ck.results] == [fault is None], (fault, [r.line() for r in ck.results])
    call = {}

    class Operand:
        data = torch.zeros(1, dtype=torch.float32)

    info = {"name": "m", "transpose": False, "weight": w, "scale": s, "shift": c["shift"]}
    got = insitu.Recorder._operand_values(call, info, Operand, w, c["shift"].clone())
    assert call["folded"] and torch.equal(got, (w * s[:, None, None, None]).double())
    plain = insitu.Recorder._operand_values(call, {"name": "m", "transpose": False, "weight": w}, Operand, w, None)
    assert not call["folded"] and torch.equal(plain, w.double())


def test_a_folded_operand_must_carry_its_shift():
    """Recorder._operand_values: the reference weight of an eval-mode operand is the packer's fold, and a call on it
    without the shift of that fold as its bias is a failed check (the conv reference alone would accept it: it sees
    what the kernel saw)"""
    g = torch.Generator().manual_seed(31)
    w, scale, shift = torch.randn(8, 4, 3, 3, generator=g), torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)

    class Operand:
        data = torch.zeros(1, dtype=torch.bfloat16)

    info = {"name": "m", "transpose": False, "weight": w, "scale": scale, "shift": shift}
    call = {}
    got = insitu.Recorder._operand_values(call, info, Operand, w, shift.clone())
    assert call["folded"] and torch.equal(got, (w * scale[:, None, None, None]).to(torch.bfloat16).double())
    for bias in (None, torch.zeros(8), shift + 2.0 ** -20):
        with pytest.raises(ValueError, match="shift"):
            insitu.Recorder._operand_values({}, info, Operand, w, bias)
    plain = insitu.Recorder._operand_values(call, {"name": "m", "transpose": False, "weight": w}, Operand, w, None)
    assert not call["folded"] and torch.equal(plain, w.to(torch.bfloat16).double())


def test_too_many_open_values_is_a_failed_check():
    """two equal logits: every band is 127.5 exactly, the float64 reference decides nothing -- a failed check, whatever
    the product wrote"""
    z = torch.zeros(1, 8, 8, 8, dtype=torch.bfloat16)
    ck = Checker("full", chunk=1)
    ck.predict_u8({"op": "predict_u8"}, z, 2, "class_prob", None, torch.full((1, 2, 8, 8), 128, dtype=torch.uint8))
    assert [r.ok for r in ck.results] == [False] and "half-integer" in ck.results[0]["error"]
    ck = Checker("full", chunk=1)  # the label is decided all the same: the lowest index
    ck.predict_u8({"op": "predict_u8"}, z, 2, "argmax", None, torch.zeros(1, 8, 8, dtype=torch.uint8))
    assert [r.ok for r in ck.results] == [True] and ck.ties["predict_u8"] == 64


# --------------------------------------------------------------------------------------------------
# the shapes of tests/test_conv_edges_gpu.py: what its checks catch and the per-tensor bound did not

def _bf16_conv(x, w, stride=1, pad=1):
    """an honest bf16 kernel: the f32 convolution of the bf16 operands, rounded once"""
    return F.conv2d(x, w, stride=stride, padding=pad)


def _edge_layer(seed, cin, cout, k, hw, batch=2):
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(batch, cin, *hw, generator=g))
    w = _bf(torch.randn(cout, cin, k, k, generator=g) * (cin * k * k) ** -0.5)
    return g, x, w


def _verdicts(run, y, ref_nchw, real=None):
    """(failed checks of the checker, whether max|ref| * 2^-7 -- the bound of tests/test_kernels_gpu.py and its
    siblings for bf16 -- passes the same tensor) for the stored NHWC result y against the f32 reference"""
    ck = Checker("full", chunk=1)
    run(ck, y)
    got = _nchw(y[..., :real].float()) if real else _nchw(y.float())
    err, old = (got - ref_nchw).abs().max().item(), ref_nchw.abs().max().item() * 2.0 ** -7
    return [r for r in ck.results if not r.ok], err <= old, ck, (err, old)


def test_register_operand_makes_a_hand_packed_operand_known_to_the_adapters():
    """Checker.register_operand: the entry HipConv2d.packed leaves under a recording, for an operand packed by hand.
    The adapters of the Recorder then take the call: an honest result passes, a nonzero pad channel is flagged."""
    from flairhip import ops
    g, x, w = _edge_layer(81, 30, 19, 3, (3, 5))
    pw = ops.PackedWeight(torch.empty(0, dtype=torch.bfloat16), 32, 19, 32, 32 | insitu.BCO_THIN, 3, 3, 1, 30)
    rec = insitu.Recorder(mode="full", chunk=1)
    rec._ops = ops
    with pytest.raises(KeyError):
        rec._weight(pw)
    assert rec.register_operand(pw, w, transpose=False, stride=1, padding=1, name="head") is pw
    info = rec._weight(pw)
    assert (info["name"], info["transpose"], info["stride"], info["padding"]) == ("head", False, 1, 1)
    assert torch.equal(info["weight"], w) and info["weight"] is not w and info["operand"] is pw
    for bad in (dict(transpose=True), dict(stride=2)):  # rows / stride of the operand contradict the statement
        with pytest.raises(ValueError, match="not packed"):
            rec.register_operand(pw, w, **{"transpose": False, "stride": 1, "padding": 1, **bad})
    with pytest.raises(ValueError, match="f32 OIHW"):
        rec.register_operand(pw, w.double(), stride=1, padding=1)
    pwt = ops.PackedWeight(torch.empty(0, dtype=torch.bfloat16), 32, 30, 32, 32 | insitu.BCO_THIN, 3, 3, 1, 19)
    rec.register_operand(pwt, w, transpose=True, stride=1, padding=1)  # rows = input channels, stride 1

    xs = _store(x, 32)
    y = _store(_bf16_conv(x, w), 32)
    args = dict(x=xs, w=pw, pad=1, dil=1, residual=None, bias=None, relu=False, stats=None)
    rec._op_conv2d({"op": "conv2d", "call": 0}, args, args, y)
    assert rec.results and all(r.ok for r in rec.results), [r.line() for r in rec.failures()]
    assert {r["what"] for r in rec.results} == {"out", "out pad channels"}
    y[1, 2, 4, 25] = 2.0 ** -20  # 19 classes in a pitch of 32: channel 25 feeds the next layer's k loop
    rec._op_conv2d({"op": "conv2d", "call": 1}, args, args, y)
    assert [r["what"] for r in rec.failures()] == ["out pad channels"] and rec.failures()[0]["where"] == (1, 2, 4, 6)
    ref = _bf16_conv(x, w)
    assert (_nchw(y[..., :19].float()) - ref).abs().max() <= ref.abs().max() * 2.0 ** -7  # the old bound never looked there


EDGE_HONEST = [  # cin, cout, k, stride, pad, input size
    (192, 64, 3, 1, 1, (9, 33)), (64, 128, 3, 2, 1, (17, 35)), (64, 128, 3, 2, 1, (18, 34)), (64, 128, 1, 2, 0, (17, 35)),
    (64, 64, 3, 1, 1, (3, 5)), (64, 64, 3, 1, 1, (1, 1)), (5, 64, 7, 2, 3, (19, 35)),
]


@pytest.mark.parametrize("cin,cout,k,stride,pad,hw", EDGE_HONEST)
def test_honest_bf16_results_pass_at_the_shapes_of_the_edge_grid(cin, cout, k, stride, pad, hw):
    """forward, input gradient (the dil = 2 call where stride = 2, asked for the odd and the even input size) and weight
    gradient: worst error / bound stays below 1, and near the half ulp of the one rounding for the stored tensors"""
    g, x, w = _edge_layer(83 + cin + hw[1], cin, cout, k, hw)
    ck = Checker("full", chunk=1)
    y = _bf16_conv(x, w, stride, pad)
    ck.conv_forward({"op": "conv2d"}, _store(x), _f64(w), stride, pad, _store(y))
    dy = _bf(torch.randn(y.shape, generator=g))
    dx = conv2d_input(x.shape, w, dy, stride=stride, padding=pad)
    ck.conv_dgrad({"op": "conv2d"}, _store(dy), _f64(w), stride, pad, _store(dx))
    dw = conv2d_weight(x, w.shape, dy, stride=stride, padding=pad)
    ck.conv_wgrad({"op": "conv_wgrad"}, _store(x), _store(dy), k, k, stride, pad, dw)
    assert [r["what"] for r in ck.results] == ["out", "dx", "dW"]
    assert all(r.ok for r in ck.results), [r.line() for r in ck.results if not r.ok]
    assert all(r["worst"] <= 0.75 for r in ck.results), [r.line() for r in ck.results]


def _fault_partial_sums():
    """192 -> 64 at 9 x 33: the partial sum of each half of the input channels rounded to bf16 before they are added"""
    _, x, w = _edge_layer(85, 192, 64, 3, (9, 33))
    y = _bf(_bf16_conv(x[:, :96], w[:, :96])) + _bf(_bf16_conv(x[:, 96:], w[:, 96:]))
    return (lambda ck, o: ck.conv_forward({"op": "conv2d"}, _store(x), _f64(w), 1, 1, o)), _store(y), _bf16_conv(x, w)


def _fault_residual_after_rounding():
    """64 -> 64 at 17 x 31 with a residual: the convolution is rounded to bf16, then the residual is added"""
    g, x, w = _edge_layer(87, 64, 64, 3, (17, 31))
    res = _bf(torch.randn(2, 64, 17, 31, generator=g))
    y = _bf(_bf16_conv(x, w)) + res
    return (lambda ck, o: ck.conv_forward({"op": "conv2d"}, _store(x), _f64(w), 1, 1, o, residual=_store(res))), \
        _store(y), _bf16_conv(x, w) + res


def _fault_dil2_last_row(hw):
    """the dil = 2 input gradient of 64 -> 128 (3 x 3 stride 2) for an input of size hw: the contribution of the last row
    of dy never arrives (at an odd height it feeds the last two input rows, at an even one the last three)"""
    g, x, w = _edge_layer(89 + hw[0], 64, 128, 3, hw)
    ho, wo = (hw[0] - 1) // 2 + 1, (hw[1] - 1) // 2 + 1
    dy = _bf(torch.randn(2, 128, ho, wo, generator=g))
    cut = dy.clone()
    cut[:, :, -1] = 0
    dx = conv2d_input(x.shape, w, cut, stride=2, padding=1)
    return (lambda ck, o: ck.conv_dgrad({"op": "conv2d"}, _store(dy), _f64(w), 2, 1, o)), _store(dx), \
        conv2d_input(x.shape, w, dy, stride=2, padding=1)


def _fault_ragged_column_group():
    """192 -> 64 at 9 x 33: in the ragged last column of tiles (output column 32) input channels 64..95 are read from
    the column before"""
    _, x, w = _edge_layer(91, 192, 64, 3, (9, 33))
    xs = x.clone()
    xs[:, 64:96] = torch.roll(x[:, 64:96], 1, dims=3)
    y = _bf16_conv(x, w)
    y[..., 32] = _bf16_conv(xs, w)[..., 32]
    return (lambda ck, o: ck.conv_forward({"op": "conv2d"}, _store(x), _f64(w), 1, 1, o)), _store(y), _bf16_conv(x, w)


# fault -> (builder, does max|ref| * 2^-7 pass the faulty tensor?)
EDGE_FAULTS = {
    "bf16 partial sums of two channel halves": (_fault_partial_sums, True),
    "residual added after the rounding": (_fault_residual_after_rounding, True),
    "dil = 2 dgrad drops the last row of dy, odd out_hw": (lambda: _fault_dil2_last_row((17, 35)), False),
    "dil = 2 dgrad drops the last row of dy, even out_hw": (lambda: _fault_dil2_last_row((18, 34)), False),
    "one channel group of the ragged column read one column off": (_fault_ragged_column_group, False),
}


@pytest.mark.parametrize("fault", sorted(EDGE_FAULTS))
def test_planted_fault_at_an_edge_shape_is_flagged_and_what_the_per_tensor_bound_said(fault):
    """every fault is flagged by the elementwise float64 bound; the second column of EDGE_FAULTS keeps on file which of
    them the bound of the stand-alone kernel tests (one number per tensor) let through: the precision detours -- the
    reason tests/test_conv_edges_gpu.py compares through tests/insitu.py"""
    build, old_passes = EDGE_FAULTS[fault]
    run, y, ref = build()
    honest_fails, honest_old, ck, _ = _verdicts(run, _store(ref), ref)
    assert not honest_fails and honest_old and ck.results[0]["worst"] <= 0.75, "the honest result must pass both bounds"
    fails, old, ck, (err, bound) = _verdicts(run, y, ref)
    print(f"\n{fault}: {fails[0]['fail'] if fails else 0} of {ck.results[0]['n']} elements flagged, worst error / bound "
          f"{ck.results[0]['worst']:.3g}; max error {err:.4g} against max|ref| * 2^-7 = {bound:.4g}: "
          f"{'passes' if old else 'fails'} the per-tensor bound")
    assert fails and fails[0]["what"] in ("out", "dx"), "the elementwise bound must flag the fault"
    assert old == old_passes


# ---- AdamW / Adam (csrc/optim.hip) against Checker.adamw ---------------------------------------------------------------
# An f32 torch emulation that rounds where the kernel rounds (f32 constants, every operation on its own, step size and
# sqrt(bc2) formed in double and rounded once) must stay inside the bound at every step count and gradient scale; each
# mutant of it must be flagged.  Step counts of the mutants are 20 or below: by step 1000 both bias corrections are 1
# to f32 precision and leaving them out is honestly invisible.

ADAM_LR, ADAM_BETAS, ADAM_N = 3e-3, (0.9, 0.95), 20000
# (decoupled, weight_decay, maximize, eps)
ADAM_KINDS = {
    "adamw": (True, 0.02, False, 1e-8),
    "adamw_max_eps1e-3": (True, 0.02, True, 1e-3),
    "adamw_wd0": (True, 0.0, False, 1e-8),
    "adam_l2": (False, 0.02, False, 1e-8),
    "adam_l2_max_eps1e-3": (False, 0.02, True, 1e-3),
    "adam_wd0_max": (False, 0.0, True, 1e-8),
}
ADAM_MUTANTS = ("no_bc2", "no_bc1", "lerp_beta1", "swapped_decay", "eps_in_sqrt", "maximize_ignored", "other_step")


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def _adam_f32(p, g, m, v, lr, betas, eps, wd, step, decoupled, maximize, mutant=None):
    """the kernel's update in f32 torch, operation by operation -> (p, m, v)"""
    import math
    b1, b2 = betas
    s = step if mutant != "other_step" else step + 1  # the neighbouring tensor's count (it skipped no step)
    bc1 = 1.0 if mutant == "no_bc1" else 1.0 - b1 ** s
    bc2 = 1.0 if mutant == "no_bc2" else 1.0 - b2 ** s
    lr32 = _f32(lr)
    step_size, bc2_sqrt = _f32(float(lr32) / bc1), _f32(math.sqrt(bc2))
    b1w = _f32(b1 if mutant == "lerp_beta1" else 1.0 - b1)
    b2f, b2w, wdf, epsf = _f32(b2), _f32(1.0 - b2), _f32(wd), _f32(eps)
    p, g, m, v = p.clone(), g.clone(), m.clone(), v.clone()
    if maximize and mutant != "maximize_ignored":
        g = -g
    dec = (not decoupled) if mutant == "swapped_decay" else decoupled
    if dec:
        p = p - lr32 * wdf * p
    elif wd != 0:
        g = g + wdf * p
    m = m + b1w * (g - m)
    v = b2f * v + b2w * g * g
    if mutant == "eps_in_sqrt":
        den = torch.sqrt(v / (bc2_sqrt * bc2_sqrt) + epsf)
    else:
        den = torch.sqrt(v) / bc2_sqrt + epsf
    p = p - step_size * m / den
    return p, m, v


def _adam_inputs(step, seed):
    """parameters of order 1, gradients of scale 1e-9 .. 10 (so that eps matters for some and not for others), exact
    zeros among them, moments of the gradient's scale (zero before the first step)"""
    g = torch.Generator().manual_seed(seed)
    n = ADAM_N
    p = torch.randn(n, generator=g)
    scale = 10.0 ** torch.randint(-9, 2, (n,), generator=g).float()
    gr = torch.randn(n, generator=g) * scale
    gr[:50] = 0
    if step > 1:
        m, v = torch.randn(n, generator=g) * scale * 0.3, (torch.randn(n, generator=g) * scale) ** 2 * 0.5
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    return p, gr, m, v


def _adam_check(kind, step, mutant=None, seed=1):
    decoupled, wd, maximize, eps = ADAM_KINDS[kind]
    p, gr, m, v = _adam_inputs(step, seed + step)
    p1, m1, v1 = _adam_f32(p, gr, m, v, ADAM_LR, ADAM_BETAS, eps, wd, step, decoupled, maximize, mutant)
    ck = Checker("full")
    ck.adamw({"op": "adamw", "call": 0}, p, gr, m, v, torch.tensor(float(step)), _f32(ADAM_LR), p1, m1, v1, ADAM_BETAS,
             eps, wd, decoupled, maximize)
    return ck


@pytest.mark.parametrize("step", [1, 2, 7, 20, 1000, 100000])
@pytest.mark.parametrize("kind", sorted(ADAM_KINDS))
def test_honest_adamw_emulation_passes(kind, step):
    ck = _adam_check(kind, step)
    assert [r["what"] for r in ck.results] == ["p", "exp_avg", "exp_avg_sq"]
    print("\n" + "\n".join(r.line() for r in ck.results))
    assert all(r.ok for r in ck.results), [r.line() for r in ck.results if not r.ok]
    assert max(r["worst"] for r in ck.results) <= 0.5, "an exact f32 emulation must sit well inside a bound of 8 roundings"


def _adam_mutant_applies(mutant, kind):
    decoupled, wd, maximize, _ = ADAM_KINDS[kind]
    return not ((mutant == "maximize_ignored" and not maximize) or (mutant == "swapped_decay" and wd == 0))


@pytest.mark.parametrize("step", [1, 2, 7, 20])
@pytest.mark.parametrize("mutant,kind", [(m, k) for m in ADAM_MUTANTS for k in sorted(ADAM_KINDS)
                                         if _adam_mutant_applies(m, k)])
def test_planted_adamw_fault_is_flagged(mutant, kind, step):
    ck = _adam_check(kind, step, mutant)
    bad = [r for r in ck.results if not r.ok]
    print(f"\n{mutant} {kind} step {step}: " + "; ".join(r.line() for r in ck.results))
    assert bad, f"{mutant} passed the float64 bound: " + "; ".join(r.line() for r in ck.results)
    # the moments do not depend on the bias corrections, eps or the step count: only p may be flagged for those
    if mutant in ("no_bc2", "no_bc1", "eps_in_sqrt", "other_step"):
        assert {r["what"] for r in bad} == {"p"}, [r.line() for r in bad]


# --------------------------------------------------------------------------------------------------
# the loss, resampling and label kernels at their edges (tests/test_loss_edges_gpu.py runs the real ones): an f32
# emulation of softmax_ce_kernel on the wide-logit table, pad channels, ignored labels, the 2 x 2 sum of the upsample
# backward, a weight sum of zero, the one-hot index

LK, LCP = 19, 32


def _ce_f32(logits, t, cw, K, gs=1.0, target_term="difference", pad="zero"):
    """csrc/resample_loss.hip's per-pixel arithmetic in f32 torch ops -> (loss, wsum, dlogits, pred, sums).
    target_term: "difference" keeps z_t - m from before the exponentials; "log_of_exp" takes it back out of
    exp(z_t - m) as a logarithm.  pad: "zero" writes zeros to the gradient's pad channels, "leak" 0 * the logit."""
    Cp = logits.shape[-1]
    z = logits[..., :K].float()
    tl = t.long()
    tc = tl.clamp(max=K - 1)
    wp = cw.float()[tc] * (tl < K)
    m = z.max(-1, keepdim=True).values
    d = z - m
    e = torch.exp(d)
    se = e.sum(-1)
    if target_term == "difference":
        term = torch.log(se) - d.gather(-1, tc.unsqueeze(-1)).squeeze(-1)
    else:
        term = torch.log(se) - torch.log(e.gather(-1, tc.unsqueeze(-1)).squeeze(-1))
    wsum = wp.sum()
    loss = (wp * term)[wp != 0].sum() / wsum
    dl = (gs * wp / wsum).unsqueeze(-1) * (e / se.unsqueeze(-1) - F.one_hot(tc, K))
    padding = torch.zeros(*z.shape[:-1], Cp - K) if pad == "zero" else 0.0 * logits[..., K:].float()
    dl = torch.cat([dl, padding], -1).to(logits.dtype)
    pred = insitu.first_max(z.double()).to(torch.uint8)
    return loss.reshape(1), wsum.reshape(1), dl, pred, dl.float().reshape(-1, Cp).sum(0)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("S", [176, 1000])
def test_a_target_term_taken_as_the_log_of_an_underflowed_exponential_is_flagged(S, dt):
    """the wide-logit input of tests/test_loss_edges_gpu.py: the target of some pixels lies S below the maximum, where
    exp(z_t - m) is 0 in f32.  log(exp(z_t - m)) is then -inf and the loss +inf: flagged; z_t - m itself passes."""
    from test_loss_edges_gpu import wide_case, wide_preconditions
    z, t, cw, _, _ = wide_case(S, "target", LK, LCP, dt, 0.0, "cpu")
    wide_preconditions(z, t, cw, LK, (1.0,))
    for term, want_bad in (("difference", set()), ("log_of_exp", {"loss"})):
        out = _ce_f32(z, t, cw, LK, target_term=term)
        assert bool(out[0].isinf().all()) == bool(want_bad)
        ck = Checker("full", chunk=1)
        ck.softmax_ce({"op": "softmax_ce"}, z, t, cw, LK, None, out)
        bad = {r["what"] for r in ck.results if not r.ok}
        assert bad == want_bad, (term, [r.line() for r in ck.results if not r.ok])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_a_gradient_that_lets_a_nan_pad_channel_through_is_flagged(dt):
    from test_loss_edges_gpu import GARBAGE, wide_case
    z, t, cw, _, _ = wide_case(0, "other", LK, LCP, dt, 0.0, "cpu")
    z = z.clone()
    z[..., LK:] = torch.tensor(GARBAGE).to(dt)[torch.arange(z[..., LK:].numel()).reshape(z[..., LK:].shape) % len(GARBAGE)]
    for pad, want_bad in (("zero", set()), ("leak", {"dlogits exact zeros", "per-class sums of the stored dlogits"})):
        ck = Checker("full", chunk=1)
        ck.softmax_ce({"op": "softmax_ce"}, z, t, cw, LK, None, _ce_f32(z, t, cw, LK, pad=pad))
        bad = {r["what"] for r in ck.results if not r.ok}
        assert ("dlogits exact zeros" in bad) == bool(want_bad) and bad <= want_bad, [r.line() for r in ck.results if not r.ok]


def test_a_weight_sum_of_zero_is_a_nan_loss_and_nothing_about_the_gradient():
    g = torch.Generator().manual_seed(5)
    z = F.pad(torch.randn(1, 1, 257, LK, generator=g) * 3, (0, LCP - LK))
    t = torch.full((1, 1, 257), 2, dtype=torch.uint8)
    cw = torch.ones(LK)
    cw[2] = 0.0
    assert bool(F.cross_entropy(z[..., :LK].reshape(-1, LK).double(), t.reshape(-1).long(), weight=cw.double()).isnan())
    loss, wsum, dl, pred, _ = _ce_f32(z, t, cw, LK)
    assert bool(loss.isnan()) and wsum.item() == 0.0 and bool(dl[..., :LK].isnan().all())
    cases = {"honest": (loss, wsum, dl, pred), "zero loss": (torch.zeros(1), wsum, dl, pred),
             "counted": (loss, torch.ones(1), dl, pred), "label": (loss, wsum, dl, (pred + 1) % LK),
             "pad": (loss, wsum, torch.full_like(dl, float("nan")), pred)}
    for name, out in cases.items():
        ck = Checker("full", chunk=1)
        ck.softmax_ce({"op": "softmax_ce"}, z, t, cw, LK, None, out)
        assert len(ck.results) == 4 and all(r.ok for r in ck.results) == (name == "honest"), \
            (name, [r.line() for r in ck.results])


def test_confusion_takes_labels_beyond_the_class_count_as_contributing_nothing():
    g = torch.Generator().manual_seed(6)
    K, n = 13, 4099
    t = torch.randint(0, K, (n,), generator=g).to(torch.uint8)
    p = torch.randint(0, K, (n,), generator=g).to(torch.uint8)
    t[::31] = 255
    t[5::97] = K
    p[7::53] = K + 2
    before = torch.randint(0, 9, (K, K), generator=g)
    valid = (t < K) & (p < K)
    honest = before + torch.bincount(t[valid].long() * K + p[valid].long(), minlength=K * K).view(K, K)
    # the planted defect: an ignored target counted in the last row
    tv = t.long().clamp(max=K - 1)[p < K]
    counted = before + torch.bincount(tv * K + p[p < K].long(), minlength=K * K).view(K, K)
    assert not torch.equal(honest, counted)
    for after, ok in ((honest, True), (counted, False), (before, False)):
        ck = Checker("full", chunk=1)
        ck.confusion({"op": "confusion_matrix_update"}, before, after, p, t)
        assert [r.ok for r in ck.results] == [ok], [r.line() for r in ck.results]


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_upsample_backward_sum_through_bf16_is_flagged(dt):
    """dlo = the sum of four children: held to ulp_stored(r) + REL * sum |child|.  A kernel that takes the sum through
    bf16 -- each child of an f32 tensor rounded to bf16 first; for a bf16 tensor the running sum rounded after every
    child -- is flagged."""
    g = torch.Generator().manual_seed(7)
    Bn, Hl, Wl, c1, c2 = 3, 9, 17, 24, 40
    dcat = torch.randn(Bn, 2 * Hl, 2 * Wl, c1 + c2, generator=g).to(dt)
    kids = dcat[..., :c1].float().reshape(Bn, Hl, 2, Wl, 2, c1).permute(2, 4, 0, 1, 3, 5).reshape(4, Bn, Hl, Wl, c1)
    honest = (kids[0] + kids[1] + kids[2] + kids[3]).to(dt)
    if dt == torch.float32:
        through = _bf(kids[0]) + _bf(kids[1]) + _bf(kids[2]) + _bf(kids[3])
    else:
        through = _bf(_bf(_bf(kids[0] + kids[1]) + kids[2]) + kids[3]).to(dt)
    rec = insitu.Recorder(None, "full", chunk=1)
    for dlo, ok in ((honest, True), (through, False)):
        n0 = len(rec.results)
        rec._op_upsample2x_concat_bwd({"op": "upsample2x_concat_bwd"}, {"dcat": dcat, "c1": c1}, None,
                                      (dlo, dcat[..., c1:]))
        res = rec.results[n0:]
        assert [r["what"] for r in res] == ["dlo", "dskip"] and res[1].ok and res[0].ok == ok, [r.line() for r in res]


def test_onehot_to_index_is_held_to_the_first_maximum():
    g = torch.Generator().manual_seed(8)
    oh = torch.randint(-1, 3, (2, 7, 5, 9), generator=g).float()
    first = insitu.first_max(oh.permute(0, 2, 3, 1).double()).to(torch.uint8)
    last = (6 - insitu.first_max(oh.flip(1).permute(0, 2, 3, 1).double())).to(torch.uint8)
    assert not torch.equal(first, last)
    for out, ok in ((first, True), (last, False)):
        ck = Checker("full", chunk=1)
        ck.onehot_to_index({"op": "onehot_to_index"}, oh, out)
        assert [r.ok for r in ck.results] == [ok]


# --------------------------------------------------------------------------------------------------
# the references of the U-TAE time-series branch (csrc/temporal.hip through flairhip/utae.py).  Per op: a float32 torch
# emulation with its output rounded once to the storage type must pass for bf16 and f32 storage (the worst error / bound
# ratio is printed), and each mutant -- the ways these ops go subtly wrong -- must fail.  Shapes are small on purpose:
# a variance taken with n - 1 moves a bf16 output by more than its rounding only while a group holds few values.

UDT = pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
UB, UT, UH, UW, UNH, UDK, UDV = 2, 4, 5, 7, 16, 4, 16   # sample 0 has its last two dates padded
UEPS = 1e-5


def _verdict(ck, honest, what):
    worst = max(r["worst"] for r in ck.results)
    bad = [r.line() for r in ck.results if not r.ok]
    print(f"\n{what}: worst error / bound {worst:.3g}" + (f"; flagged: {bad[:3]}" if bad else ""))
    assert (not bad) if honest else bad, (what, bad[:5])
    return worst


def _upad():
    pad = torch.zeros(UB, UT, dtype=torch.uint8)
    pad[0, UT - 2:] = 1
    return pad.reshape(-1)


def _gn_unrows(r, shape, seq):
    """inverse of Checker._gn_rows"""
    if seq is None:
        return r.reshape(shape)
    Bq, Tq = seq
    return r.reshape(Bq, -1, Tq, r.shape[2], r.shape[3]).permute(0, 2, 1, 3, 4).reshape(shape)


def _gn_inputs(seq, dt, seed=71):
    g = torch.Generator().manual_seed(seed)
    if seq is None:
        N, Hh, Ww, C, G = 2, 3, 3, 32, 4           # 72 values per group
    else:
        N, Hh, Ww, C, G = seq[0] * seq[1], 2, 3, 128, 16   # T * 8 values per group
    x = torch.randn(N, Hh, Ww, C, generator=g) * 2 + 0.5
    x[-1] = torch.randn(Hh, Ww, C, generator=g) * 1e-3          # variance 1e-6: eps = 1e-5 decides the result
    if seq is not None:
        x = x.reshape(seq[0], seq[1], Hh, Ww, C)
        x[-1] = torch.randn(seq[1], Hh, Ww, C, generator=g) * 1e-3   # every date of the last series
        x[0, -1] = 0.0                                          # a padded date as mask_images_ leaves it
        x = x.reshape(N, Hh, Ww, C)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res = torch.randn(N, Hh, Ww, C, generator=g)
    dy = torch.randn(N, Hh, Ww, C, generator=g)
    return x.to(dt), gamma, beta, res.to(dt), dy.to(dt), G


def _gn_emulate(x, gamma, beta, G, relu, res, seq, dy=None, mutant=None):
    """float32 GroupNorm forward (dy None) or backward on storage-typed tensors -> f32 results"""
    rows = lambda t: Checker._gn_rows(t.float(), G, seq)
    xg = rows(x)
    src = rows(torch.roll(x.float(), -1, dims=-1)) if mutant == "group_shift" else xg
    n = xg.shape[1] * xg.shape[3]
    if mutant == "skip_padded":  # statistics over the real dates only: sample 0's last date is padded
        keep = torch.ones(xg.shape[0], xg.shape[1], 1, 1)
        keep[: xg.shape[0] // seq[0], -1] = 0
        cnt = keep.sum((1, 3), keepdim=True) * xg.shape[3]
        m = (src * keep).sum((1, 3), keepdim=True) / cnt
        var = (((src - m) ** 2) * keep).sum((1, 3), keepdim=True) / cnt
    else:
        m = src.mean((1, 3), keepdim=True)
        var = ((src - m) ** 2).mean((1, 3), keepdim=True)
    if mutant == "n_minus_1":
        var = var * n / (n - 1)
    rs = 1.0 / torch.sqrt(var + (0.0 if mutant == "no_eps" else UEPS))
    g, b = gamma.reshape(G, -1), beta.reshape(G, -1)
    xh = (xg - m) * rs
    pre = xh * g + b
    if dy is None:
        if mutant == "relu_after_residual":
            y = torch.relu(pre + rows(res))
        else:
            y = torch.relu(pre) if relu else pre
            if res is not None:
                y = y + rows(res)
        return _gn_unrows(y, x.shape, seq)
    gm = rows(dy)
    if relu:
        gm = torch.where(pre > 0, gm, torch.zeros(()))
    prod = gm * xh
    if mutant == "dgamma_bf16":
        prod = _bf(prod)
    dgamma, dbeta = prod.sum((0, 1)).reshape(-1), gm.sum((0, 1)).reshape(-1)
    gg = gm * g
    if mutant == "const_stats":
        dx = rs * gg
    else:
        dx = rs * (gg - gg.mean((1, 3), keepdim=True) - xh * (gg * xh).mean((1, 3), keepdim=True))
    return _gn_unrows(dx, x.shape, seq), dgamma, dbeta


def _run_gn(dt, seq, relu, with_res, mutant=None):
    x, gamma, beta, res, _, G = _gn_inputs(seq, dt)
    res = res if with_res else None
    y = _gn_emulate(x, gamma, beta, G, relu, res, seq, mutant=mutant).to(dt)
    ck = Checker("full")
    ck.group_norm({"op": "group_norm"}, x, gamma, beta, G, UEPS, relu, res, y, seq=seq)
    return ck


def _run_gn_bwd(dt, seq, relu, mutant=None):
    x, gamma, beta, _, dy, G = _gn_inputs(seq, dt)
    dx, dgamma, dbeta = _gn_emulate(x, gamma, beta, G, relu, None, seq, dy=dy, mutant=mutant)
    ck = Checker("full")
    ck.group_norm_bwd({"op": "group_norm_bwd"}, x, dy, gamma, beta, G, UEPS, relu, dx.to(dt), dgamma, dbeta, seq=seq)
    return ck


@UDT
@pytest.mark.parametrize("seq,relu,with_res", [(None, False, False), (None, True, True), ((2, 3), False, False),
                                               ((6, 1), False, False)], ids=["2d", "2d-relu-res", "seq", "seq-T1"])
def test_group_norm_emulation_passes(dt, seq, relu, with_res):
    _verdict(_run_gn(dt, seq, relu, with_res), True, f"group_norm {seq} {dt}")
    _verdict(_run_gn_bwd(dt, seq, relu), True, f"group_norm_bwd {seq} {dt}")


@UDT
@pytest.mark.parametrize("mutant,seq", [("n_minus_1", None), ("n_minus_1", (2, 3)), ("no_eps", None), ("no_eps", (2, 3)),
                                        ("group_shift", None), ("group_shift", (2, 3)), ("skip_padded", (2, 3)),
                                        ("relu_after_residual", None)], ids=str)
def test_group_norm_mutant_is_flagged(dt, mutant, seq):
    relu = mutant == "relu_after_residual"
    _verdict(_run_gn(dt, seq, relu, relu, mutant), False, f"group_norm {mutant} {seq} {dt}")


@UDT
@pytest.mark.parametrize("seq", [None, (2, 3)], ids=["2d", "seq"])
@pytest.mark.parametrize("mutant", ["const_stats", "dgamma_bf16"])
def test_group_norm_bwd_mutant_is_flagged(dt, mutant, seq):
    ck = _run_gn_bwd(dt, seq, seq is None, mutant)
    _verdict(ck, False, f"group_norm_bwd {mutant} {seq} {dt}")
    flagged = {r["what"] for r in ck.results if not r.ok}
    assert flagged == ({"dx"} if mutant == "const_stats" else {"dgamma"}), flagged


def test_group_norm_bwd_counts_too_many_ambiguous_relu_masks_on_the_reference_alone():
    """gamma = beta = 0 puts every pre-activation at zero: the mask is open wherever dy is not 0, which is too often"""
    x, gamma, beta, _, dy, G = _gn_inputs(None, torch.float32)
    ck = Checker("full")
    zero = torch.zeros_like(gamma)
    dx, dgamma, dbeta = _gn_emulate(x, zero, zero, G, True, None, None, dy=dy)
    ck.group_norm_bwd({"op": "group_norm_bwd"}, x, dy, zero, zero, G, UEPS, True, dx, dgamma, dbeta)
    assert [r["what"] for r in ck.results if not r.ok] == ["ambiguous ReLU masks"]


# ---- L-TAE attention

def _ltae_inputs(dt, seed=73):
    g = torch.Generator().manual_seed(seed)
    N = UB * UT
    k = torch.randn(N, UH, UW, UNH * UDK, generator=g).to(dt)
    v = torch.randn(N, UH, UW, UNH * UDV, generator=g).to(dt)
    Q = torch.randn(UNH, UDK, generator=g) * (2.0 / UDK) ** 0.5
    drop = torch.empty(UNH, UB, UT, UH * UW).bernoulli_(0.9, generator=g) / 0.9
    dout = torch.randn(UB, UH, UW, UNH * UDV, generator=g).to(dt)
    ext = torch.randn(UNH, UB, UT, UH * UW, generator=g)
    return k, v, Q, _upad(), drop, dout, ext


def _ltae_emulate(k, v, Q, pad, drop, mutant=None):
    P = UH * UW
    k5, v5 = k.float().reshape(UB, UT, P, UNH, UDK), v.float().reshape(UB, UT, P, UNH, UDV)
    padm = pad.reshape(UB, UT).bool()[:, :, None, None]
    temp = float(UDK) if mutant == "temperature" else float(UDK) ** 0.5
    s = (k5 * Q).sum(-1) / temp
    if mutant != "pad_keeps_weight":
        s = s.masked_fill(padm, -1e3)
    dr = torch.ones_like(s) if drop is None else drop.permute(1, 2, 3, 0)
    p = torch.softmax(s, dim=1)
    if mutant == "drop_before_norm":
        e = torch.exp(s - s.max(1, keepdim=True).values) * dr
        at = e / e.sum(1, keepdim=True).clamp_min(1e-30)
    else:
        at = p * dr
    used = _bf(at) if mutant == "prob_bf16" else at
    out = (used[..., None] * v5).sum(1)
    return out.reshape(UB, UH, UW, -1), at.permute(3, 0, 1, 2).contiguous(), p.permute(3, 0, 1, 2).contiguous()


def _run_ltae(dt, train, mutant=None):
    k, v, Q, pad, drop, _, _ = _ltae_inputs(dt)
    drop = drop if train else None
    out, attn, prob = _ltae_emulate(k, v, Q, pad, drop, mutant)
    ck = Checker("full")
    ck.ltae_attention({"op": "ltae_attention"}, k, v, Q, pad, drop, UB, UT, out.to(dt), attn, prob if train else None)
    return ck


def _ltae_bwd_emulate(k, v, Q, pad, drop, prob, dout, ext, mutant=None):
    P = UH * UW
    k5, v5 = k.float().reshape(UB, UT, P, UNH, UDK), v.float().reshape(UB, UT, P, UNH, UDV)
    padm = pad.reshape(UB, UT).bool()[:, :, None, None]
    p, dr = prob.permute(1, 2, 3, 0), drop.permute(1, 2, 3, 0)
    go = dout.float().reshape(UB, 1, P, UNH, UDV)
    da = (go * v5).sum(-1)
    if mutant != "no_dattn_ext":
        da = da + ext.permute(1, 2, 3, 0)
    if mutant == "through_dropped_attn":
        at = p * dr
        ds = at * (da - (at * da).sum(1, keepdim=True))
    else:
        dp = da * dr
        ds = p * (dp - (p * dp).sum(1, keepdim=True))
    ds = ds.masked_fill(padm, 0.0) / float(UDK) ** 0.5
    dk = (ds[..., None] * Q).reshape(k.shape)
    dv = ((p * dr)[..., None] * go).reshape(v.shape)
    prod = ds[..., None] * k5
    dq = prod[:1].sum((0, 1, 2)) if mutant == "dq_one_sample" else prod.sum((0, 1, 2))
    return dk, dv, dq


def _run_ltae_bwd(dt, mutant=None):
    k, v, Q, pad, drop, dout, ext = _ltae_inputs(dt)
    _, _, prob = _ltae_emulate(k, v, Q, pad, drop)
    dk, dv, dq = _ltae_bwd_emulate(k, v, Q, pad, drop, prob, dout, ext, mutant)
    ck = Checker("full")
    ck.ltae_attention_bwd({"op": "ltae_attention_bwd"}, k, v, Q, pad, drop, prob, dout, ext, UB, UT, dk.to(dt), dv.to(dt), dq)
    return ck


@UDT
def test_ltae_attention_emulation_passes(dt):
    _verdict(_run_ltae(dt, False), True, f"ltae_attention {dt}")
    _verdict(_run_ltae(dt, True), True, f"ltae_attention_train {dt}")
    ck = _run_ltae_bwd(dt)
    _verdict(ck, True, f"ltae_attention_bwd {dt}")
    assert [t for t, _ in ck.grad_sources] == ["dQ"]


@UDT
@pytest.mark.parametrize("mutant", ["temperature", "pad_keeps_weight", "drop_before_norm", "prob_bf16"])
def test_ltae_attention_mutant_is_flagged(dt, mutant):
    _verdict(_run_ltae(dt, True, mutant), False, f"ltae_attention_train {mutant} {dt}")


@UDT
@pytest.mark.parametrize("mutant", ["no_dattn_ext", "dq_one_sample", "through_dropped_attn"])
def test_ltae_attention_bwd_mutant_is_flagged(dt, mutant):
    ck = _run_ltae_bwd(dt, mutant)
    _verdict(ck, False, f"ltae_attention_bwd {mutant} {dt}")
    if mutant == "dq_one_sample":
        assert {r["what"] for r in ck.results if not r.ok} == {"dQ"}


# ---- temporal_aggregate

def _agg_inputs(dt, seed=79, C=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(UB * UT, UH, UW, C, generator=g).to(dt)
    attn = torch.rand(UNH, UB, UT, UH * UW, generator=g) + 0.05  # non-zero at the padded dates: the mask matters
    dout = torch.randn(UB, UH, UW, C, generator=g).to(dt)
    return x, attn, _upad(), dout


def _run_aggregate(dt, mutant=None):
    x, attn, pad, dout = _agg_inputs(dt)
    C, P = x.shape[-1], UH * UW
    x5 = x.float().reshape(UB, UT, P, UNH, C // UNH)
    a4 = attn.permute(1, 2, 3, 0)
    if mutant == "heads_rotated":
        a4 = torch.roll(a4, 1, dims=-1)
    dead = pad.reshape(UB, UT).bool()[:, :, None, None]
    am = a4 if mutant == "no_pad_mask" else a4.masked_fill(dead, 0.0)
    out = (am[..., None] * x5).sum(1).reshape(UB, UH, UW, C)
    go = dout.float().reshape(UB, 1, P, UNH, C // UNH)
    dx = (am[..., None] * go).reshape(x.shape)
    dattn = (x5 * go).sum(-1)
    if mutant != "no_pad_mask":
        dattn = dattn.masked_fill(dead, 0.0)
    if mutant == "dattn_group_missing":
        dattn[..., 5] = 0.0
    ck = Checker("full")
    ck.temporal_aggregate({"op": "temporal_aggregate"}, x, attn, pad, UB, UT, True, out.to(dt))
    ck.temporal_aggregate_bwd({"op": "temporal_aggregate_bwd"}, x, attn, pad, dout, UB, UT, True, dx.to(dt),
                              dattn.permute(3, 0, 1, 2).contiguous())
    return ck


@UDT
def test_temporal_aggregate_emulation_passes(dt):
    _verdict(_run_aggregate(dt), True, f"temporal_aggregate and its backward {dt}")


@UDT
@pytest.mark.parametrize("mutant", ["heads_rotated", "no_pad_mask", "dattn_group_missing"])
def test_temporal_aggregate_mutant_is_flagged(dt, mutant):
    ck = _run_aggregate(dt, mutant)
    _verdict(ck, False, f"temporal_aggregate {mutant} {dt}")
    flagged = {r["what"] for r in ck.results if not r.ok}
    assert flagged == ({"dattn"} if mutant == "dattn_group_missing" else {"out", "dx", "dattn"} - (
        {"dattn"} if mutant == "heads_rotated" else set())), flagged


# ---- reflect padding, column sums, the encoding, the elementwise kernels

def _run_reflect(dt, hw, mutant=None):
    g = torch.Generator().manual_seed(83)
    x = torch.randn(2, 16, *hw, generator=g).to(dt)
    dpad = torch.randn(2, 16, hw[0] + 2, hw[1] + 2, generator=g).to(dt)
    xx = x.float().requires_grad_()
    y = F.pad(xx, (1, 1, 1, 1), mode="reflect")
    d = dpad.float().clone()
    if mutant == "corners_dropped":
        for cy in (0, -1):
            for cx in (0, -1):
                d[:, :, cy, cx] = 0.0
    (y * d).sum().backward()
    ck = Checker("full")
    ck.reflect_pad1({"op": "reflect_pad1"}, _nhwc(x), _nhwc(y.detach()).to(dt))
    ck.reflect_pad1_bwd({"op": "reflect_pad1_bwd"}, _nhwc(dpad), _nhwc(xx.grad).to(dt))
    return ck


@UDT
@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (5, 7), (10, 10)], ids=str)
def test_reflect_pad_emulation_passes_and_dropped_corners_are_flagged(dt, hw):
    _verdict(_run_reflect(dt, hw), True, f"reflect_pad1 and its backward {hw} {dt}")
    ck = _run_reflect(dt, hw, "corners_dropped")
    _verdict(ck, False, f"reflect_pad1_bwd corners_dropped {hw} {dt}")
    bad = [r for r in ck.results if not r.ok]
    # the four pixels next to the corners (they receive up to four contributions), and nothing else
    assert [r["what"] for r in bad] == ["dx"] and bad[0]["fail"] <= 4 * 2 * 16


@UDT
def test_column_sums_emulation_passes_and_a_dropped_partial_block_is_flagged(dt):
    g = torch.Generator().manual_seed(89)
    x = torch.randn(70, 24, generator=g).to(dt)          # 70 rows: two blocks of 32 and a partial one of 6
    blocks = [x.float()[i:i + 32].sum(0) for i in range(0, 70, 32)]
    for parts, honest in ((blocks, True), (blocks[:-1], False)):
        ck = Checker("full")
        ck.column_sums({"op": "column_sums"}, x, sum(parts))
        _verdict(ck, honest, f"column_sums {'all blocks' if honest else 'last partial block dropped'} {dt}")


def _encoding_emulate(pos, d, repeat, mutant=None, period=1000.0):
    j = torch.arange(d * repeat)
    jj, head = j % d, j // d
    pair = head if mutant == "exponent_per_head" else torch.div(jj, 2, rounding_mode="floor")
    arg = pos.float()[:, None] / torch.pow(torch.tensor(period), 2.0 * pair.float() / d)
    odd = (jj % 2 == 1)[None, :]
    if mutant == "sin_cos_swapped":
        odd = ~odd
    return torch.where(odd, torch.cos(arg), torch.sin(arg))


@pytest.mark.parametrize("mutant", [None, "sin_cos_swapped", "exponent_per_head"])
def test_positional_encoding_emulation_and_mutants(mutant):
    pos = torch.tensor([0.0, 1.0, 17.0, 203.0, 364.0])
    ck = Checker("full")
    ck.positional_encoding({"op": "positional_encoding"}, pos, 16, 16, 1000.0, _encoding_emulate(pos, 16, 16, mutant))
    _verdict(ck, mutant is None, f"positional_encoding {mutant}")


@UDT
def test_elementwise_utae_kernels(dt):
    g = torch.Generator().manual_seed(97)
    N, C = UB * UT, 32
    x = torch.randn(N, UH, UW, C, generator=g).to(dt)
    pad = _upad()
    vec = torch.randn(N, C, generator=g)
    m = (torch.empty(N, UH, UW, C).bernoulli_(0.8, generator=g) / 0.8).to(dt)
    flags = torch.tensor([0, 0, 1, 1, 0, 0, 0, 0], dtype=torch.uint8)
    raw = torch.randn(N, 3, UH, UW, generator=g)
    raw[2:4] = 0.0
    padm = pad.bool()[:, None, None, None]
    for mutant in (None, "leak", "double_rounding", "flags"):
        ck = Checker("full")
        ck.add_rowvec({"op": "add_rowvec_"}, x, vec, (x.float() + vec[:, None, None, :]).to(dt))
        masked = torch.where(padm & (mutant != "leak" or torch.arange(C) > 0), torch.tensor(1.5, dtype=dt), x)
        ck.mask_images({"op": "mask_images_"}, x, pad, 1.5, masked)
        ck.mul({"op": "mul"}, x, m, ((_bf(x.float() * 1.0078125) if mutant == "double_rounding" else x.float()) * m.float()
                                     ).to(dt))
        ck.detect_pad_images({"op": "detect_pad_images"}, raw, 0.0, flags if mutant != "flags" else 1 - flags)
        _verdict(ck, mutant is None, f"add_rowvec / mask_images / mul / detect_pad_images {mutant} {dt}")
        want = {None: [], "leak": ["mask_images_"], "double_rounding": ["mul"], "flags": ["detect_pad_images"]}[mutant]
        assert [r["op"] for r in ck.results if not r.ok] == want


# ---- the transposed-operand paths of flairhip/utae.py

@UDT
def test_transposed_operand_references_disagree_with_the_untransposed_weight(dt):
    """ConvTranspose2d(3, 1, 1) as a pad-1 conv with a transposed operand, and the input gradient of a reflect-padded
    (pad-0) 3x3 conv as a pad-2 conv with out_hw: correct emulations pass conv_transposed, and a reference built from
    the same weight taken as it stands (no exchange of the channel axes, no flipped taps) rejects them"""
    g = torch.Generator().manual_seed(101)
    q = _bf if dt == torch.bfloat16 else (lambda t: t)
    C, Hh, Ww = 16, 5, 7
    w = q(torch.randn(C, C, 3, 3, generator=g) / 8)          # in == out, so that the untransposed weight has a valid shape
    x = q(torch.randn(2, C, Hh, Ww, generator=g))
    bias = torch.randn(C, generator=g)
    up = torch.relu(F.conv_transpose2d(x, w, padding=1) + bias[None, :, None, None])
    dxp = F.conv_transpose2d(x, w, padding=0)                # [2, C, H + 2, W + 2]
    for what, out, pad_t, pad_call, b, relu in (("ConvTranspose2d forward", up, 1, 1, bias, True),
                                                ("reflect conv input gradient", dxp, 0, 2, None, False)):
        ck = Checker("full")
        ck.conv_transposed({"op": "conv2d"}, _nhwc(x).to(dt), w.double(), pad_t, _nhwc(out).to(dt), bias=b, relu=relu)
        _verdict(ck, True, f"{what} {dt}")
        ck = Checker("full")
        ck.conv_forward({"op": "conv2d"}, _nhwc(x).to(dt), w.double(), 1, pad_call, _nhwc(out).to(dt), bias=b, relu=relu)
        _verdict(ck, False, f"{what} against the untransposed weight {dt}")
    # and the adjoint really is the adjoint: <conv(x', w), d> == <x', conv_transposed(d, w)> in float64
    xp, d = torch.randn(2, C, Hh + 2, Ww + 2, generator=g).double(), x.double()
    lhs = (F.conv2d(xp, w.double()) * d).sum()
    rhs = (xp * F.conv_transpose2d(d, w.double())).sum()
    assert abs(lhs - rhs) <= 1e-9 * abs(lhs)


def test_conv_transpose_weight_gradient_must_take_the_output_gradient_as_its_input():
    """the backward of ConvTranspose2d as the product evaluates it: right after the forward conv of the output gradient d0
    (the ':D' operand), conv_wgrad(d0, x) -- with the operands the other way round the values are those of another layer"""
    g = torch.Generator().manual_seed(109)
    C, Hh, Ww = 16, 5, 7
    d0, xa = torch.randn(2, Hh, Ww, C, generator=g), torch.randn(2, Hh, Ww, C, generator=g)
    for x, dy, ok in ((d0, xa, True), (xa, d0, False)):
        rec = insitu.Recorder(torch.nn.Module(), "full")
        rec._convT_grad = (6, (d0.data_ptr(), tuple(d0.shape)))
        dw = conv2d_weight(_nchw(x), (C, C, 3, 3), _nchw(dy), padding=1)
        args = {"x": x, "dy": dy, "kh": 3, "kw": 3, "stride": 1, "pad": 1, "accumulate": False, "out": None}
        rec._op_conv_wgrad({"op": "conv_wgrad", "call": 7}, args, args, dw)
        assert [r["what"] for r in rec.results if not r.ok] == ([] if ok else
                                                               ["ConvTranspose2d weight gradient: x is the output gradient"])
        assert rec._convT_grad is None


def test_packed_bias_vector_of_the_utae_operands():
    g = torch.Generator().manual_seed(103)
    n, pitch = 19, 24
    b, scale, shift = torch.randn(n, generator=g), torch.rand(pitch, generator=g) + 0.5, torch.randn(pitch, generator=g)
    train, folded = torch.zeros(pitch), torch.zeros(pitch)
    train[:n] = b
    folded[:n] = shift[:n] + scale[:n] * b
    for vec, sc, sh, hb, ok in ((train, None, None, b, True), (folded, scale, shift, b, True), (train, scale, shift, b, False),
                                (folded, None, None, b, False), (torch.zeros(pitch), None, None, None, True),
                                (train, None, None, None, False), (shift.clone(), scale, shift, b, False)):
        ck = Checker("full")
        ck.packed_bias({"op": "utae_packed"}, vec, hb, n, sc, sh)
        assert [r.ok for r in ck.results] == [ok]


def test_grad_source_rules_of_the_utae_step():
    """dW as the dim=1 concatenation of two consecutive wgrads, [:n].clone() slices of checked sums and of checked
    dgamma / dbeta vectors, Conv1d / Linear views of a 1x1 dW and dQ as returned -- and nothing looser"""
    g = torch.Generator().manual_seed(107)
    rec = insitu.Recorder(torch.nn.Module(), "full")
    dwa, dwb, lin = torch.randn(8, 6, 3, 3, generator=g), torch.randn(8, 10, 3, 3, generator=g), torch.randn(12, 20, 1, 1, generator=g)
    dgam, sums, dq = torch.randn(24, generator=g), torch.randn(32, generator=g), torch.randn(16, 4, generator=g)
    rec.grad_sources += [("dW", dwa), ("dW", dwb), ("dW", lin), ("dgamma", dgam), ("dQ", dq)]
    rec.sum_sources.append(sums)

    def orphan(t, name="m.weight"):
        p = torch.nn.Parameter(torch.zeros_like(t))
        p.grad = t.clone()
        return rec.grad_orphans([(name, p)]) != []

    assert not orphan(torch.cat([dwa, dwb], 1)) and orphan(torch.cat([dwb, dwa], 1))
    assert not orphan(lin.view(12, 20, 1)) and not orphan(lin.view(12, 20)) and orphan(lin.view(12, 20).t().contiguous())
    assert orphan(lin.view(12, 20)[:, :10].contiguous()) and orphan(lin.view(20, 12))
    assert not orphan(dgam[:19].clone(), "m.weight") and orphan(dgam[1:20].clone()) and orphan(dgam[:19] * 1.0000001)
    assert not orphan(sums[:19].clone(), "m.bias") and orphan(sums[2:21].clone(), "m.bias")
    # column sums of a tensor that no checked conv_wgrad call read are not a bias gradient (dy in place of d0)
    rec.sum_inputs[id(sums)] = (40, (4096, (2, 5, 7, 32)))
    assert orphan(sums[:19].clone(), "m.bias")
    rec.wgrad_operands += [(20, (4096, (2, 5, 7, 32))), (41, (8192, (2, 5, 7, 32))), (49, (4096, (2, 5, 7, 32)))]
    assert orphan(sums[:19].clone(), "m.bias")      # the same address in another node, another tensor in this one
    rec.wgrad_operands.append((45, (4096, (2, 5, 7, 32))))
    assert not orphan(sums[:19].clone(), "m.bias")
    assert not orphan(dq, "Q") and orphan(dq.t().contiguous().t(), "Q") is False  # the same values in another layout
    assert orphan(dq[:8].clone(), "Q") and orphan(dq + 1e-6, "Q")
