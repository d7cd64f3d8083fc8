"""The operand cache of the conv layers on the device: the layout request is the key, one batched re-pack covers
every re-packable entry, and a fused optimizer step invalidates what it must.  Pack kernels only, tiny shapes."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
REQUESTS = [(True, False), (False, False), (True, True), (False, True)]  # (ring, thin)


def _conv(cin, cout, k, stride=1, padding=0):
    from flairhip import nn as hnn
    return hnn.HipConv2d(cin, cout, k, stride, padding).cuda()


def test_the_layout_request_is_the_cache_key(cuda):
    from flairhip import lib as L
    wide = _conv(64, 64, 3, padding=1)
    first = [wide.packed(BF, ring=r, thin=t) for r, t in REQUESTS]
    again = [wide.packed(BF, ring=r, thin=t) for r, t in reversed(REQUESTS)][::-1]
    for (ring, _), pw, pw2 in zip(REQUESTS, first, again):
        assert bool(pw.bco & L.BCO_RING) == ring
        assert pw2 is pw
    assert len({id(pw) for pw in first}) == 4

    thin_layer = _conv(16, 32, 3, padding=1)
    for ring, thin in REQUESTS + REQUESTS[::-1]:
        assert bool(thin_layer.packed(BF, ring=ring, thin=thin).bco & L.BCO_THIN) == thin

    unpadded = _conv(64, 64, 3, padding=0)  # neither pad-1 kernel applies: four times the same question
    assert len({id(unpadded.packed(BF, ring=r, thin=t)) for r, t in REQUESTS}) == 1


class _Layers(nn.Module):
    def __init__(self):
        super().__init__()
        self.ring = _conv(64, 64, 3, padding=1)
        self.thin = _conv(16, 32, 3, padding=1)
        self.igemm = _conv(64, 128, 3, stride=2, padding=1)
        self.stem = _conv(5, 64, 7, stride=2, padding=3)
        self.fusion = _conv(64 + 24, 40, 1)


def test_one_batched_repack_covers_every_repackable_entry(cuda, monkeypatch):
    from flairhip import lib as L
    from flairhip import nn as hnn
    from flairhip import ops
    torch.manual_seed(5)
    m = _Layers()
    # (layer, transpose, ring, thin): the default request of every layer in both directions, then every other layout
    # request on the ring layer -- a plan that looks for a fixed list of names misses some of these
    whole = [(c, tr, True, True) for c in (m.ring, m.thin, m.igemm) for tr in (False, True)]
    whole += [(m.stem, False, True, True)]
    whole += [(m.ring, tr, r, t) for tr in (False, True) for r, t in REQUESTS if not (r and t)]
    splits, out_pitch = (64, 24), ops.pad_channels(40)
    blocks = [(off, c, ops.pad_channels(c), False) for off, c in ((0, 64), (64, 24))]
    blocks += [(off, c, out_pitch, True) for off, c in ((0, 64), (64, 24))]
    assert sum(splits) == m.fusion.in_channels

    def request_all():
        w = m.fusion.weight.detach()
        return ([c.packed(BF, transpose=tr, ring=r, thin=t) for c, tr, r, t in whole] +
                [hnn._fusion_slice(m.fusion, w, off, c, BF, pitch, tr) for off, c, pitch, tr in blocks])

    before = request_all()
    kinds = [pw.bco & (L.BCO_RING | L.BCO_THIN | L.BCO_STEM) for pw in before]
    assert {L.BCO_RING, L.BCO_THIN, L.BCO_STEM, 0} == set(kinds)  # every table of the batch has work
    old = [pw.data.clone() for pw in before]
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p))
    plan = hnn.PackPlan(m)
    plan.refresh(BF)
    assert sorted(t[0] for t in plan.batch.tables) == sorted(set(kinds))  # one table per layout
    assert sum(t[2] for t in plan.batch.tables) == len(before)

    fresh = []
    for c, tr, ring, thin in whole:
        fresh.append(ops.pack_conv_weight(c.weight.detach(), BF, c.stride, c.out_pitch if tr else c.in_pitch,
                                          transpose=tr, allow_ring=ring and c.padding == 1,
                                          allow_thin=thin and c.padding == 1, allow_stem=c.padding == 3))
    for off, c, pitch, tr in blocks:
        fresh.append(ops.pack_conv_weight(m.fusion.weight.detach()[:, off:off + c].contiguous(), BF, 1, pitch,
                                          transpose=tr))
    for i, (pw, ref, was) in enumerate(zip(before, fresh, old)):
        assert pw.bco == ref.bco and torch.equal(pw.data, ref.data), i
        assert not torch.equal(pw.data, was), i

    calls = []
    real = ops.pack_conv_weight
    monkeypatch.setattr(ops, "pack_conv_weight", lambda *a, **k: calls.append(a) or real(*a, **k))
    after = request_all()
    assert not calls
    assert all(a is b for a, b in zip(after, before))


def test_a_fused_optimizer_step_reaches_the_next_forward(cuda, monkeypatch):
    """torch's fused AdamW moves no ``_version``: the operand of step 2 must still be the pack of step 1's result"""
    from flairhip import nn as hnn
    from flairhip import ops
    torch.manual_seed(6)
    conv, bn = _conv(64, 64, 3, padding=1), hnn.HipBatchNorm2d(64).cuda().train()
    opt = torch.optim.AdamW([conv.weight, bn.weight, bn.bias], lr=1e-2, fused=True)
    x = torch.randn(1, 16, 16, 64, device=cuda).to(BF)
    used = []
    real = ops.conv2d_bn_stats
    monkeypatch.setattr(ops, "conv2d_bn_stats", lambda x, pw, *a, **k: used.append(pw) or real(x, pw, *a, **k))
    weights = [conv.weight.detach().clone()]
    for _ in range(2):
        y = hnn.conv_bn_act(x, conv, bn)
        opt.zero_grad(set_to_none=True)
        y.float().square().sum().backward()
        opt.step()
        weights.append(conv.weight.detach().clone())
    assert not torch.equal(weights[0], weights[1])
    assert len(used) == 2 and used[1] is not used[0]
    assert torch.equal(used[1].data, ops.pack_conv_weight(weights[1], BF, 1, 64).data)
    assert not torch.equal(used[1].data, used[0].data)
