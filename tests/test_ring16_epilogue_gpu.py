"""The epilogue forms of conv3x3_ring16_kernel (csrc/conv3x3_ring.hip: statistics only, plain, residual, general),
each chosen once per launch from the call's flags: every form against torch's CPU float64 conv2d on the bf16-rounded
operands at the bound of tests/test_ring_conv_gpu.py, the statistics rows against the float64 sums of the stored
tensor, run-to-run bits, and res aliasing out -- at ragged sizes of both tile shapes, with two output-channel blocks,
and with a grid of 8 blocks so that a block walks several tiles and the channel block changes between them."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B = 2
DT = torch.bfloat16
# cin, cout, H, W, FFA_RING_GRID (0 = default): 9x33 and 17x40 run on 8x32 tiles, 18x20 on 16x16 tiles
CASES = [
    (64, 128, 9, 33, 0),
    (128, 64, 17, 40, 0),
    (128, 128, 18, 20, 0),
    (64, 128, 17, 40, 8),    # 12 pixel tiles x 2 channel blocks on 8 blocks: three or four tiles per block
    (128, 128, 18, 20, 8),   # 8 pixel tiles x 2 channel blocks on 8 blocks
]
# form -> (bias, residual, relu, stats): what ring16_epilogue_form keys on
FORMS = {
    "stats": (False, False, False, True),
    "plain": (False, False, False, False),
    "res": (False, True, False, False),
    "general": (True, True, True, True),
    "general_bias": (True, False, False, False),
    "general_res_stats": (False, True, False, True),
}


def to_nhwc(x_nchw, dev, cp):
    b, c, h, w = x_nchw.shape
    out = torch.zeros(b, h, w, cp, dtype=torch.float32)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return out.to(DT).to(dev).contiguous()


def rq(x):
    return x.to(DT).double()


@functools.lru_cache(maxsize=None)
def operands(case):
    """Host tensors and the float64 references of one case, computed once and shared by the forms."""
    cin, cout, H, W, _ = case
    g = torch.Generator().manual_seed(cin * 5 + cout + H * W)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    bias = torch.randn(cout, generator=g)
    res = torch.randn(B, cout, H, W, generator=g)
    conv = F.conv2d(rq(x), rq(w), None, padding=1)
    return x, w, bias, res, conv


def reference(case, form):
    _, _, bias, res, conv = operands(case)
    hb, hr, relu, _ = FORMS[form]
    ref = conv
    if hb:
        ref = ref + bias.double().view(1, -1, 1, 1)
    if hr:
        ref = ref + rq(res)
    return ref.relu() if relu else ref


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}_g{c[4]}" for c in CASES])
def test_ring16_epilogue_form(cuda, monkeypatch, case, form):
    from flairhip import ops, lib as L
    cin, cout, H, W, cap = case
    monkeypatch.setenv("FFA_RING", "1")
    if cap:
        monkeypatch.setenv("FFA_RING_GRID", str(cap))
    x, w, bias, res, conv = operands(case)
    hb, hr, relu, hs = FORMS[form]
    xd = to_nhwc(x, cuda, cin)
    pw = ops.pack_conv_weight(w.to(cuda), DT, 1, cin)
    assert pw.bco & L.BCO_RING, "eligible layer did not get the ring layout"
    bd = bias.to(cuda) if hb else None
    rd = to_nhwc(res, cuda, cout) if hr else None
    rows = ops.conv_stat_rows(B, H, W, pw)

    def run(residual, out=None):
        st = torch.full((rows * 2 * cout,), float("nan"), device=cuda) if hs else None
        y = ops.conv2d(xd, pw, 1, cout, bias=bd, residual=residual, relu=relu, stats=st, out=out)
        return y, st

    y, st = run(rd)
    torch.cuda.synchronize()
    # the bound of tests/test_ring_conv_gpu.py: half a bf16 ulp of the largest convolution value, twice that where
    # a bias or a residual is added in front of the rounding
    tol = float(conv.abs().max()) * 2 ** -7 * (2 if (hb or hr) else 1)
    got = y.double().cpu().permute(0, 3, 1, 2)
    err = (got - reference(case, form)).abs().max().item()
    print(f"{form} {case}: max error {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    if hs:
        part = st.view(rows, 2, cout).double().sum(0).cpu()
        stored = y.double().cpu().view(-1, cout)
        assert torch.allclose(part[0], stored.sum(0), rtol=1e-5, atol=1e-3)
        assert torch.allclose(part[1], (stored * stored).sum(0), rtol=1e-5, atol=1e-3)
    # run to run
    y2, st2 = run(rd)
    torch.cuda.synchronize()
    assert torch.equal(y, y2)
    if hs:
        assert torch.equal(st, st2)
    # res aliasing out: a lane reads its own residual elements before it writes them
    if hr:
        buf = rd.clone()
        y3, st3 = run(buf, out=buf)
        torch.cuda.synchronize()
        assert y3.data_ptr() == buf.data_ptr()
        assert torch.equal(y3, y)
        if hs:
            assert torch.equal(st3, st)


@pytest.mark.parametrize("form", ["stats", "plain", "res", "general"])
def test_ring16_epilogue_form_with_prologue(cuda, monkeypatch, form):
    """The same forms behind the fused BatchNorm + ReLU prologue: bit for bit the plain kernel on the tensor
    ffa_bn_apply writes (the prologue kernels are instantiations of their own per form)."""
    from flairhip import ops
    cin, cout, H, W = 64, 128, 17, 40
    monkeypatch.setenv("FFA_RING", "1")
    monkeypatch.setenv("FFA_RING_GRID", "8")
    x, w, bias, res, _ = operands((cin, cout, H, W, 8))
    hb, hr, relu, hs = FORMS[form]
    g = torch.Generator().manual_seed(11)
    sc = (torch.rand(cin, generator=g) + 0.5).to(cuda)
    sh = (torch.randn(cin, generator=g) * 0.5 + 0.3).to(cuda)
    xd = to_nhwc(x, cuda, cin)
    pw = ops.pack_conv_weight(w.to(cuda), DT, 1, cin)
    bd = bias.to(cuda) if hb else None
    rd = to_nhwc(res, cuda, cout) if hr else None
    rows = ops.conv_stat_rows(B, H, W, pw)
    st_a = torch.full((rows * 2 * cout,), float("nan"), device=cuda) if hs else None
    st_b = torch.full((rows * 2 * cout,), float("nan"), device=cuda) if hs else None
    xn = ops.bn_apply(xd, sc, sh, relu=True)
    ref = ops.conv3x3_ring(xn, pw, cout, bias=bd, residual=rd, relu=relu, stats=st_a)
    got = ops.conv3x3_ring(xd, pw, cout, bias=bd, residual=rd, relu=relu, stats=st_b, pro_scale=sc, pro_shift=sh)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    if hs:
        assert torch.equal(st_a, st_b)
