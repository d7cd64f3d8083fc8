"""Every kernel of csrc/temporal.hip on its own, forward and backward, against float64.

Each test calls one flairhip.ops wrapper and compares it with a float64 restatement, in plain torch on the CPU, of the
formula in the reference's flair_hub/models/multitemp_model.py (torch autograd in float64 for the backward kernels).
Inputs are quantised to the storage type (f32 or bf16) first and handed to both sides, so the comparison sees the
kernel's f32 arithmetic and its one output rounding only.

Tolerances (none of them is fitted to what the kernels give):
  f32 storage   the same torch formula is also run in float32 on the CPU; the kernel may err by 16 times that run's
                maximum error against float64 (summation order, expf / sinf / powf of the device), with a floor of
                2^-20 * max(1, max |ref|) for outputs that are exactly 0 or exact in float32
  bf16 storage  per element |got - ref| <= 2^-8 |ref| + the f32 bound (the one bf16 output rounding); the
                f32 outputs of a bf16 call (attn, prob, dattn, dQ, dgamma, dbeta) get the f32 bound alone
The ReLU mask of the GroupNorm backward is recomputed by the kernel in f32, so those tests assert that the float64
pre-activation keeps min |pre| >= 1e-5 on the quantised inputs (GN2D_SEED) and leave no element out.

Kernels of csrc/temporal.hip, the tests that call them, and what one MI355X run of this module measured.
Each entry: largest |got - ref| / max(1, max |ref|) over the cases, and that error as a fraction of its bound.
  kernel (csrc/temporal.hip)       test                                       f32 storage        bf16 storage
  reflect_pad1_kernel              test_reflect_pad1                          exact              exact
  reflect_pad1_bwd_kernel          test_reflect_pad1                          8.3e-08  0.06      3.0e-03  1.00
  group_norm_kernel, 2-D           test_group_norm_2d                         1.1e-07  0.07      3.0e-03  0.99
  group_norm_kernel, sequence      test_group_norm_seq                        9.1e-08  0.06      3.0e-03  0.98
  group_norm_bwd_kernel, 2-D       test_group_norm_2d              dx         1.1e-07  0.07      2.7e-03  0.99
                                                                   dgamma     1.7e-07  0.08      1.2e-07  0.08
                                                                   dbeta      1.5e-07  0.09      3.2e-08  0.03
  group_norm_bwd_kernel, sequence  test_group_norm_seq             dx         1.6e-07  0.08      2.8e-03  0.99
                                                                   dgamma     1.7e-07  0.08      1.3e-07  0.07
                                                                   dbeta      1.0e-07  0.06      3.5e-08  0.04
  positional_encoding_kernel       test_positional_encoding                   1.4e-05  0.36      (f32 only)
  add_rowvec_kernel                test_add_rowvec                            4.1e-08  0.04      2.1e-03  1.00
  detect_pad_kernel                test_detect_pad_images                     exact              (f32 only)
  mask_images_kernel               test_mask_images                           exact              exact
  mul_kernel                       test_mul_dropout                           3.8e-08  0.04      1.9e-03  0.97
  ltae_attention_kernel            test_ltae_attention_forward*    out        2.5e-07  0.08      3.1e-03  1.00
                                                                   attn       9.4e-08  0.06      1.1e-07  0.07
  ltae_attention_train_kernel      test_ltae_attention_forward*,   out        2.5e-07  0.09      3.1e-03  1.00
                                   test_ltae_attention_dropout_*   attn       1.3e-07  0.07      1.3e-07  0.07
                                                                   prob       1.1e-07  0.06      1.1e-07  0.07
  ltae_attention_bwd_kernel        test_ltae_attention_dropout_*,  dk         3.2e-07  0.12      2.4e-03  0.99
                                   test_ltae_attention_backward_*  dv         1.5e-07  0.06      3.0e-03  0.99
                                                                   dQ         3.6e-07  0.18      2.9e-07  0.10
  temporal_aggregate_kernel        test_temporal_aggregate                    8.5e-08  0.08      2.8e-03  0.99
  temporal_aggregate_bwd_kernel    test_temporal_aggregate         dx         4.3e-08  0.05      3.8e-03  1.00
                                                                   dattn      1.5e-07  0.15      8.6e-08  0.06
  mean_stack_kernel                test_sentinel_gpu.py::test_mean_stack_kernel
The f32 kernels stay within 0.4 of a bound that is itself 1e-6 to 2e-5; the bf16-stored outputs sit at their bound because
bf16 round-to-nearest alone errs by up to 2^-8 of the value (half an ulp of an 8-bit significand), which is the bound's
first term: what is left for the arithmetic is the f32 part.
No bound was moved.  test_ltae_attention_dropout_and_backward at n_head * d_k = 3 found ops.ltae_attention_bwd failing
in column_sums (rows of 8 columns): the kernel now pads its dQ partial rows to a multiple of 8.
"""
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
HW = {1: (1, 1), 9: (3, 3), 10: (2, 5), 77: (7, 11), 65 * 65: (65, 65), 128 * 129: (128, 129)}  # P -> (h, w)
EPS = 1e-5

_measured = {}  # (kernel, storage) -> largest error as a fraction of its bound, largest error relative to max(1, |ref|)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (kernel, storage), (frac, rel) in sorted(_measured.items()):
        print(f"\nMEASURED {kernel:28s} {storage:5s} {rel:9.2e} of max(1, max|ref|)   {frac:6.3f} of the bound", end="")


def _quant(t, dtype):
    """values of the storage type, held in f32"""
    return t.to(dtype).float()


def _dev(t, dtype, cuda):
    return t.to(dtype).contiguous().to(cuda)


def _f32_bound(ref, yard):
    """16 x the error of the float32 CPU run of the same formula, floor 2^-20 max(1, max |ref|)"""
    assert yard.dtype == torch.float32 and ref.dtype == torch.float64 and yard.shape == ref.shape
    return max(16.0 * (yard.double() - ref).abs().max().item(), 2.0 ** -20 * max(1.0, ref.abs().max().item()))


def _check(kernel, dtype, got, ref, yard, f32_out=False, what=""):
    """got (device tensor, ref's layout up to a reshape) against the float64 ref within the module's bounds"""
    storage = "bf16" if dtype == BF16 else "f32"
    assert got.dtype == (F32 if f32_out else dtype), (kernel, what, got.dtype)
    got = got.detach().cpu().double().reshape(ref.shape)
    bound = _f32_bound(ref, yard)
    lim = torch.full_like(ref, bound)
    if dtype == BF16 and not f32_out:
        lim = lim + 2.0 ** -8 * ref.abs()
    err = (got - ref).abs()
    frac = (err / lim).max().item()
    rel = err.max().item() / max(1.0, ref.abs().max().item())
    old = _measured.get((kernel, storage), (0.0, 0.0))
    _measured[(kernel, storage)] = (max(old[0], frac), max(old[1], rel))
    assert torch.isfinite(got).all() and bool((err <= lim).all()), \
        f"{kernel} {storage} {what}: max error {err.max().item():.3e}, {frac:.2f} of the bound (f32 part {bound:.3e})"


# --------------------------------------------------------------------------------------------------
# float64 / float32 restatements (channel-last, as the kernels hold the tensors)

def _group_norm(x, gamma, beta, groups, dims):
    """nn.GroupNorm: x [..., C] -> [..., G, C/G], biased statistics over `dims` of that view"""
    C = x.shape[-1]
    xg = x.reshape(*x.shape[:-1], groups, C // groups)
    mean = xg.mean(dim=dims, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=dims, keepdim=True)
    y = (xg - mean) / torch.sqrt(var + EPS) * gamma.reshape(groups, -1) + beta.reshape(groups, -1)
    return y.reshape(x.shape)


def _gn_ref(x, gamma, beta, groups, dims, dt, relu=False, res=None, dy=None):
    """-> pre-activation, y [, dx, dgamma, dbeta]"""
    x, gamma, beta = (t.to(dt).clone().requires_grad_(dy is not None) for t in (x, gamma, beta))
    pre = _group_norm(x, gamma, beta, groups, dims)
    y = F.relu(pre) if relu else pre
    if res is not None:
        y = y + res.to(dt)
    if dy is None:
        return pre.detach(), y.detach()
    (y * dy.to(dt)).sum().backward()
    return pre.detach(), y.detach(), x.grad, gamma.grad, beta.grad


def _attention_ref(k, v, Q, pad, drop, dt, dout=None, dattn_ext=None):
    """MultiHeadAttention + ScaledDotProductAttention with one learnt query per head: k [B,T,P,NH,DK], v [B,T,P,NH,DV],
    Q [NH,DK], pad bool [B,T], drop / dattn_ext [NH,B,T,P] -> out [B,P,NH,DV], attn, prob [NH,B,T,P] [, dk, dv, dQ]"""
    grad = dout is not None
    k, v, Q = (t.to(dt).clone().requires_grad_(grad) for t in (k, v, Q))
    score = (k * Q).sum(-1) / math.sqrt(k.shape[-1])                  # [B,T,P,NH]
    score = score.masked_fill(pad[:, :, None, None], -1e3)
    prob = torch.softmax(score, dim=1)
    attn = prob if drop is None else prob * drop.to(dt).permute(1, 2, 3, 0)
    out = (attn[..., None] * v).sum(1)
    res = [out.detach(), attn.detach().permute(3, 0, 1, 2), prob.detach().permute(3, 0, 1, 2)]
    if grad:
        loss = (out * dout.to(dt)).sum()
        if dattn_ext is not None:
            loss = loss + (attn * dattn_ext.to(dt).permute(1, 2, 3, 0)).sum()
        loss.backward()
        res += [k.grad, v.grad, Q.grad]
    return res


def _aggregate_ref(x, attn, pad, use_pad, dt, dout=None):
    """Temporal_Aggregator 'att_group': x [B,T,P,C], attn [NH,B,T,P] -> out [B,P,C] [, dx, dattn]"""
    grad = dout is not None
    x, attn = (t.to(dt).clone().requires_grad_(grad) for t in (x, attn))
    a = attn.permute(1, 2, 3, 0)
    if use_pad:
        a = a * (~pad).to(dt)[:, :, None, None]
    out = (a.repeat_interleave(x.shape[-1] // attn.shape[0], dim=-1) * x).sum(1)
    if not grad:
        return [out.detach()]
    (out * dout.to(dt)).sum().backward()
    return [out.detach(), x.grad, attn.grad]


def _positional_ref(pos, d, repeat, dt, period=1000.0):
    """PositionalEncoder: pos [n] -> [n, d * repeat]"""
    j = torch.arange(d, dtype=dt)
    denom = torch.pow(torch.tensor(period, dtype=dt), 2 * torch.div(j, 2, rounding_mode="floor") / d)
    tab = pos.to(dt)[:, None] / denom
    tab[:, 0::2] = torch.sin(tab[:, 0::2])
    tab[:, 1::2] = torch.cos(tab[:, 1::2])
    return torch.cat([tab] * repeat, dim=-1)


def _pads(B, T, kind):
    """bool [B,T]: 'none', 'some' (the last sample loses its later dates, the first its last one) or 'all' (as 'some',
    and every date of sample 0 padded)"""
    pad = torch.zeros(B, T, dtype=torch.bool)
    if kind != "none":
        pad[B - 1, T // 2:] = True
        pad[0, T - 1] = True
        if kind == "all":
            pad[0] = True
    return pad


def _u8(pad, cuda):
    return pad.reshape(-1).to(torch.uint8).to(cuda)


# --------------------------------------------------------------------------------------------------
# GroupNorm, 2-D geometry (ConvLayer's nn.GroupNorm(4)): group_norm, group_norm_bwd

GN2D_SHAPES = [(1, 32, 3, 3), (5, 64, 7, 11), (3, 128, 5, 4)]  # n = 72 (under one block), 1232 (no multiple of 256), 640
GN2D_SEED = 1  # keeps min |pre| >= 1e-5 at every shape for f32 and for bf16 inputs (test_group_norm_relu_margins)


def _gn2d_inputs(shape, dtype):
    """NHWC x, gamma, beta, residual, dy of one shape; drawn in NCHW order as x = randn * 2 + 0.5, gamma = rand + 0.5,
    beta = randn"""
    N, C, H, W = shape
    g = torch.Generator().manual_seed(GN2D_SEED)
    x = torch.randn(N, C, H, W, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res, dy = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    x, res, dy = (_quant(t, dtype).permute(0, 2, 3, 1).contiguous() for t in (x, res, dy))
    return x, gamma, beta, res, dy


@DTYPES
@pytest.mark.parametrize("shape", GN2D_SHAPES, ids=str)
def test_group_norm_relu_margins(shape, dtype):
    """CPU: the seed keeps the float64 pre-activation away from the ReLU's kink on the quantised inputs, and the
    restatement above is nn.GroupNorm"""
    x, gamma, beta, _, _ = _gn2d_inputs(shape, dtype)
    pre, _ = _gn_ref(x, gamma, beta, 4, (1, 2, 4), torch.float64)
    assert pre.abs().min().item() >= 1e-5
    torch_pre = F.group_norm(x.double().permute(0, 3, 1, 2), 4, gamma.double(), beta.double(), EPS).permute(0, 2, 3, 1)
    assert (pre - torch_pre).abs().max().item() <= 1e-12


@gpu
@DTYPES
@pytest.mark.parametrize("shape", GN2D_SHAPES, ids=str)
def test_group_norm_2d(cuda, shape, dtype):
    from flairhip import ops
    x, gamma, beta, res, dy = _gn2d_inputs(shape, dtype)
    xd, rd, dyd, gd, bd = _dev(x, dtype, cuda), _dev(res, dtype, cuda), _dev(dy, dtype, cuda), gamma.to(cuda), beta.to(cuda)
    for relu in (False, True):
        for r, rdev in ((None, None), (res, rd)):
            ref = _gn_ref(x, gamma, beta, 4, (1, 2, 4), torch.float64, relu, r, dy)
            yard = _gn_ref(x, gamma, beta, 4, (1, 2, 4), F32, relu, r, dy)
            if relu:
                assert ref[0].abs().min().item() >= 1e-5  # the kernel's f32 ReLU mask is the float64 one
            what = f"relu={relu} residual={r is not None}"
            _check("group_norm (2-D)", dtype, ops.group_norm(xd, gd, bd, 4, relu=relu, residual=rdev), ref[1], yard[1],
                   what=what)
            if r is None:  # a residual's gradient is dy itself: the backward kernel does not see it
                dx, dgamma, dbeta = ops.group_norm_bwd(xd, dyd, gd, bd, 4, relu=relu)
                _check("group_norm_bwd (2-D) dx", dtype, dx, ref[2], yard[2], what=what)
                _check("group_norm_bwd (2-D) dgamma", dtype, dgamma, ref[3], yard[3], f32_out=True, what=what)
                _check("group_norm_bwd (2-D) dbeta", dtype, dbeta, ref[4], yard[4], f32_out=True, what=what)


# --------------------------------------------------------------------------------------------------
# GroupNorm, sequence geometry (LTAE2d.in_norm over the T dates of a pixel, out_norm with T = 1)

@gpu
@DTYPES
@pytest.mark.parametrize("geom", [(2, 5, 3, 4), (1, 1, 2, 3), (3, 9, 1, 1), (2, 2, 5, 7)], ids=str)
def test_group_norm_seq(cuda, geom, dtype):
    from flairhip import ops
    B, T, h, w = geom
    C, G = 128, 16
    g = torch.Generator().manual_seed(3)
    x = _quant(torch.randn(B, T, h, w, C, generator=g) * 2 + 0.5, dtype)
    dy = _quant(torch.randn(B, T, h, w, C, generator=g), dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    ref = _gn_ref(x, gamma, beta, G, (1, 5), torch.float64, dy=dy)
    yard = _gn_ref(x, gamma, beta, G, (1, 5), F32, dy=dy)
    xd, dyd = _dev(x.reshape(B * T, h, w, C), dtype, cuda), _dev(dy.reshape(B * T, h, w, C), dtype, cuda)
    gd, bd = gamma.to(cuda), beta.to(cuda)
    _check("group_norm (sequence)", dtype, ops.group_norm_seq(xd, B, T, gd, bd, G), ref[1], yard[1])
    dx, dgamma, dbeta = ops.group_norm_seq_bwd(xd, dyd, B, T, gd, bd, G)
    _check("group_norm_bwd (sequence) dx", dtype, dx, ref[2], yard[2])
    _check("group_norm_bwd (sequence) dgamma", dtype, dgamma, ref[3], yard[3], f32_out=True)
    _check("group_norm_bwd (sequence) dbeta", dtype, dbeta, ref[4], yard[4], f32_out=True)


@gpu
def test_group_norm_bwd_refuses_channel_groups_that_do_not_divide_the_block(cuda):
    from flairhip import ops
    from flairhip.lib import FlairHipError
    x = torch.randn(2 * 3, 2, 2, 384, device=cuda)  # 384 / 16 = 24 channels per group, 256 % 24 != 0
    gamma, beta = torch.ones(384, device=cuda), torch.zeros(384, device=cuda)
    with pytest.raises(FlairHipError, match="do not divide the block size"):
        ops.group_norm_seq_bwd(x, x.clone(), 2, 3, gamma, beta, 16)
    with pytest.raises(FlairHipError, match="do not divide the block size"):
        ops.group_norm_bwd(x, x.clone(), gamma, beta, 16)


# --------------------------------------------------------------------------------------------------
# reflect padding (nn.Conv2d(padding_mode="reflect")): reflect_pad1, reflect_pad1_bwd

@gpu
@DTYPES
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("hw", [(2, 2), (2, 5), (3, 3), (7, 11)], ids=str)  # H = 2, 3: rows 1 and H-2 coincide or touch
def test_reflect_pad1(cuda, hw, C, dtype):
    from flairhip import ops
    (H, W), N = hw, 2
    g = torch.Generator().manual_seed(4)
    x = _quant(torch.randn(N, C, H, W, generator=g), dtype)
    dpad = _quant(torch.randn(N, C, H + 2, W + 2, generator=g), dtype)

    def run(dt):
        xx = x.to(dt).requires_grad_()
        y = F.pad(xx, (1, 1, 1, 1), mode="reflect")
        (y * dpad.to(dt)).sum().backward()
        return y.detach().permute(0, 2, 3, 1), xx.grad.permute(0, 2, 3, 1)

    ref, yard = run(torch.float64), run(F32)
    got = ops.reflect_pad1(_dev(x.permute(0, 2, 3, 1), dtype, cuda))
    assert got.dtype == dtype and torch.equal(got.float().cpu(), ref[0].float())
    _check("reflect_pad1_bwd", dtype, ops.reflect_pad1_bwd(_dev(dpad.permute(0, 2, 3, 1), dtype, cuda)), ref[1], yard[1])


# --------------------------------------------------------------------------------------------------
# positional_encoding, add_rowvec_

@gpu
@pytest.mark.parametrize("d,repeat", [(16, 16), (5, 3)])  # the model's case; odd d
def test_positional_encoding(cuda, d, repeat):
    from flairhip import ops
    pos = torch.tensor([0.0, 1.0, 364.0, 1000.0, 17.0, 203.0])
    ref, yard = _positional_ref(pos, d, repeat, torch.float64), _positional_ref(pos, d, repeat, F32)
    _check("positional_encoding", F32, ops.positional_encoding(pos.to(cuda), d, repeat), ref, yard)


@gpu
@DTYPES
@pytest.mark.parametrize("d,repeat", [(16, 16), (5, 3)])
def test_add_rowvec(cuda, d, repeat, dtype):
    from flairhip import ops
    N, P, C = 3, 7, d * repeat  # P * C = 105 with C = 15: no multiple of 256
    g = torch.Generator().manual_seed(5)
    x = _quant(torch.randn(N, 1, P, C, generator=g), dtype)
    vec = _positional_ref(torch.tensor([0.0, 364.0, 1000.0]), d, repeat, F32)
    ref = x.double() + vec.double()[:, None, None, :]
    yard = x + vec[:, None, None, :]
    xd = _dev(x, dtype, cuda)
    got = ops.add_rowvec_(xd, vec.to(cuda))
    assert got.data_ptr() == xd.data_ptr()  # in place
    _check("add_rowvec", dtype, got, ref, yard)


# --------------------------------------------------------------------------------------------------
# detect_pad_images, mask_images_, mul

SIZES = [1, 255, 257, 10 * 7 * 11]  # elements per image


@gpu
@pytest.mark.parametrize("value", [0.0, 2.5])
@pytest.mark.parametrize("size", SIZES)
def test_detect_pad_images(cuda, size, value):
    from flairhip import ops
    g = torch.Generator().manual_seed(6)
    last = torch.full((size,), value)
    last[-1] = value + 1.0                                       # differs from the pad value in its last element only
    images = [torch.randn(size, generator=g), torch.full((size,), value), last, torch.full((size,), float("nan")),
              torch.full((size,), -value)]                       # -0.0 == 0.0: padded, as == says; -2.5: not padded
    x = torch.stack(images)
    expect = (x == value).all(dim=1)
    assert expect.tolist() == [False, True, False, False, value == 0.0]
    got = ops.detect_pad_images(x.to(cuda), value)
    assert got.dtype == torch.uint8 and got.cpu().bool().tolist() == expect.tolist()
    _measured[("detect_pad_images (exact)", "f32")] = (0.0, 0.0)


@gpu
@DTYPES
@pytest.mark.parametrize("value", [0.0, 1.5])
@pytest.mark.parametrize("size", SIZES)
def test_mask_images(cuda, size, value, dtype):
    from flairhip import ops
    g = torch.Generator().manual_seed(7)
    x = _quant(torch.randn(5, size, generator=g), dtype)
    pad = torch.tensor([1, 0, 0, 1, 0], dtype=torch.bool)
    expect = torch.where(pad[:, None], torch.tensor(value), x)
    xd = _dev(x, dtype, cuda)
    got = ops.mask_images_(xd, _u8(pad, cuda), value)
    assert got.data_ptr() == xd.data_ptr() and got.dtype == dtype and torch.equal(got.float().cpu(), expect)
    _measured[("mask_images (exact)", "bf16" if dtype == BF16 else "f32")] = (0.0, 0.0)


@gpu
@DTYPES
@pytest.mark.parametrize("size", SIZES)
def test_mul_dropout(cuda, size, dtype):
    """the MLP dropout of LTAE2d and its backward: y = x * m with m = 0 or 1 / (1 - p), p = 0.2"""
    from flairhip import ops
    g = torch.Generator().manual_seed(8)
    x = _quant(torch.randn(3, size, generator=g), dtype)
    m = _quant(torch.empty(3, size).bernoulli_(0.8, generator=g) / 0.8, dtype)
    _check("mul", dtype, ops.mul(_dev(x, dtype, cuda), _dev(m, dtype, cuda)), x.double() * m.double(), x * m)


# --------------------------------------------------------------------------------------------------
# L-TAE attention

GEOMS = [(2, 5, 77, 16, 4, 16), (3, 4, 9, 16, 4, 16), (1, 1, 1, 3, 1, 5), (2, 61, 10, 4, 8, 32)]  # B, T, P, NH, DK, DV
PADS = ["none", "some", "all"]


def _attention_inputs(geom, dtype, seed=9):
    B, T, P, NH, DK, DV = geom
    g = torch.Generator().manual_seed(seed)
    k = _quant(torch.randn(B, T, P, NH, DK, generator=g), dtype)
    v = _quant(torch.randn(B, T, P, NH, DV, generator=g), dtype)
    Q = torch.randn(NH, DK, generator=g) * math.sqrt(2.0 / DK)       # MultiHeadAttention's initialisation
    dout = _quant(torch.randn(B, P, NH, DV, generator=g), dtype)
    dattn_ext = torch.randn(NH, B, T, P, generator=g)
    drop = torch.empty(NH, B, T, P).bernoulli_(0.9, generator=g) / 0.9  # keep = 0.9, scaled by 1 / 0.9
    return k, v, Q, dout, dattn_ext, drop


def _attention_dev(geom, k, v, Q, dtype, cuda):
    B, T, P, NH, DK, DV = geom
    h, w = HW[P]
    return _dev(k.reshape(B * T, h, w, NH * DK), dtype, cuda), _dev(v.reshape(B * T, h, w, NH * DV), dtype, cuda), Q.to(cuda)


def _attention_forward(cuda, geom, kind, dtype):
    from flairhip import ops
    B, T = geom[:2]
    k, v, Q, _, _, _ = _attention_inputs(geom, dtype)
    pad = _pads(B, T, kind)
    ref, yard = _attention_ref(k, v, Q, pad, None, torch.float64), _attention_ref(k, v, Q, pad, None, F32)
    if kind == "all":  # the reference's masked_fill(-1e3) on every date: uniform 1 / T
        assert torch.equal(ref[1][:, 0], torch.full_like(ref[1][:, 0], 1.0 / T))
    kd, vd, Qd = _attention_dev(geom, k, v, Q, dtype, cuda)
    out, attn = ops.ltae_attention(kd, vd, Qd, _u8(pad, cuda), B, T)
    out_t, attn_t, prob_t = ops.ltae_attention_train(kd, vd, Qd, _u8(pad, cuda), B, T, None)
    assert torch.equal(out, out_t) and torch.equal(attn, attn_t) and torch.equal(attn_t, prob_t)
    _check("ltae_attention out", dtype, out, ref[0], yard[0], what=kind)
    _check("ltae_attention attn", dtype, attn, ref[1], yard[1], f32_out=True, what=kind)
    _check("ltae_attention_train out", dtype, out_t, ref[0], yard[0], what=kind)
    _check("ltae_attention_train attn", dtype, attn_t, ref[1], yard[1], f32_out=True, what=kind)


@gpu
@DTYPES
@pytest.mark.parametrize("kind", PADS)
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_ltae_attention_forward(cuda, geom, kind, dtype):
    _attention_forward(cuda, geom, kind, dtype)


@gpu
def test_ltae_attention_forward_grid_stride(cuda):
    """B * P * NH > 4096 blocks x 128 threads: the forward kernels' grid-stride loop"""
    geom = (2, 2, 128 * 129, 16, 4, 16)
    assert geom[0] * geom[2] * geom[3] > 4096 * 128
    _attention_forward(cuda, geom, "some", F32)


def _attention_backward(cuda, geom, kind, dtype, variants):
    from flairhip import ops
    B, T = geom[:2]
    k, v, Q, dout, dattn_ext, drop = _attention_inputs(geom, dtype)
    pad = _pads(B, T, kind)
    kd, vd, Qd = _attention_dev(geom, k, v, Q, dtype, cuda)
    padd, doutd = _u8(pad, cuda), _dev(dout.reshape(B, *HW[geom[2]], -1), dtype, cuda)
    for with_drop, with_ext in variants:
        dr, ext = (drop if with_drop else None), (dattn_ext if with_ext else None)
        what = f"{kind} drop={with_drop} dattn_ext={with_ext}"
        ref = _attention_ref(k, v, Q, pad, dr, torch.float64, dout, ext)
        yard = _attention_ref(k, v, Q, pad, dr, F32, dout, ext)
        assert bool((ref[3][pad] == 0).all())  # the float64 dk of a padded date is exactly 0
        drd = None if dr is None else dr.to(cuda)
        out, attn, prob = ops.ltae_attention_train(kd, vd, Qd, padd, B, T, drd)
        _check("ltae_attention_train out", dtype, out, ref[0], yard[0], what=what)
        _check("ltae_attention_train attn", dtype, attn, ref[1], yard[1], f32_out=True, what=what)
        _check("ltae_attention_train prob", dtype, prob, ref[2], yard[2], f32_out=True, what=what)
        # prob as the float64 softmax rounded to f32: the backward kernel is checked on its own arithmetic
        probd = ref[2].float().contiguous().to(cuda)
        args = (kd, vd, Qd, padd, drd, probd, doutd, None if ext is None else ext.to(cuda), B, T)
        dk, dv, dq = ops.ltae_attention_bwd(*args)
        _check("ltae_attention_bwd dk", dtype, dk, ref[3], yard[3], what=what)
        _check("ltae_attention_bwd dv", dtype, dv, ref[4], yard[4], what=what)
        _check("ltae_attention_bwd dQ", dtype, dq, ref[5], yard[5], f32_out=True, what=what)
        assert bool((dk.float().cpu().reshape(ref[3].shape)[pad] == 0).all()), what
        dk2, dv2, _ = ops.ltae_attention_bwd(*args)  # dQ goes through LDS float atomics: never compared bitwise
        assert torch.equal(dk, dk2) and torch.equal(dv, dv2), what
        # and from the kernel's own prob, as the training step chains them
        dk, dv, dq = ops.ltae_attention_bwd(kd, vd, Qd, padd, drd, prob, *args[6:])
        _check("ltae_attention_bwd dk", dtype, dk, ref[3], yard[3], what=what + " (chained)")
        _check("ltae_attention_bwd dv", dtype, dv, ref[4], yard[4], what=what + " (chained)")
        _check("ltae_attention_bwd dQ", dtype, dq, ref[5], yard[5], f32_out=True, what=what + " (chained)")


@gpu
@DTYPES
@pytest.mark.parametrize("kind", PADS)
@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_ltae_attention_dropout_and_backward(cuda, geom, kind, dtype):
    _attention_backward(cuda, geom, kind, dtype, [(True, True), (True, False), (False, True)])


@gpu
def test_ltae_attention_backward_grid_stride(cuda):
    """B * P * NH > 1024 blocks x 128 threads: the backward's grid-stride loop, dQ accumulated in LDS across iterations"""
    geom = (2, 3, 65 * 65, 16, 4, 16)
    assert geom[0] * geom[2] * geom[3] > 1024 * 128
    _attention_backward(cuda, geom, "some", F32, [(True, True)])


# --------------------------------------------------------------------------------------------------
# temporal_aggregate, temporal_aggregate_bwd

@gpu
@DTYPES
@pytest.mark.parametrize("use_pad", [True, False])
@pytest.mark.parametrize("btp", [(2, 5, 77), (1, 1, 1), (3, 4, 9)], ids=str)
@pytest.mark.parametrize("C,NH", [(64, 16), (128, 16), (32, 4)])
def test_temporal_aggregate(cuda, C, NH, btp, use_pad, dtype):
    from flairhip import ops
    B, T, P = btp
    h, w = HW[P]
    g = torch.Generator().manual_seed(10)
    x = _quant(torch.randn(B, T, P, C, generator=g), dtype)
    dout = _quant(torch.randn(B, P, C, generator=g), dtype)
    attn = torch.rand(NH, B, T, P, generator=g) + 0.05  # not normalised, non-zero at the padded dates: use_pad matters
    pad = _pads(B, T, "some")
    ref = _aggregate_ref(x, attn, pad, use_pad, torch.float64, dout)
    yard = _aggregate_ref(x, attn, pad, use_pad, F32, dout)
    xd, attnd, padd = _dev(x.reshape(B * T, h, w, C), dtype, cuda), attn.to(cuda), _u8(pad, cuda)
    _check("temporal_aggregate", dtype, ops.temporal_aggregate(xd, attnd, padd, B, T, use_pad), ref[0], yard[0])
    dx, dattn = ops.temporal_aggregate_bwd(xd, attnd, padd, _dev(dout.reshape(B, h, w, C), dtype, cuda), B, T, use_pad)
    _check("temporal_aggregate_bwd dx", dtype, dx, ref[1], yard[1])
    _check("temporal_aggregate_bwd dattn", dtype, dattn, ref[2], yard[2], f32_out=True)
    dx, dattn = dx.float().cpu().reshape(B, T, P, C), dattn.cpu()
    if use_pad:
        assert bool((ref[1][pad] == 0).all()) and bool((ref[2][:, pad] == 0).all())
        assert bool((dx[pad] == 0).all()) and bool((dattn[:, pad] == 0).all())
    else:
        assert bool((dx[pad] != 0).any()) and bool((dattn[:, pad] != 0).any())


# --------------------------------------------------------------------------------------------------
# the wrappers refuse operands that would make a kernel read out of bounds

@gpu
def test_temporal_wrappers_refuse_bad_operands(cuda):
    from flairhip import ops
    B, T, h, w, NH, DK, DV, C = 2, 3, 2, 2, 4, 2, 4, 16
    N, P = B * T, h * w
    x = torch.randn(N, h, w, C, device=cuda)
    gamma, beta = torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    k, v, Q = torch.randn(N, h, w, NH * DK, device=cuda), torch.randn(N, h, w, NH * DV, device=cuda), torch.randn(NH, DK, device=cuda)
    pad = torch.zeros(N, dtype=torch.uint8, device=cuda)
    masks = torch.rand(NH, B, T, P, device=cuda)
    dout, dagg = torch.randn(B, h, w, NH * DV, device=cuda), torch.randn(B, h, w, C, device=cuda)

    def refused(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    # the operands above are accepted
    ops.group_norm(x, gamma, beta, 4, residual=x)
    ops.group_norm_seq(x, B, T, gamma, beta, 4)
    ops.group_norm_bwd(x, x, gamma, beta, 4)
    ops.group_norm_seq_bwd(x, x, B, T, gamma, beta, 4)
    ops.ltae_attention(k, v, Q, pad, B, T)
    ops.ltae_attention_train(k, v, Q, pad, B, T, masks)
    ops.ltae_attention_bwd(k, v, Q, pad, masks, masks, dout, masks, B, T)
    ops.temporal_aggregate(x, masks, pad, B, T, True)
    ops.temporal_aggregate_bwd(x, masks, pad, dagg, B, T, True)
    ops.mask_images_(x.clone(), pad, 0.0)

    # N != B * T
    for fn, args in ((ops.group_norm_seq, (x, B, T + 1, gamma, beta, 4)), (ops.group_norm_seq_bwd, (x, x, B, T + 1, gamma, beta, 4)),
                     (ops.ltae_attention, (k, v, Q, pad, B, T + 1)), (ops.ltae_attention_train, (k, v, Q, pad, B, T + 1)),
                     (ops.ltae_attention_bwd, (k, v, Q, pad, None, masks, dout, None, B, T + 1)),
                     (ops.temporal_aggregate, (x, masks, pad, B, T + 1, True)),
                     (ops.temporal_aggregate_bwd, (x, masks, pad, dagg, B, T + 1, True))):
        refused(r"leading size 6 is not B \* T = 8", fn, *args)

    # pad: dtype, length, layout, device
    for bad in (pad.bool(), pad.long(), pad[:-1], torch.zeros(2 * N, dtype=torch.uint8, device=cuda)[::2], pad.cpu()):
        for fn, args in ((ops.ltae_attention, (k, v, Q, bad, B, T)), (ops.ltae_attention_train, (k, v, Q, bad, B, T)),
                         (ops.ltae_attention_bwd, (k, v, Q, bad, None, masks, dout, None, B, T)),
                         (ops.temporal_aggregate, (x, masks, bad, B, T, True)),
                         (ops.temporal_aggregate_bwd, (x, masks, bad, dagg, B, T, True)),
                         (ops.mask_images_, (x.clone(), bad, 0.0))):
            refused(r"pad must be a contiguous uint8 tensor of B \* T = 6 elements", fn, *args)

    # gamma / beta: dtype, length, layout
    for bad in (gamma.bfloat16(), gamma[:-1], torch.ones(2 * C, device=cuda)[::2], gamma.cpu()):
        for name, pick in (("gamma", lambda: (bad, beta)), ("beta", lambda: (gamma, bad))):
            ga, be = pick()
            refused(f"group_norm: {name} must be contiguous f32 of 16 elements", ops.group_norm, x, ga, be, 4)
            refused(f"group_norm_seq: {name} must be contiguous f32 of 16", ops.group_norm_seq, x, B, T, ga, be, 4)
            refused(f"group_norm_bwd: {name} must be contiguous f32 of 16", ops.group_norm_bwd, x, x, ga, be, 4)
            refused(f"group_norm_seq_bwd: {name} must be contiguous f32 of 16", ops.group_norm_seq_bwd, x, x, B, T, ga, be, 4)
    refused("16 channels do not split into 3 groups", ops.group_norm, x, gamma, beta, 3)
    refused("residual must be contiguous", ops.group_norm, x, gamma, beta, 4, residual=x.bfloat16())
    refused("dy must be contiguous", ops.group_norm_bwd, x, x.bfloat16(), gamma, beta, 4)
    refused("dy must be contiguous", ops.group_norm_seq_bwd, x, x[:, :1], B, T, gamma, beta, 4)

    # Q and the channel counts
    attention = ((ops.ltae_attention, lambda q, kk=k, vv=v: (kk, vv, q, pad, B, T)),
                 (ops.ltae_attention_train, lambda q, kk=k, vv=v: (kk, vv, q, pad, B, T)),
                 (ops.ltae_attention_bwd, lambda q, kk=k, vv=v: (kk, vv, q, pad, None, masks, dout, None, B, T)))
    for fn, args in attention:
        refused("Q must be contiguous f32 of 8 elements", fn, *args(Q.bfloat16()))
        refused("Q must be contiguous f32 of 8 elements", fn, *args(Q.t().contiguous().t()))
        refused(r"Q must be \[n_head, d_k\]", fn, *args(Q.reshape(-1)))
        refused("inconsistent shapes", fn, *args(torch.randn(NH, DK + 1, device=cuda)))           # k channels != n_head * d_k
        refused("inconsistent shapes", fn, *args(Q, vv=torch.randn(N, h, w, NH * DV + 1, device=cuda)))  # v channels % n_head
        refused("inconsistent shapes", fn, *args(Q, vv=v.bfloat16()))
    refused("32 channels do not split into 5 heads", ops.temporal_aggregate, torch.randn(N, h, w, 32, device=cuda),
            torch.rand(5, B, T, P, device=cuda), pad, B, T, True)
    refused("32 channels do not split into 5 heads", ops.temporal_aggregate_bwd, torch.randn(N, h, w, 32, device=cuda),
            torch.rand(5, B, T, P, device=cuda), pad, torch.randn(B, h, w, 32, device=cuda), B, T, True)

    # the register arrays of the training pair
    k9, Q9 = torch.randn(N, h, w, NH * 9, device=cuda), torch.randn(NH, 9, device=cuda)
    v33, dout33 = torch.randn(N, h, w, NH * 33, device=cuda), torch.randn(B, h, w, NH * 33, device=cuda)
    refused("d_k = 9, d_v = 4 exceed", ops.ltae_attention_train, k9, v, Q9, pad, B, T)
    refused("d_k = 9, d_v = 4 exceed", ops.ltae_attention_bwd, k9, v, Q9, pad, None, masks, dout, None, B, T)
    refused("d_k = 2, d_v = 33 exceed", ops.ltae_attention_train, k, v33, Q, pad, B, T)
    refused("d_k = 2, d_v = 33 exceed", ops.ltae_attention_bwd, k, v33, Q, pad, None, masks, dout33, None, B, T)

    # drop / prob / dattn_ext / attn: contiguous f32 [n_head, B, T, h*w]
    for bad in (masks.bfloat16(), masks[:, :, :, :-1], masks.permute(1, 0, 2, 3), masks.reshape(NH, B, T, h, w),
                torch.rand(NH, B, T, 2 * P, device=cuda)[..., ::2], masks.cpu()):
        shape = r"contiguous f32 \[n_head, B, T, h\*w\] = \[4, 2, 3, 4\]"
        refused("ltae_attention_train: drop must be " + shape, ops.ltae_attention_train, k, v, Q, pad, B, T, bad)
        refused("ltae_attention_bwd: drop must be " + shape, ops.ltae_attention_bwd, k, v, Q, pad, bad, masks, dout, None, B, T)
        refused("ltae_attention_bwd: prob must be " + shape, ops.ltae_attention_bwd, k, v, Q, pad, None, bad, dout, None, B, T)
        refused("ltae_attention_bwd: dattn_ext must be " + shape, ops.ltae_attention_bwd, k, v, Q, pad, None, masks, dout, bad, B, T)
        if bad.dim() == 4 and bad.shape[0] == NH:
            refused("temporal_aggregate: attn must be " + shape, ops.temporal_aggregate, x, bad, pad, B, T, True)
            refused("temporal_aggregate_bwd: attn must be " + shape, ops.temporal_aggregate_bwd, x, bad, pad, dagg, B, T, True)
    refused(r"attn must be \[n_head, B, T, h\*w\]", ops.temporal_aggregate, x, masks.reshape(NH, B, T, h, w), pad, B, T, True)
    refused("ltae_attention_bwd: dout must be contiguous", ops.ltae_attention_bwd, k, v, Q, pad, None, masks, dout[:1], None, B, T)
    refused("temporal_aggregate_bwd: dout must be contiguous", ops.temporal_aggregate_bwd, x, masks, pad, dagg.bfloat16(), B, T, True)
