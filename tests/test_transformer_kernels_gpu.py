"""Every Swin-Transformer / UPerNet token kernel (csrc/gemm.hip, csrc/transformer.hip) on its own against float64.

Each GPU test calls one flairhip.ops wrapper and compares it with a float64 restatement of the operation in plain torch on
the CPU (torch autograd in float64 for the backward kernels; window attention is timm's formula as oracle/swin_upernet.py
states it).  Inputs are quantised to the storage type (f32 or bf16) first and handed to both sides.

Tolerances (the scheme of tests/test_temporal_kernels_gpu.py; none of them is fitted to what the kernels give):
  f32 storage, and the f32 outputs of bf16 calls   16 x the maximum error of the same formula run in float32 on the CPU
                against float64, floor 2^-20 * max(1, max |ref|)                                    ("the f32 bound")
  bf16-stored outputs   per element |got - ref| <= 2^-8 |ref| + the f32 bound + sum_t 2^-8 A_t, one A_t for every
                intermediate bf16 rounding of a quantity t that then enters the output linearly: A_t is that linear map
                applied to absolute values in float64 (the `a` of tests/insitu.py)
Rounding points read from the kernels (each is an `extra` term below):
  gemm_bf16_kernel<2|4>, gemm256_bf16_kernel   (R1) bias + accumulator (after ReLU, or GELU when no aux is kept) is packed
                to bf16 into the LDS epilogue tile; when a residual, row_scale or aux is present it is unpacked again and
                GELU / GELU'(aux) / row_scale / residual are applied to the ROUNDED value before the second, output
                rounding: A = |sc| |act(pre)|, A = |sc| |gelu'(pre)| |pre| through the GELU (plus the second-order term
                0.4 (2^-8 pre)^2, |gelu''| <= 0.8), A = |sc| |gelu'(aux)| |pre| for DGELU.  (R2) the stored pre-activation
                aux is that same rounded value: one output rounding, no extra term.
                The bf16 epilogues evaluate Phi by a polynomial fit (gemm_phi_minus_half2): GELU_FIT / DGELU_FIT below are
                its approximation errors against erf, measured in float64 on the CPU by test_gelu_fit_constants (not a
                rounding, so not a 2^-8 term): + |sc| GELU_FIT, + |sc| |pre| DGELU_FIT.
  window_attention_bf16_kernel   (R3) the unnormalised probabilities e = 2^(s - max) are rounded to bf16 for the PV MFMA
                and divided by the f32 sum of the unrounded ones: A = softmax(s) . |v|.  Padding tokens' q / k / v are the
                qkv bias rounded to bf16 "like every other element of the qkv tensor": the reference takes the rounded
                bias for them (that is the operation, not an error).
  window_attention_bwd_kernel    (R4) pass A rounds dS to bf16 for dQ = scale dS K: A = scale |dS| . |k|; pass B rounds P
                and dS for dV = P^T dO and dK = scale dS^T Q: A = P^T . |dO|, A = scale |dS|^T . |q|.  dtable is summed from
                the f32 dS (f32 bound alone).  Unlisted in the issue, found in store_grad(): the padding tokens' dq / dk / dv
                that make dbias_pad are the very MFMA results of the rounded P / dS, so dbias_pad (f32, no output rounding)
                carries the A terms of its padding tokens, summed.
  every other kernel keeps f32 between its bf16 load and its one bf16 store.
The CPU tests of this module put f32 torch emulations that round at exactly these points through the same _check
(test_emulation_*: they must stay inside the bounds), and mutants of them that must fail (test_mutant_*).

Wrappers of the "Swin-Transformer / UPerNet" block of flairhip/ops.py, their kernels, the tests that call them, and what one
MI355X run of this module measured: largest |got - ref| / max(1, max |ref|) over the cases, and that error as a fraction
of its bound.
  wrapper (kernels)                                       test                                  f32 storage     bf16 storage
  linear, f32 (gemm_f32_kernel, plan 0)                   test_linear_f32                 out   5.5e-07  0.15   (f32 only)
                                                                                          aux   3.4e-07  0.12
  linear, bf16 (gemm_bf16_kernel<2>, plan 1)              test_linear_bf16      one rounding                    3.3e-03  0.99
                                                                                    two-step                    5.4e-03  0.99
                                                                                          aux                   2.5e-03  0.99
  linear, bf16 (gemm_bf16_kernel<4>, plan 2)              test_linear_bf16      one rounding                    2.8e-03  0.99
                                                                                    two-step                    5.1e-03  0.99
                                                                                          aux                   2.2e-03  0.99
  linear, bf16 (gemm256_bf16_kernel, plan 3)              test_linear_bf16      one rounding                    2.9e-03  0.99
                                                                                    two-step                    5.5e-03  0.99
                                                                                          aux                   2.2e-03  0.99
  linear_wgrad (gemm_tn_f32_kernel | gemm_tn_bf16_kernel, test_linear_wgrad               dW    3.0e-07  0.07   1.5e-07  0.06
                gemm_tn_reduce_kernel)                                                    db    3.4e-07  0.13   8.5e-08  0.08
  space_to_depth (space_to_depth_kernel)                  test_space_to_depth                   exact           exact
  layer_norm (layer_norm_kernel<false>, six lane cases)   test_layer_norm,                y     1.6e-07  0.10   3.7e-03  0.99
                                                          test_layer_norm_capped_chunks,  mean  1.2e-07  0.08   6.2e-08  0.06
                                                          test_layer_norm_constant_row    rstd  7.7e-08  0.08   9.3e-08  0.07
  layer_norm_bwd (layer_norm_bwd_kernel<false>,           the same three tests            dx    1.6e-07  0.12   3.2e-03  0.99
                  layer_norm_bwd_params_kernel<false>,                                  dgamma  1.6e-07  0.09   1.5e-07  0.08
                  layer_norm_bwd_reduce_kernel)                                          dbeta  1.5e-07  0.10   3.9e-08  0.04
  patch_merge_norm (layer_norm_kernel<true>)              test_patch_merge_norm           y     1.2e-07  0.08   2.9e-03  0.99
                                                                                          mean  7.3e-08  0.07   4.8e-08  0.05
                                                                                          rstd  6.4e-08  0.07   6.6e-08  0.07
  patch_merge_norm_bwd (layer_norm_bwd_kernel<true>,      test_patch_merge_norm           dx    1.5e-07  0.10   3.4e-03  0.99
                        layer_norm_bwd_params_kernel<true>, layer_norm_bwd_reduce_kernel) dgamma 1.4e-07 0.07   1.5e-07  0.08
                                                                                         dbeta  1.5e-07  0.07   3.7e-08  0.04
  window_attention (window_attention_f32_kernel |         test_window_attention,                6.4e-07  0.13   3.9e-03  0.81
                    window_attention_bf16_kernel<4,4>, <10,3>)  test_window_attention_map_smaller_than_the_window
  window_attention_bwd (window_attention_bwd_f32_kernel | the same two tests              dqkv  7.7e-07  0.19   5.8e-03  0.87
                        window_attention_bwd_kernel<4,4>, <10,3>, column_sums_kernel,   dtable  5.3e-07  0.18   5.7e-07  0.26
                        column_sums_reduce_kernel, zero_f32_kernel)                  dbias_pad  3.2e-07  0.24   1.6e-03  0.66
  gelu (gelu_kernel)                                      test_gelu                             4.6e-08  0.05   9.7e-04  0.97
  adaptive_avg_pool (adaptive_avg_pool_kernel)            test_adaptive_avg_pool                1.8e-07  0.11   3.0e-03  0.99
  adaptive_avg_pool_bwd (adaptive_avg_pool_bwd_kernel)    test_adaptive_avg_pool                9.4e-08  0.07   3.3e-03  0.99
  bilinear_slice (bilinear_slice_kernel)                  test_bilinear_slice                   2.4e-07  0.07   3.2e-03  0.99
  bilinear_slice_bwd (bilinear_slice_bwd_kernel)          test_bilinear_slice                   2.0e-07  0.06   2.9e-03  0.94
  scale_rows (scale_rows_kernel)                          test_scale_rows                       4.1e-08  0.04   3.0e-03  0.93
  column_sums (column_sums_kernel, column_sums_reduce_kernel)  test_column_sums                 1.1e-07  0.07   1.8e-07  0.06
  updown2x_slice (blur3_slice_kernel)                     test_updown2x_slice                   7.5e-08  0.05   2.2e-03  0.98
  linear_plan (host only)                                 every test_linear* case asserts it
The f32 kernels stay within 0.25 of bounds that are themselves 1e-6 to 1e-5.  bf16-stored outputs sit at 0.99 of their
bound because one bf16 rounding alone errs by up to 2^-8 of the value at the bottom of a binade, and over 10^4 to 10^7
elements each term of the bound is met on its own: the output rounding where the extra terms vanish, the (R1) rounding where
the residual cancels the product.  The CPU emulations give the same figures (linear 0.96 to 0.99 at every shape; attention
out 0.51 to 0.81, dqkv 0.70 to 0.87, dbias_pad 0.05 to 0.65 over the windows), so no exact emulation can stay under half
of this bound; the kernels' attention figures are those of the emulation to three digits.  No bound was moved, and no case
exceeded its bound on the GPU.  test_linear_wgrad's accumulate + with_bias case found ops.linear_wgrad adding the bias
gradient to an uninitialised tensor: the wrapper now starts it from 0.
Kernels of the two files not in the table: none.  zero_f32_kernel is the dbias_pad = 0 path of window_attention_bwd (maps
without padding, asserted exactly 0); column_sums_reduce_kernel / gemm_tn_reduce_kernel / layer_norm_bwd_*_kernel run inside
the wrappers listed with them.  The wrapper's output of window_attention has no padding positions (padding queries are
dropped in the kernel), so "untouched" is checked as: every real position is written (the output is pre-allocated by the
wrapper, finite and within bounds everywhere).
"""
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
EPS = 1e-5
ACT_NONE, ACT_GELU, ACT_DGELU, ACT_RELU = 0, 1, 2, 3
U = 2.0 ** -8  # largest relative error of one bf16 rounding
# approximation error of the bf16 GEMM epilogue's polynomial Phi (csrc/gemm.hip) against erf: in gelu(x) = x Phi(x) and in
# gelu'(x) = Phi(x) + x phi(x); test_gelu_fit_constants derives both in float64 from the polynomial itself
GELU_FIT, DGELU_FIT = 7.2e-5, 1.8e-5

_measured = {}  # (kernel, storage) -> largest error as a fraction of its bound, largest error relative to max(1, |ref|)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (kernel, storage), (frac, rel) in sorted(_measured.items()):
        print(f"\nMEASURED {kernel:44s} {storage:5s} {rel:9.2e} of max(1, max|ref|)   {frac:6.3f} of the bound", end="")


def _quant(t, dtype):
    """values of the storage type, held in f32"""
    return t.to(dtype).float()


def _dev(t, dtype, cuda):
    return t.to(dtype).contiguous().to(cuda)


def _f32_bound(ref, yard):
    """16 x the error of the float32 CPU run of the same formula, floor 2^-20 max(1, max |ref|)"""
    assert yard.dtype == torch.float32 and ref.dtype == torch.float64 and yard.shape == ref.shape
    return max(16.0 * (yard.double() - ref).abs().max().item(), 2.0 ** -20 * max(1.0, ref.abs().max().item()))


def _check(kernel, dtype, got, ref, yard, f32_out=False, what="", extra=None):
    """got (ref's layout up to a reshape) against the float64 ref within the module's bounds; extra: sum_t 2^-8 A_t (and
    the fit terms) of a bf16 call, per element, already scaled"""
    storage = "bf16" if dtype == BF16 else "f32"
    assert got.dtype == (F32 if f32_out else dtype), (kernel, what, got.dtype)
    got = got.detach().cpu().double().reshape(ref.shape)
    bound = _f32_bound(ref, yard)
    lim = torch.full_like(ref, bound)
    if dtype == BF16 and not f32_out:
        lim = lim + U * ref.abs()
    if dtype == BF16 and extra is not None:
        lim = lim + extra.reshape(ref.shape)
    err = (got - ref).abs()
    frac = (err / lim).max().item()
    rel = err.max().item() / max(1.0, ref.abs().max().item())
    old = _measured.get((kernel, storage), (0.0, 0.0))
    _measured[(kernel, storage)] = (max(old[0], frac), max(old[1], rel))
    assert torch.isfinite(got).all() and bool((err <= lim).all()), \
        f"{kernel} {storage} {what}: max error {err.max().item():.3e}, {frac:.2f} of the bound (f32 part {bound:.3e})"


def _fails(*args, **kw):
    """a mutant must be refused by _check"""
    try:
        _check(*args, **kw)
    except AssertionError:
        return True
    return False


def _bf(t):
    return t.to(BF16).float()


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


# --------------------------------------------------------------------------------------------------
# token GEMM: linear

# (M, K, N) -> plan: 1 gemm_bf16_kernel<2>, 2 gemm_bf16_kernel<4>, 3 gemm256_bf16_kernel (ops.linear_plan asserts it)
BF16_GEMMS = [((72, 32, 8), 1), ((129, 64, 264), 1), ((300, 128, 384), 1),
              ((6107, 64, 1016), 2),          # 48 x 8 = 384 blocks, M tail and N tail, K < 256
              ((12288 + 40, 256, 520), 2),    # K >= 256 but 49 x 3 < 240 blocks of 256
              ((61340, 256, 232), 3),         # 240 x 1 blocks, M tail and N tail
              ((15260, 288, 1000), 3),        # 60 x 4 blocks, K no multiple of 64
              ((15360, 1024, 1024), 3)]       # aligned, deep K
F32_GEMMS = [(70, 128, 8), (333, 200, 136), (65, 7, 9)]
# name, bias, act, aux kept (GELU) / supplied (DGELU), residual, in place, row_scale's rows_per_scale (0: none)
EPILOGUES = [("plain", False, ACT_NONE, False, False, False, 0), ("bias", True, ACT_NONE, False, False, False, 0),
             ("gelu", True, ACT_GELU, False, False, False, 0), ("gelu+aux", True, ACT_GELU, True, False, False, 0),
             ("dgelu", False, ACT_DGELU, True, False, False, 0), ("relu", True, ACT_RELU, False, False, False, 0),
             ("residual", True, ACT_NONE, False, True, False, 0), ("residual in place", False, ACT_NONE, False, True, True, 0),
             ("row_scale", True, ACT_NONE, False, True, False, 64),       # a dropped sample: rows = the residual
             ("row_scale 37", True, ACT_GELU, True, True, False, 37)]     # 37 divides no tile height (64, 128, 256)


def _linear_inputs(shape, dtype):
    M, K, N = shape
    g = torch.Generator().manual_seed(M * 7 + K * 3 + N)
    x = _quant(torch.randn(M, K, generator=g), dtype)
    w = _quant(torch.randn(N, K, generator=g) / math.sqrt(K), dtype)
    bias = torch.randn(N, generator=g)
    res = _quant(torch.randn(M, N, generator=g), dtype)
    aux = _quant(torch.randn(M, N, generator=g) * 1.5, dtype)
    return x, w, bias, res, aux


def _row_scale(M, rps):
    """DropPath factors 0 or 1 / 0.8 per group of rps rows; the second group (or the only one's neighbour) is dropped"""
    n = -(-M // rps)
    sc = torch.full((n,), 1.25)
    sc[min(1, n - 1)] = 0.0
    if n > 3:
        sc[n - 1] = 0.0  # the ragged last group
    return sc


def _linear_ref(acc, bias, act, aux, sc, res, dt, memo=None):
    """acc = x w^T in dt -> (pre-activation, activation, output) of ffa_linear_ex's epilogue order; memo keeps the
    activations of one shape across its epilogues"""
    key = (bias is not None, act, dt)
    if memo is not None and key in memo:
        pre, y = memo[key]
    else:
        pre = acc if bias is None else acc + bias.to(dt)
        if act == ACT_GELU:
            y = _gelu(pre)
        elif act == ACT_DGELU:
            y = pre * _dgelu(aux.to(dt))
        elif act == ACT_RELU:
            y = F.relu(pre)
        else:
            y = pre
        if memo is not None:
            memo[key] = (pre, y)
    out = y
    if sc is not None:
        out = out * sc.to(dt)[:, None]
    if res is not None:
        out = out + res.to(dt)
    return pre, y, out


def _linear_extra(pre, y, act, keep_aux, aux, sc, two_step):
    """the bf16 kernels' (R1) term and the polynomial-fit terms, float64"""
    s = torch.ones(pre.shape[0], 1, dtype=F64) if sc is None else sc.double().abs()[:, None]
    extra = torch.zeros_like(pre)
    if two_step:
        if act == ACT_GELU and keep_aux:
            extra = U * s * _dgelu(pre).abs() * pre.abs() + s * 0.4 * (U * pre) ** 2
        elif act == ACT_DGELU:
            extra = U * s * _dgelu(aux.double()).abs() * pre.abs()
        else:
            extra = U * s * y.abs()
    if act == ACT_GELU:
        extra = extra + s * GELU_FIT
    elif act == ACT_DGELU:
        extra = extra + s * pre.abs() * DGELU_FIT
    return extra


def _linear_emulate(acc, bias, act, keep_aux, aux, sc, res, bias_shift_from=None):
    """the bf16 kernels' epilogue in f32 torch, rounding where they round; acc = x w^T in f32 -> (out, aux) bf16"""
    v = acc
    if bias is not None:
        b = bias.clone()
        if bias_shift_from is not None:  # mutant: the bias read one column off in the N-tail tile
            b[bias_shift_from:] = torch.roll(bias, 1)[bias_shift_from:]
        v = v + b
    if act == ACT_RELU:
        v = F.relu(v)
    if act == ACT_GELU and not keep_aux:
        v = _gelu(v)
    t = v.to(BF16)                                                     # (R1)
    if res is None and sc is None and not (keep_aux or act == ACT_DGELU):
        return t, None
    o, kept = t.float(), None
    if act == ACT_GELU and keep_aux:
        kept, o = t, _gelu(o)                                          # (R2)
    elif act == ACT_DGELU:
        o = o * _dgelu(aux.float())
    if sc is not None:
        o = o * sc[:, None]
    if res is not None:
        o = o + res
    return o.to(BF16), kept


def _linear_case(shape, dtype, run, name):
    """every epilogue of one shape through `run(x, w, bias, act, aux_in, keep_aux, res, in_place, sc, rps, acc32) ->
    (out, kept aux or None)`; the float64 / float32 products are formed once"""
    x, w, bias, res, aux = _linear_inputs(shape, dtype)
    M = shape[0]
    acc64, acc32, memo = x.double() @ w.double().t(), x @ w.t(), {}
    for ep, use_bias, act, use_aux, use_res, in_place, rps in EPILOGUES:
        if in_place and dtype == F32:
            continue
        b = bias if use_bias else None
        sc = _row_scale(M, rps) if rps else None
        rows = None if sc is None else sc.repeat_interleave(rps)[:M]
        r = res if use_res else None
        keep_aux = use_aux and act == ACT_GELU
        a_in = aux if act == ACT_DGELU else None
        ref = _linear_ref(acc64, b, act, a_in, rows, r, F64, memo)
        yard = _linear_ref(acc32, b, act, a_in, rows, r, F32, memo)
        out, kept = run(x, w, b, act, a_in, keep_aux, r, in_place, sc, rps, acc32)
        extra, label = None, name
        if dtype == BF16:
            two_step = r is not None or sc is not None or use_aux  # the kernels' second epilogue pass, after (R1)
            extra = _linear_extra(ref[0], ref[1], act, keep_aux, a_in, rows, two_step)
            label = name + (" two-step" if two_step else "")
        _check(label, dtype, out, ref[2], yard[2], what=f"{shape} {ep}", extra=extra)
        if keep_aux:
            _check(name + " aux", dtype, kept, ref[0], yard[0], what=f"{shape} {ep}")
        if rows is not None:  # a dropped sample's rows are the residual, bit for bit
            dropped = rows == 0
            assert bool(dropped.any()) and torch.equal(out.float().cpu()[dropped], r[dropped]), (shape, ep)


def _linear_gpu(cuda, dtype):
    from flairhip import ops

    operands = {}

    def run(x, w, b, act, a_in, keep_aux, r, in_place, sc, rps, acc32):
        if "x" not in operands:  # one shape per _linear_case: uploaded once
            operands["x"], operands["w"] = _dev(x, dtype, cuda), _dev(w, dtype, cuda)
        xd, wd = operands["x"], operands["w"]
        rd = None if r is None else _dev(r, dtype, cuda)
        aux = _dev(a_in, dtype, cuda) if a_in is not None else None
        if keep_aux:
            aux = torch.full((x.shape[0], w.shape[0]), float("nan"), dtype=dtype, device=cuda)
        out = ops.linear(xd, wd, None if b is None else b.to(cuda), act=act, residual=rd, out=rd if in_place else None,
                         aux=aux, row_scale=None if sc is None else sc.to(cuda), rows_per_scale=rps)
        if in_place:
            assert out.data_ptr() == rd.data_ptr()
        return out, (aux if keep_aux else None)
    return run


@gpu
@pytest.mark.parametrize("shape,plan", BF16_GEMMS, ids=lambda v: str(v))
def test_linear_bf16(cuda, shape, plan):
    from flairhip import ops
    assert ops.linear_plan(BF16, *shape) == plan
    _linear_case(shape, BF16, _linear_gpu(cuda, BF16), f"linear (plan {plan})")


@gpu
@pytest.mark.parametrize("shape", F32_GEMMS, ids=str)
def test_linear_f32(cuda, shape):
    from flairhip import ops
    assert ops.linear_plan(F32, *shape) == 0
    _linear_case(shape, F32, _linear_gpu(cuda, F32), "linear (plan 0)")


def _emulated_linear(skip_k_from_row=None, bias_shift_from=None):
    def run(x, w, b, act, a_in, keep_aux, r, in_place, sc, rps, acc32):
        acc = acc32
        if skip_k_from_row is not None:  # mutant: the M-tail tile never sees the last 32-wide K block
            acc = acc32.clone()
            acc[skip_k_from_row:] = x[skip_k_from_row:, :-32] @ w[:, :-32].t()
        rows = None if sc is None else sc.repeat_interleave(rps)[:x.shape[0]]
        return _linear_emulate(acc, b, act, keep_aux, a_in, rows, r, bias_shift_from)
    return run


@pytest.mark.parametrize("shape,plan", BF16_GEMMS[:5], ids=lambda v: str(v))
def test_emulation_linear_bf16(shape, plan):
    """CPU: an f32 GEMM that rounds at (R1) / (R2) stays inside the bf16 bounds at every epilogue (the three plan-3
    shapes run the same epilogue code on more rows; they were put through this once, figures in the commit message)"""
    _linear_case(shape, BF16, _emulated_linear(), "emulation linear")


def test_mutant_linear():
    """CPU: a GEMM that skips the last 32-wide K block in the M-tail tile, and one that reads the bias one column off in the
    N-tail tile, are refused"""
    shape = (129, 64, 264)  # plan 1: 64-token tiles, the tail tile is row 128; the N-tail tile starts at column 256
    with pytest.raises(AssertionError, match="linear"):
        _linear_case(shape, BF16, _emulated_linear(skip_k_from_row=128), "mutant linear")
    with pytest.raises(AssertionError, match="bias"):
        _linear_case(shape, BF16, _emulated_linear(bias_shift_from=256), "mutant linear")
    for key in [k for k in _measured if k[0].startswith("mutant")]:
        del _measured[key]


def test_gelu_fit_constants():
    """CPU, float64: the polynomial Phi of the bf16 GEMM epilogues (coefficients of gemm_phi_minus_half2) against erf"""
    coef = [4.234514475e-11, -4.329148151e-09, 1.947642545e-07, -5.124695235e-06, 8.877788787e-05, -1.084315358e-03,
            9.749136865e-03, -6.626226753e-02, 3.988730609e-01]
    x = torch.linspace(-12.0, 12.0, 240001, dtype=F64)
    xc = x.clamp(-4.4, 4.4)
    q = torch.zeros_like(x)
    for c in coef:
        q = q * xc * xc + c
    phi = xc * q + 0.5
    assert (x * phi - _gelu(x)).abs().max().item() <= GELU_FIT
    assert (phi + x * torch.exp(-0.5 * x * x) * 0.3989422804014327 - _dgelu(x)).abs().max().item() <= DGELU_FIT


# --------------------------------------------------------------------------------------------------
# linear_wgrad

@gpu
@DTYPES
@pytest.mark.parametrize("KN", [(8, 8), (96, 288), (200, 136), (768, 96)], ids=str)
@pytest.mark.parametrize("M", [1, 70, 333, 4096 + 17])
def test_linear_wgrad(cuda, M, KN, dtype):
    from flairhip import ops
    K, N = KN
    g = torch.Generator().manual_seed(M + 5 * K + N)
    x, dy = _quant(torch.randn(M, K, generator=g), dtype), _quant(torch.randn(M, N, generator=g), dtype)
    base = torch.randn(N, K, generator=g)
    ref, yard = dy.double().t() @ x.double(), dy.t() @ x
    refb, yardb = dy.double().sum(0), dy.sum(0)
    xd, dyd = _dev(x, dtype, cuda), _dev(dy, dtype, cuda)
    dw = ops.linear_wgrad(xd, dyd)
    _check("linear_wgrad dW", dtype, dw, ref, yard, f32_out=True)
    dw2, db = ops.linear_wgrad(xd, dyd, with_bias=True)
    assert torch.equal(dw, dw2) and torch.equal(dw, ops.linear_wgrad(xd, dyd))  # deterministic split and reduction
    _check("linear_wgrad db", dtype, db, refb, yardb, f32_out=True)
    out = base.to(cuda)
    got = ops.linear_wgrad(xd, dyd, out=out, accumulate=True)
    assert got.data_ptr() == out.data_ptr()
    _check("linear_wgrad dW", dtype, got, ref + base.double(), yard + base, f32_out=True, what="accumulate")
    _, db2 = ops.linear_wgrad(xd, dyd, out=base.to(cuda), accumulate=True, with_bias=True)  # db starts from 0
    _check("linear_wgrad db", dtype, db2, refb, yardb, f32_out=True, what="accumulate")


# --------------------------------------------------------------------------------------------------
# LayerNorm, PatchMerging's gather + LayerNorm

# C / 8 pieces -> (lanes per row, pieces per lane): the largest C of each case and one that leaves masked lanes
LN_CS = [8, 96, 128, 136, 256, 264, 512, 520, 1024, 1032, 2048, 2056, 4096]


def _ln_ref(x, gamma, beta, dt, dy=None, dres=None, uncentred=False):
    """nn.LayerNorm over the last dimension -> y, mean, rstd [, dx, dgamma, dbeta]; dres: the gradient of a residual
    connection around the normalised branch, added to dx"""
    x, gamma, beta = (t.to(dt).clone().requires_grad_(dy is not None) for t in (x, gamma, beta))
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) if uncentred else ((x - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(EPS, dtype=F32).to(dt))
    y = (x - mean) * rstd * gamma + beta
    res = [y.detach(), mean.detach().squeeze(-1), rstd.detach().squeeze(-1)]
    if dy is not None:
        loss = (y * dy.to(dt)).sum()
        if dres is not None:
            loss = loss + (x * dres.to(dt)).sum()
        loss.backward()
        res += [x.grad, gamma.grad, beta.grad]
    return res


def _ln_inputs(rows, C, dtype, seed=11):
    g = torch.Generator().manual_seed(seed + C)
    x = _quant(torch.randn(rows, C, generator=g) * 2 + 0.5, dtype)
    dy, dres = _quant(torch.randn(rows, C, generator=g), dtype), _quant(torch.randn(rows, C, generator=g), dtype)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    return x, dy, dres, gamma, beta


def _layer_norm_gpu(cuda, rows, C, dtype, x=None, what=""):
    from flairhip import ops
    x0, dy, dres, gamma, beta = _ln_inputs(rows, C, dtype)
    x = x0 if x is None else x
    xd, dyd, drd, gd, bd = _dev(x, dtype, cuda), _dev(dy, dtype, cuda), _dev(dres, dtype, cuda), gamma.to(cuda), beta.to(cuda)
    what = f"rows={rows} C={C} {what}"
    for with_res in (False, True):
        ref = _ln_ref(x, gamma, beta, F64, dy, dres if with_res else None)
        yard = _ln_ref(x, gamma, beta, F32, dy, dres if with_res else None)
        if not with_res:
            stats = torch.full((rows, 2), float("nan"), device=cuda)
            y = ops.layer_norm(xd, gd, bd, stats=stats)
            _check("layer_norm", dtype, y, ref[0], yard[0], what=what)
            assert torch.equal(y, ops.layer_norm(xd, gd, bd)), what  # stats absent: the same output
            _check("layer_norm mean", dtype, stats[:, 0], ref[1], yard[1], f32_out=True, what=what)
            _check("layer_norm rstd", dtype, stats[:, 1], ref[2], yard[2], f32_out=True, what=what)
        stats64 = torch.stack([ref[1], ref[2]], dim=1).float().contiguous().to(cuda)  # the float64 statistics, as f32
        dx, dg, db = ops.layer_norm_bwd(xd, dyd, gd, stats64, dres=drd if with_res else None)
        _check("layer_norm_bwd dx", dtype, dx, ref[3], yard[3], what=f"{what} dres={with_res}")
        _check("layer_norm_bwd dgamma", dtype, dg, ref[4], yard[4], f32_out=True, what=what)
        _check("layer_norm_bwd dbeta", dtype, db, ref[5], yard[5], f32_out=True, what=what)


@gpu
@DTYPES
@pytest.mark.parametrize("C", LN_CS)
def test_layer_norm(cuda, C, dtype):
    for rows in (1, 70):
        _layer_norm_gpu(cuda, rows, C, dtype)


@gpu
@DTYPES
def test_layer_norm_capped_chunks(cuda, dtype):
    """rows = 256 * 512 + 3: the dgamma / dbeta chunk count is capped at 512 and the last chunks are empty"""
    _layer_norm_gpu(cuda, 256 * 512 + 3, 8, dtype)


@gpu
@DTYPES
@pytest.mark.parametrize("C", [8, 136, 4096])
def test_layer_norm_constant_row(cuda, C, dtype):
    """variance 0: rstd comes from eps alone (316.2), y = beta on that row; kept apart because that row's rstd and dx set
    max |ref|, which would loosen the floor for ordinary rows"""
    x = _ln_inputs(3, C, dtype)[0]
    x[1] = 1.5
    _layer_norm_gpu(cuda, 3, C, dtype, x=x, what="constant row")


def _merge(x):
    """timm PatchMerging.forward's gather: [B,H,W,C] -> [B,H/2,W/2,4C]"""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 4, 2, 5).flatten(3)


@gpu
@DTYPES
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("hw", [(2, 2), (8, 12), (2, 14)], ids=str)
@pytest.mark.parametrize("C", [8, 96, 192, 1024])
def test_patch_merge_norm(cuda, C, hw, B, dtype):
    from flairhip import ops
    (H, W), rows = hw, B * (hw[0] // 2) * (hw[1] // 2)
    g = torch.Generator().manual_seed(13 + C + H)
    x = _quant(torch.randn(B, H, W, C, generator=g) * 2 + 0.5, dtype)
    dy = _quant(torch.randn(B, H // 2, W // 2, 4 * C, generator=g), dtype)
    gamma, beta = torch.rand(4 * C, generator=g) + 0.5, torch.randn(4 * C, generator=g)

    def run(dt):
        xx = x.to(dt).clone().requires_grad_()
        r = _ln_ref(_merge(xx).detach().reshape(rows, 4 * C), gamma, beta, dt, dy.reshape(rows, 4 * C))
        _merge(xx).backward(r[3].reshape(B, H // 2, W // 2, 4 * C))  # the gather's transpose: every element once
        return r[:3] + [xx.grad] + r[4:]

    ref, yard = run(F64), run(F32)
    xd, gd, bd = _dev(x, dtype, cuda), gamma.to(cuda), beta.to(cuda)
    stats = torch.full((rows, 2), float("nan"), device=cuda)
    y = ops.patch_merge_norm(xd, gd, bd, stats=stats)
    assert y.shape == (B, H // 2, W // 2, 4 * C) and torch.equal(y, ops.patch_merge_norm(xd, gd, bd))
    _check("patch_merge_norm", dtype, y, ref[0], yard[0])
    _check("patch_merge_norm mean", dtype, stats[:, 0], ref[1], yard[1], f32_out=True)
    _check("patch_merge_norm rstd", dtype, stats[:, 1], ref[2], yard[2], f32_out=True)
    stats64 = torch.stack([ref[1], ref[2]], dim=1).float().contiguous().to(cuda)
    dx, dg, db = ops.patch_merge_norm_bwd(xd, _dev(dy, dtype, cuda), gd, stats64)
    _check("patch_merge_norm_bwd dx", dtype, dx, ref[3], yard[3])
    _check("patch_merge_norm_bwd dgamma", dtype, dg, ref[4], yard[4], f32_out=True)
    _check("patch_merge_norm_bwd dbeta", dtype, db, ref[5], yard[5], f32_out=True)


def test_mutant_layer_norm():
    """CPU: a variance that is not centred and a backward that drops dres are refused (f32 and bf16 storage)"""
    for dtype in (F32, BF16):
        x, dy, dres, gamma, beta = _ln_inputs(70, 136, dtype)
        ref, yard = _ln_ref(x, gamma, beta, F64, dy, dres), _ln_ref(x, gamma, beta, F32, dy, dres)
        bad = _ln_ref(x, gamma, beta, F32, dy, dres, uncentred=True)
        nores = _ln_ref(x, gamma, beta, F32, dy, None)
        _check("emulation layer_norm", dtype, yard[0].to(dtype), ref[0], yard[0])
        _check("emulation layer_norm_bwd dx", dtype, yard[3].to(dtype), ref[3], yard[3])
        assert _fails("mutant", dtype, bad[0].to(dtype), ref[0], yard[0])
        assert _fails("mutant", dtype, nores[3].to(dtype), ref[3], yard[3])
        _measured.pop(("mutant", "bf16" if dtype == BF16 else "f32"), None)


# --------------------------------------------------------------------------------------------------
# window attention

HEAD_DIM = 32


def _partition(t, ws):
    B, Hp, Wp, C = t.shape
    return t.reshape(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)


def _reverse(wins, ws, B, Hp, Wp):
    C = wins.shape[-1]
    return wins.reshape(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)


def _to_windows(t, fill, ws, shift):
    """torch.roll by -shift, then pad at the bottom / right with `fill` [C], then window partition"""
    B, H, W, C = t.shape
    if shift:
        t = torch.roll(t, shifts=(-shift, -shift), dims=(1, 2))
    Hp, Wp = -(-H // ws) * ws, -(-W // ws) * ws
    full = fill.reshape(1, 1, 1, C).expand(B, Hp, Wp, C).clone()
    full[:, :H, :W] = t
    return _partition(full, ws), Hp, Wp


def _from_windows(wins, ws, shift, B, H, W, Hp, Wp):
    """-> ([B,H,W,C] at the real tokens' own places, [C] summed over the padding positions)"""
    full = _reverse(wins, ws, B, Hp, Wp)
    real = full[:, :H, :W]
    pad = full.sum((0, 1, 2)) - real.sum((0, 1, 2))
    if shift:
        real = torch.roll(real, shifts=(shift, shift), dims=(1, 2))
    return real, pad


def _attention_logits(q, k, table, heads, ws, shift, Hp, Wp, scale, swap_index=False, mask_off=0):
    from oracle.swin_upernet import relative_position_index, shifted_window_mask
    N = ws * ws
    idx = relative_position_index(ws)
    if swap_index:
        idx = idx.t()
    s = (q * scale) @ k.transpose(-2, -1) + table[idx.reshape(-1)].reshape(N, N, heads).permute(2, 0, 1).unsqueeze(0)
    if shift:
        if mask_off:  # mutant: the first region boundary at Hp - ws - 1
            img = torch.zeros(1, Hp, Wp, 1)
            for i, hs in enumerate((slice(0, -ws - mask_off), slice(-ws - mask_off, -shift), slice(-shift, None))):
                for j, wsl in enumerate((slice(0, -ws), slice(-ws, -shift), slice(-shift, None))):
                    img[:, hs, wsl, :] = 3 * i + j
            mw = _partition(img, ws).reshape(-1, N)
            mask = (mw.unsqueeze(1) != mw.unsqueeze(2)).to(s.dtype) * -100.0
        else:
            mask = shifted_window_mask(Hp, Wp, ws, shift).to(s.dtype)
        nW = mask.shape[0]
        s = (s.reshape(-1, nW, heads, N, N) + mask.reshape(1, nW, 1, N, N)).reshape(-1, heads, N, N)
    return s


def _attention_ref(qkv, bias, table, heads, ws, shift, dt, dout=None, terms=False, **mutant):
    """timm's SwinTransformerBlock._attn between the two projections on a given qkv tensor [B,H,W,3C]; padding tokens
    project to the qkv bias.  -> out [, dqkv, dtable, dbias_pad]; terms: also the float64 A maps of (R3) / (R4):
    (A_out [, A_dqkv, A_dbias])"""
    B, H, W, C3 = qkv.shape
    C, N, scale = C3 // 3, ws * ws, HEAD_DIM ** -0.5
    grad = dout is not None
    qkv, bias, table = (t.to(dt).clone().requires_grad_(grad) for t in (qkv, bias, table))
    xw, Hp, Wp = _to_windows(qkv, bias, ws, shift)
    q, k, v = xw.reshape(-1, N, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4).unbind(0)       # [nW B, heads, N, 32]
    p = _attention_logits(q, k, table, heads, ws, shift, Hp, Wp, scale, **mutant).softmax(-1)

    def back(t):  # [nW B, heads, N, 32] -> tokens
        return _from_windows(t.transpose(1, 2).reshape(-1, N, heads * HEAD_DIM), ws, shift, B, H, W, Hp, Wp)

    out = back(p @ v)[0]
    res = [out.detach()]
    if grad:
        (out * dout.to(dt)).sum().backward()
        res += [qkv.grad, table.grad, bias.grad]
    if terms:
        with torch.no_grad():
            extra = [U * back(p @ v.abs())[0]]
            if grad:
                dow = _to_windows(dout.to(dt), torch.zeros(C, dtype=dt), ws, shift)[0]
                do = dow.reshape(-1, N, heads, HEAD_DIM).transpose(1, 2)
                dp = do @ v.transpose(-2, -1)
                ds = p * (dp - (p * dp).sum(-1, keepdim=True))
                a = [scale * ds.abs() @ k.abs(), scale * ds.abs().transpose(-2, -1) @ q.abs(), p.transpose(-2, -1) @ do.abs()]
                a = torch.stack(a, dim=1)                                                   # [nW B, 3, heads, N, 32]
                real, pad = _from_windows(a.permute(0, 3, 1, 2, 4).reshape(-1, N, C3), ws, shift, B, H, W, Hp, Wp)
                extra += [U * real, U * pad]
        res.append(extra)
    return res


def _attention_emulate(qkv, bias, table, heads, ws, shift, dout, drop_last_key_tile=False, **mutant):
    """window_attention_bf16_kernel / window_attention_bwd_kernel in f32 torch, rounding at (R3) / (R4) and at the
    stores -> out bf16, dqkv bf16, dtable f32, dbias_pad f32"""
    B, H, W, C3 = qkv.shape
    C, N, scale = C3 // 3, ws * ws, HEAD_DIM ** -0.5
    xw, Hp, Wp = _to_windows(qkv, bias, ws, shift)
    q, k, v = xw.reshape(-1, N, 3, heads, HEAD_DIM).permute(2, 0, 3, 1, 4).unbind(0)
    s = _attention_logits(q, k, table, heads, ws, shift, Hp, Wp, scale, **mutant)
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    er = _bf(e)                                                                             # (R3)
    if drop_last_key_tile:  # mutant: P V stops before the ragged last 16-key tile
        er[..., (N - 1) // 16 * 16:] = 0
    o = (er @ v) / e.sum(-1, keepdim=True)

    def back(t):
        return _from_windows(t.transpose(1, 2).reshape(-1, N, heads * HEAD_DIM), ws, shift, B, H, W, Hp, Wp)

    p = e / e.sum(-1, keepdim=True)
    do = _to_windows(dout, torch.zeros(C), ws, shift)[0].reshape(-1, N, heads, HEAD_DIM).transpose(1, 2)
    dp = do @ v.transpose(-2, -1)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    pr, dsr = _bf(p), _bf(ds)                                                               # (R4)
    g = torch.stack([scale * (dsr @ k), scale * (dsr.transpose(-2, -1) @ q), pr.transpose(-2, -1) @ do], dim=1)
    dqkv, dbias = _from_windows(g.permute(0, 3, 1, 2, 4).reshape(-1, N, C3), ws, shift, B, H, W, Hp, Wp)
    from oracle.swin_upernet import relative_position_index
    dtable = torch.zeros_like(table).index_add_(0, relative_position_index(ws).reshape(-1),
                                                ds.sum(0).permute(1, 2, 0).reshape(N * N, heads))
    return back(o)[0].to(BF16), dqkv.to(BF16), dtable, dbias


def _attention_maps(ws):
    """(H, W, shifts): an exact multiple of the window; H % ws = 1 and W % ws = ws - 1"""
    shifts = sorted({0, 1, ws - 1, ws // 2})
    return [(2 * ws, ws, shifts), (ws + 1, 2 * ws - 1, shifts)]


def _attention_inputs(B, H, W, heads, ws, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    C = heads * HEAD_DIM
    qkv = _quant(torch.randn(B, H, W, 3 * C, generator=g), dtype)
    dout = _quant(torch.randn(B, H, W, C, generator=g), dtype)
    bias = torch.randn(3 * C, generator=g)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g) * 0.5
    return qkv, dout, bias, table, (bias if dtype == F32 else _bf(bias))  # the padding tokens' q / k / v as stored


def _attention_case(B, H, W, heads, ws, shift, dtype, run, name):
    qkv, dout, bias, table, bias_used = _attention_inputs(B, H, W, heads, ws, dtype, H * 31 + W + ws + shift + heads)
    ref = _attention_ref(qkv, bias_used, table, heads, ws, shift, F64, dout, terms=True)
    yard = _attention_ref(qkv, bias_used, table, heads, ws, shift, F32, dout)
    out, dqkv, dtable, dbias = run(qkv, dout, bias, bias_used, table, heads, ws, shift)
    what = f"B={B} {H}x{W} heads={heads} ws={ws} shift={shift}"
    e_out, e_dqkv, e_dbias = ref[4]
    _check(name, dtype, out, ref[0], yard[0], what=what, extra=e_out)
    _check(name + "_bwd dqkv", dtype, dqkv, ref[1], yard[1], what=what, extra=e_dqkv)
    _check(name + "_bwd dtable", dtype, dtable, ref[2], yard[2], f32_out=True, what=what)
    _check(name + "_bwd dbias_pad", dtype, dbias, ref[3], yard[3], f32_out=True, what=what, extra=e_dbias)
    if H % ws == 0 and W % ws == 0:
        assert bool((ref[3] == 0).all()) and bool((dbias == 0).all()), what  # no padding token: exactly 0


def _attention_gpu(cuda, dtype):
    from flairhip import ops

    def run(qkv, dout, bias, bias_used, table, heads, ws, shift):
        qd, dd, bd, td = _dev(qkv, dtype, cuda), _dev(dout, dtype, cuda), bias.to(cuda), table.to(cuda)
        out = ops.window_attention(qd, bd, td, heads, ws, shift, HEAD_DIM ** -0.5)
        dqkv, dtable, dbias = ops.window_attention_bwd(qd, dd, bd, td, heads, ws, shift, HEAD_DIM ** -0.5)
        return out, dqkv, dtable, dbias
    return run


def _attention_emulated(**mutant):
    def run(qkv, dout, bias, bias_used, table, heads, ws, shift):
        return _attention_emulate(qkv, bias_used, table, heads, ws, shift, dout, **mutant)
    return run


def _attention_sweep(ws, dtype, run, name):
    for H, W, shifts in _attention_maps(ws):
        for shift in shifts:
            for heads, B in ((1, 1), (3, 2), (1, 2), (3, 1)):
                _attention_case(B, H, W, heads, ws, shift, dtype, run, name)


@gpu
@DTYPES
@pytest.mark.parametrize("ws", [2, 3, 5, 8, 9, 11, 12])
def test_window_attention(cuda, ws, dtype):
    _attention_sweep(ws, dtype, _attention_gpu(cuda, dtype), "window_attention")


@gpu
@DTYPES
def test_window_attention_map_smaller_than_the_window(cuda, dtype):
    for heads, B in ((1, 2), (3, 1)):
        _attention_case(B, 5, 9, heads, 7, 0, dtype, _attention_gpu(cuda, dtype), "window_attention")


@pytest.mark.parametrize("ws", [2, 3, 5, 8, 9, 11, 12])
def test_emulation_window_attention(ws):
    """CPU: f32 attention that rounds P and dS where the bf16 kernels do stays inside the bf16 bounds"""
    _attention_sweep(ws, BF16, _attention_emulated(), "emulation window_attention")
    if ws == 8:
        _attention_case(2, 5, 9, 3, 7, 0, BF16, _attention_emulated(), "emulation window_attention")


def test_mutant_window_attention():
    """CPU: a relative-position index with i and j swapped, a mask-region boundary at Hp - ws - 1 and a P V product without
    the ragged last key tile at N = 81 are refused"""
    for kw, (B, H, W, heads, ws, shift) in (({"swap_index": True}, (1, 6, 3, 1, 3, 0)),
                                            ({"mask_off": 1}, (1, 10, 5, 1, 5, 2)),
                                            ({"drop_last_key_tile": True}, (1, 18, 9, 1, 9, 0))):
        _attention_case(B, H, W, heads, ws, shift, BF16, _attention_emulated(), "emulation window_attention")
        with pytest.raises(AssertionError, match="of the bound"):
            _attention_case(B, H, W, heads, ws, shift, BF16, _attention_emulated(**kw), "mutant")
    for key in [k for k in _measured if k[0].startswith("mutant")]:
        del _measured[key]


# --------------------------------------------------------------------------------------------------
# small kernels

@gpu
@DTYPES
def test_gelu(cuda, dtype):
    from flairhip import ops
    g = torch.Generator().manual_seed(17)
    edge = torch.tensor([0.0, -0.0, 8.0, -8.0, 0.5, -0.5, 3.0, -3.0])
    for x in (edge, _quant(torch.cat([edge, torch.randn(8 * 1031, generator=g) * 2]), dtype)):  # n = 8; > one block
        _check("gelu", dtype, ops.gelu(_dev(x, dtype, cuda)), _gelu(x.double()), _gelu(x))


@gpu
@DTYPES
@pytest.mark.parametrize("ps", [2, 4])
def test_space_to_depth(cuda, ps, dtype):
    from flairhip import ops
    B, H, W, C = 2, 8, 12, 8
    x = _quant(torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(18)), dtype)
    ref = x.reshape(B, H // ps, ps, W // ps, ps, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H // ps, W // ps, ps * ps * C)
    got = ops.space_to_depth(_dev(x, dtype, cuda), ps)
    assert got.dtype == dtype and torch.equal(got.float().cpu(), ref)
    _measured[("space_to_depth (exact)", "bf16" if dtype == BF16 else "f32")] = (0.0, 0.0)


@gpu
@DTYPES
@pytest.mark.parametrize("rows,C,rps", [(70, 8, 37), (300, 264, 64), (5, 16, 1)])
def test_scale_rows(cuda, rows, C, rps, dtype):
    from flairhip import ops
    g = torch.Generator().manual_seed(19)
    x = _quant(torch.randn(rows, C, generator=g), dtype)
    sc = torch.rand(-(-rows // rps), generator=g) * 2
    sc[0] = 0.0
    full = sc.repeat_interleave(rps)[:rows, None]
    got = ops.scale_rows(_dev(x, dtype, cuda), sc.to(cuda), rps)
    _check("scale_rows", dtype, got, x.double() * full.double(), x * full)


@gpu
@DTYPES
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("rows", [1, 256 * 512 + 3])
def test_column_sums(cuda, rows, C, dtype):
    from flairhip import ops
    x = _quant(torch.randn(rows, C, generator=torch.Generator().manual_seed(20)) + 0.25, dtype)
    _check("column_sums", dtype, ops.column_sums(_dev(x, dtype, cuda)), x.double().sum(0), x.sum(0), f32_out=True)


def _pool_ref(x, S, dt, dy=None, floor_end=False):
    """nn.AdaptiveAvgPool2d(S) on NHWC -> y [, dx]"""
    xx = x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_(dy is not None)
    if floor_end:  # mutant: region end floor((i + 1) H / S) instead of the ceiling
        B, C, H, W = xx.shape
        y = torch.stack([torch.stack([xx[:, :, i * H // S:max((i + 1) * H // S, i * H // S + 1),
                                         j * W // S:max((j + 1) * W // S, j * W // S + 1)].mean((2, 3))
                                      for j in range(S)], -1) for i in range(S)], -2)
    else:
        y = F.adaptive_avg_pool2d(xx, S)
    res = [y.detach().permute(0, 2, 3, 1)]
    if dy is not None:
        (y * dy.to(dt).permute(0, 3, 1, 2)).sum().backward()
        res.append(xx.grad.permute(0, 2, 3, 1))
    return res


def _pool_inputs(hw, S, C, dtype):
    g = torch.Generator().manual_seed(21 + S)
    return (_quant(torch.randn(2, hw[0], hw[1], C, generator=g), dtype), _quant(torch.randn(2, S, S, C, generator=g), dtype))


@gpu
@DTYPES
@pytest.mark.parametrize("C", [8, 264])
@pytest.mark.parametrize("S", [1, 2, 3, 6])
@pytest.mark.parametrize("hw", [(7, 5), (16, 16), (5, 7)], ids=str)  # S = 6 > W, and S = 6 > H: regions of one pixel repeat
def test_adaptive_avg_pool(cuda, hw, S, C, dtype):
    from flairhip import ops
    x, dy = _pool_inputs(hw, S, C, dtype)
    ref, yard = _pool_ref(x, S, F64, dy), _pool_ref(x, S, F32, dy)
    _check("adaptive_avg_pool", dtype, ops.adaptive_avg_pool(_dev(x, dtype, cuda), S), ref[0], yard[0])
    _check("adaptive_avg_pool_bwd", dtype, ops.adaptive_avg_pool_bwd(_dev(dy, dtype, cuda), hw), ref[1], yard[1])


def test_mutant_adaptive_avg_pool():
    """CPU: a pool whose regions end at floor((i + 1) H / S) is refused wherever S does not divide the map"""
    for dtype in (F32, BF16):
        x, _ = _pool_inputs((7, 5), 3, 8, dtype)
        ref, yard = _pool_ref(x, 3, F64), _pool_ref(x, 3, F32)
        _check("emulation adaptive_avg_pool", dtype, yard[0].to(dtype), ref[0], yard[0])
        assert _fails("mutant", dtype, _pool_ref(x, 3, F32, floor_end=True)[0].to(dtype), ref[0], yard[0])
        _measured.pop(("mutant", "bf16" if dtype == BF16 else "f32"), None)


@gpu
@DTYPES
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("hw_in,hw_out", [((1, 1), (5, 3)), ((5, 7), (5, 7)), ((9, 12), (3, 4)), ((3, 4), (7, 10))], ids=str)
def test_bilinear_slice(cuda, hw_in, hw_out, align, dtype):
    from flairhip import ops
    B, C, pitch, off = 2, 16, 40, 8
    g = torch.Generator().manual_seed(22)
    x = _quant(torch.randn(B, *hw_in, C, generator=g), dtype)
    add = _quant(torch.randn(B, *hw_out, C, generator=g), dtype)
    dwide = _quant(torch.randn(B, *hw_out, pitch, generator=g), dtype)

    def run(dt):
        xx = x.to(dt).permute(0, 3, 1, 2).clone().requires_grad_()
        y = F.interpolate(xx, size=hw_out, mode="bilinear", align_corners=align)
        (y * dwide[..., off:off + C].to(dt).permute(0, 3, 1, 2)).sum().backward()
        return y.detach().permute(0, 2, 3, 1), xx.grad.permute(0, 2, 3, 1)

    ref, yard = run(F64), run(F32)
    xd = _dev(x, dtype, cuda)
    _check("bilinear_slice", dtype, ops.bilinear_slice(xd, hw_out, align_corners=align), ref[0], yard[0], what="dense")
    wide = torch.full((B, *hw_out, pitch), 7.0, dtype=dtype, device=cuda)
    got = ops.bilinear_slice(xd, hw_out, out=wide, offset=off, addend=_dev(add, dtype, cuda), align_corners=align)
    assert got.data_ptr() == wide.data_ptr()
    _check("bilinear_slice", dtype, wide[..., off:off + C], ref[0] + add.double(), yard[0] + add, what="slice + addend")
    assert bool((wide[..., :off] == 7.0).all()) and bool((wide[..., off + C:] == 7.0).all())  # the rest of the pitch is untouched
    dx = ops.bilinear_slice_bwd(_dev(dwide, dtype, cuda), hw_in, C, offset=off, align_corners=align)
    _check("bilinear_slice_bwd", dtype, dx, ref[1], yard[1])


@gpu
@DTYPES
@pytest.mark.parametrize("hw", [(1, 1), (1, 3), (5, 12)], ids=str)
def test_updown2x_slice(cuda, hw, dtype):
    from flairhip import ops
    B, C, pitch, off = 2, 8, 24, 16
    (H, W), g = hw, torch.Generator().manual_seed(23)
    wide = _quant(torch.randn(B, H, W, pitch, generator=g), dtype)

    def run(dt):
        xx = wide[..., off:off + C].to(dt).permute(0, 3, 1, 2)
        up = F.interpolate(xx, size=(2 * H, 2 * W), mode="bilinear", align_corners=False)
        return F.interpolate(up, size=(H, W), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)

    ref, yard = run(F64), run(F32)
    wd = _dev(wide, dtype, cuda)
    _check("updown2x_slice", dtype, ops.updown2x_slice(wd, C, x_offset=off), ref, yard, what="dense output")
    dst = torch.full((B, H, W, pitch), 7.0, dtype=dtype, device=cuda)
    ops.updown2x_slice(wd, C, x_offset=off, out=dst, offset=8)
    _check("updown2x_slice", dtype, dst[..., 8:8 + C], ref, yard, what="slice to slice")
    assert bool((dst[..., :8] == 7.0).all()) and bool((dst[..., 8 + C:] == 7.0).all())


# --------------------------------------------------------------------------------------------------
# the wrappers refuse operands that would make a kernel read out of bounds

def _refused(match, fn, *args, **kw):
    with pytest.raises(ValueError, match=match):
        fn(*args, **kw)


def _bad_vecs(v):
    """wrong dtype, short, strided, on the CPU"""
    return (v.bfloat16(), v[:-1], torch.ones(2 * v.numel(), device=v.device)[::2], v.cpu())


@gpu
def test_layer_norm_refuses_bad_operands(cuda):
    from flairhip import ops
    from flairhip.lib import FlairHipError
    rows, C = 6, 16
    x, gamma, beta = torch.randn(rows, C, device=cuda), torch.ones(C, device=cuda), torch.zeros(C, device=cuda)
    stats = torch.empty(rows, 2, device=cuda)
    ops.layer_norm(x, gamma, beta, stats=stats)
    ops.layer_norm_bwd(x, x, gamma, stats, dres=x)
    for bad in _bad_vecs(gamma):
        _refused("layer_norm: gamma must be contiguous f32 of 16", ops.layer_norm, x, bad, beta)
        _refused("layer_norm: beta must be contiguous f32 of 16", ops.layer_norm, x, gamma, bad)
        _refused("layer_norm_bwd: gamma must be contiguous f32 of 16", ops.layer_norm_bwd, x, x, bad, stats)
    for bad in (stats.double(), stats[:-1], stats.t().contiguous().t(), stats.reshape(-1), stats.cpu()):
        _refused(r"layer_norm: stats must be contiguous f32 \[6, 2\]", ops.layer_norm, x, gamma, beta, stats=bad)
        _refused(r"layer_norm_bwd: stats must be contiguous f32 \[6, 2\]", ops.layer_norm_bwd, x, x, gamma, bad)
    for bad in (x.bfloat16(), x[:-1], x.t().contiguous().t(), x.cpu()):
        _refused("layer_norm_bwd: dy must be contiguous", ops.layer_norm_bwd, x, bad, gamma, stats)
        _refused("layer_norm_bwd: dres must be contiguous", ops.layer_norm_bwd, x, x, gamma, stats, dres=bad)
    xs = torch.randn(rows, 2 * C, device=cuda)[:, ::2]
    _refused("layer_norm: input must be contiguous", ops.layer_norm, xs, gamma, beta)
    _refused("layer_norm_bwd: input must be contiguous", ops.layer_norm_bwd, xs, x, gamma, stats)
    x12 = torch.randn(rows, 12, device=cuda)
    with pytest.raises(FlairHipError, match="layer_norm"):  # C % 8: the host-side requirement
        ops.layer_norm(x12, torch.ones(12, device=cuda), torch.zeros(12, device=cuda))


@gpu
def test_patch_merge_norm_refuses_bad_operands(cuda):
    from flairhip import ops
    B, H, W, C = 2, 4, 6, 8
    x, dy = torch.randn(B, H, W, C, device=cuda), torch.randn(B, H // 2, W // 2, 4 * C, device=cuda)
    gamma, beta = torch.ones(4 * C, device=cuda), torch.zeros(4 * C, device=cuda)
    stats = torch.empty(B * 6, 2, device=cuda)
    ops.patch_merge_norm(x, gamma, beta, stats=stats)
    ops.patch_merge_norm_bwd(x, dy, gamma, stats)
    for bad in _bad_vecs(gamma):
        _refused("patch_merge_norm: gamma must be contiguous f32 of 32", ops.patch_merge_norm, x, bad, beta)
        _refused("patch_merge_norm: beta must be contiguous f32 of 32", ops.patch_merge_norm, x, gamma, bad)
        _refused("patch_merge_norm_bwd: gamma must be contiguous f32 of 32", ops.patch_merge_norm_bwd, x, dy, bad, stats)
    for bad in (stats[:-1], stats.double(), stats.cpu()):
        _refused(r"patch_merge_norm: stats must be contiguous f32 \[12, 2\]", ops.patch_merge_norm, x, gamma, beta, stats=bad)
        _refused(r"patch_merge_norm_bwd: stats must be contiguous f32 \[12, 2\]", ops.patch_merge_norm_bwd, x, dy, gamma, bad)
    for bad in (dy.bfloat16(), dy[:1], dy.reshape(B, H // 2, W // 2 * 4, C), dy.cpu()):
        _refused("patch_merge_norm_bwd: dy must be contiguous", ops.patch_merge_norm_bwd, x, bad, gamma, stats)
    for odd in (torch.randn(B, 3, 6, C, device=cuda), torch.randn(B, 4, 5, C, device=cuda)):
        _refused("odd map", ops.patch_merge_norm, odd, gamma, beta)
        _refused("odd map", ops.patch_merge_norm_bwd, odd, dy, gamma, stats)


@gpu
def test_window_attention_refuses_bad_operands(cuda):
    from flairhip import ops
    from flairhip.lib import FlairHipError
    B, H, W, heads, ws = 1, 3, 9, 1, 7
    C = heads * HEAD_DIM
    qkv, dout = torch.randn(B, H, W, 3 * C, device=cuda), torch.randn(B, H, W, C, device=cuda)
    bias, table = torch.randn(3 * C, device=cuda), torch.randn((2 * ws - 1) ** 2, heads, device=cuda)
    scale = HEAD_DIM ** -0.5
    ops.window_attention(qkv, bias, table, heads, ws, 3, scale)
    ops.window_attention_bwd(qkv, dout, bias, table, heads, ws, 3, scale)
    for bad in _bad_vecs(bias):
        _refused("window_attention: qkv_bias must be contiguous f32 of 96", ops.window_attention, qkv, bad, table, heads, ws, 0, scale)
        _refused("window_attention_bwd: qkv_bias must be contiguous f32 of 96", ops.window_attention_bwd, qkv, dout, bad,
                 table, heads, ws, 0, scale)
    wide = torch.randn((2 * ws - 1) ** 2, 2, device=cuda)
    for bad in (table.bfloat16(), table[:-1], wide[:, :1], table.reshape(-1), table.cpu()):
        _refused("window_attention: relative position bias table", ops.window_attention, qkv, bias, bad, heads, ws, 0, scale)
        _refused("window_attention_bwd: relative position bias table", ops.window_attention_bwd, qkv, dout, bias, bad,
                 heads, ws, 0, scale)
    for bad in (dout.bfloat16(), dout[:, :-1], dout.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3), dout.cpu()):
        with pytest.raises(ValueError, match="dout"):
            ops.window_attention_bwd(qkv, bad, bias, table, heads, ws, 0, scale)
    # host side: a cyclic shift larger than the map (win_token wraps by one subtraction), after the guard exists
    with pytest.raises(FlairHipError, match="shift 5 exceeds the 3 x 9 map"):
        ops.window_attention(qkv, bias, table, heads, ws, 5, scale)
    with pytest.raises(FlairHipError, match="shift 5 exceeds the 3 x 9 map"):
        ops.window_attention_bwd(qkv, dout, bias, table, heads, ws, 5, scale)


@gpu
def test_small_wrappers_refuse_bad_operands(cuda):
    from flairhip import ops
    from flairhip.lib import FlairHipError
    rows, C = 10, 16
    x = torch.randn(rows, C, device=cuda)
    sc = torch.ones(4, device=cuda)
    ops.scale_rows(x, sc, 3)
    _refused("scale_rows: row_scale must be contiguous f32", ops.scale_rows, x, sc[:3], 3)        # ceil(10 / 3) = 4
    _refused("scale_rows: row_scale must be contiguous f32", ops.scale_rows, x, sc.double(), 3)
    _refused("scale_rows: row_scale must be contiguous f32", ops.scale_rows, x, sc.cpu(), 3)
    _refused("scale_rows: row_scale must be contiguous f32", ops.scale_rows, x, torch.ones(8, device=cuda)[::2], 3)
    _refused("scale_rows: row_scale must be contiguous f32", ops.scale_rows, x, sc, 0)
    xs = torch.randn(rows, 2 * C, device=cuda)[:, ::2]
    _refused("scale_rows: input must be contiguous", ops.scale_rows, xs, sc, 3)
    _refused("gelu: input must be contiguous", ops.gelu, xs)
    w = torch.randn(8, C, device=cuda)
    ops.linear(x, w, row_scale=sc, rows_per_scale=3)
    _refused("linear: row_scale must be contiguous f32", ops.linear, x, w, row_scale=sc[:3], rows_per_scale=3)
    _refused("linear: row_scale must be contiguous f32", ops.linear, x, w, row_scale=sc.double(), rows_per_scale=3)
    with pytest.raises(FlairHipError, match="multiple of 32"):  # K % 32 for bf16: the host-side requirement
        ops.linear(torch.zeros(8, 48, dtype=BF16, device=cuda), torch.zeros(8, 48, dtype=BF16, device=cuda))
    dy = torch.randn(2, 3, 3, C, device=cuda)
    ops.adaptive_avg_pool_bwd(dy, (7, 5))
    _refused(r"adaptive_avg_pool_bwd: dy must be \[B, S, S, C\]", ops.adaptive_avg_pool_bwd, torch.randn(2, 3, 2, C, device=cuda), (7, 5))
    _refused("contiguous CUDA NHWC", ops.adaptive_avg_pool_bwd, dy.permute(0, 2, 1, 3), (7, 5))
    _refused("contiguous CUDA NHWC", ops.adaptive_avg_pool_bwd, dy.cpu(), (7, 5))
    ops.bilinear_slice_bwd(dy, (2, 2), 8, offset=8)
    _refused("bilinear_slice_bwd: slice", ops.bilinear_slice_bwd, dy, (2, 2), 16, offset=8)
    _refused("contiguous CUDA NHWC", ops.bilinear_slice_bwd, dy.permute(0, 2, 1, 3), (2, 2), 8)
