"""Functional layer over the C ABI: torch tensors in, torch tensors out, no autograd.

PyTorch is used here for device memory and the current HIP stream only.  Activations are
contiguous NHWC tensors ``[B, H, W, C]`` (bf16 or f32) whose channel count is a multiple of 16;
every function launches on ``torch.cuda.current_stream()`` and returns immediately.
"""
from __future__ import annotations

import logging
import os

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import lib as _l

logger = logging.getLogger(__name__)

CH_ALIGN = 16


def pad_channels(c: int, align: int = CH_ALIGN) -> int:
    return (c + align - 1) // align * align


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _l.BF16
    if t.dtype == torch.float32:
        return _l.F32
    raise TypeError(f"flairhip: unsupported dtype {t.dtype}")


def _dtype_id(dtype: torch.dtype) -> int:
    return _l.BF16 if dtype == torch.bfloat16 else _l.F32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk_nhwc(t: torch.Tensor, name: str) -> None:
    if not (t.is_cuda and t.dim() == 4 and t.is_contiguous()):
        raise ValueError(f"flairhip: {name} must be a contiguous CUDA NHWC tensor, got {tuple(t.shape)} "
                         f"strides {t.stride()} on {t.device}")


_workspaces = {}
_retired_workspaces = []


def workspace(nbytes: int, device: torch.device, slot: str = "default") -> torch.Tensor:
    """Grow-only scratch buffer per (device, slot); the library itself never allocates.  A buffer that is outgrown
    stays alive (``_retired_workspaces``): captured hipGraphs (GraphedTrainStep, GraphedCall) have its raw pointer
    baked into their kernel arguments, and the caching allocator would otherwise hand the freed block to another
    tensor that later replays then scribble split-K partials and statistics over."""
    key = (device.index, slot)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired_workspaces.append(buf)
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


# --------------------------------------------------------------------------------------------------
# convolution

@dataclass
class PackedWeight:
    data: torch.Tensor  # packed operand (opaque bytes viewed as the compute dtype)
    rows: int           # padded row count (output channels of the GEMM)
    rows_real: int
    ci_pitch: int       # channel pitch of the activation it multiplies
    bco: int
    kh: int
    kw: int
    stride: int         # stride of the conv the operand is used for (1 for every dgrad operand)
    ch_real: int = 0    # real (unpadded) reduction channels


def pack_conv_weight(w_oihw: torch.Tensor, dtype: torch.dtype, stride: int, ci_pitch: int,
                     transpose: bool = False, scale: Optional[torch.Tensor] = None,
                     allow_ring: bool = True, allow_thin: bool = True, allow_stem: bool = True) -> PackedWeight:
    """OIHW f32 master weight -> MFMA operand for ffa_conv_run (forward, or dgrad when transpose=True).
    allow_ring / allow_thin / allow_stem admit the layouts ffa_conv_plan may pick besides conv_igemm's; which forms of
    call each layout serves is the table at ffa_conv_call_t (include/flairhip.h).  The caller vouches for the padding:
    the ring and thin kernels are pad-1 kernels, the stem kernel a pad-3 one."""
    lib = _l.load()
    if w_oihw.dtype != torch.float32 or not w_oihw.is_contiguous():
        raise ValueError("pack_conv_weight: master weight must be contiguous f32 OIHW")
    O, I, kh, kw = w_oihw.shape
    rows_real = I if transpose else O
    use_stride = 1 if transpose else stride
    did = _dtype_id(dtype)
    # the dgrad operand of a stride-2 layer is read through the zero insertion (dil = 2): conv_igemm only
    ring_ok = allow_ring and not (transpose and stride != 1)
    thin_ok = allow_thin and not (transpose and stride != 1)
    # the stem kernel stages the first 8 channels of a pixel only: forward operand of a <= 8-channel input
    stem_ok = allow_stem and not transpose and I <= 8  # (the caller vouches for pad = 3)
    bco = lib.ffa_conv_plan(did, kh, kw, use_stride, rows_real, ci_pitch,
                            (1 if ring_ok else 0) | (2 if thin_ok else 0) | (4 if stem_ok else 0))
    if bco <= 0:
        raise _l.FlairHipError(f"no conv kernel for {kh}x{kw} stride {use_stride}")
    blk = bco & 0xFFF
    rows = (rows_real + blk - 1) // blk * blk
    rg = lib.ffa_conv_row_group(kh)
    nbytes = lib.ffa_pack_conv_weight_bytes(did, rows, ci_pitch, kh, kw, bco)
    dst = torch.empty(nbytes // (2 if dtype == torch.bfloat16 else 4), dtype=dtype, device=w_oihw.device)
    _l.check(lib.ffa_pack_conv_weight(did, w_oihw.data_ptr(), _ptr(scale), dst.data_ptr(), O, I, kh, kw,
                                      1 if transpose else 0, rows, ci_pitch, bco, rg, _stream()), "pack_conv_weight")
    return PackedWeight(dst, rows, rows_real, ci_pitch, bco, kh, kw, use_stride, O if transpose else I)


class PackBatch:
    """Descriptor tables for ffa_pack_conv_weights_batched: re-packs many conv operands in one launch per layout.

    entries: (master weight OIHW f32, PackedWeight it feeds, transpose flag[, (first column, columns)]).  A column block
    belongs to a 1x1 fusion weight, and ffa_conv_plan gives a 1x1 operand no other layout than conv_igemm's (the only
    one ffa_pack_desc_fill takes a block for).  The tables hold raw device pointers, so they must be rebuilt when a
    parameter or a packed buffer is re-allocated."""

    def __init__(self, entries, dtype: torch.dtype):
        lib = _l.load()
        self.dtype_id = _dtype_id(dtype)
        self.keep = []
        nb = lib.ffa_pack_desc_bytes()
        desc = C.create_string_buffer(nb)
        hosts = {}  # layout bits of bco -> the descriptors of that layout, back to back
        for e in entries:
            w, pw, transpose = e[:3]
            O, I, kh, kw = w.shape
            off, c = e[3] if len(e) > 3 else (0, I)  # column block W[:, off : off + c] of a fusion 1x1 weight
            _l.check(lib.ffa_pack_desc_fill(C.addressof(desc), w.data_ptr(), None, pw.data.data_ptr(), O, I, off, c, kh, kw,
                                            1 if transpose else 0, pw.rows, pw.ci_pitch, pw.bco,
                                            lib.ffa_conv_row_group(kh), self.dtype_id), "pack_desc_fill")
            hosts.setdefault(pw.bco & (_l.BCO_RING | _l.BCO_THIN | _l.BCO_STEM), bytearray()).extend(desc.raw)
            self.keep.append((w, pw))
        dev = entries[0][0].device
        self.tables = [(layout, torch.frombuffer(host, dtype=torch.uint8).to(dev), len(host) // nb)
                       for layout, host in hosts.items()]

    def run(self) -> None:
        lib = _l.load()
        for layout, table, n in self.tables:
            _l.check(lib.ffa_pack_conv_weights_batched(self.dtype_id, layout, table.data_ptr(), n, _stream()),
                     "pack_conv_weights_batched")


def conv_out_size(h: int, k: int, stride: int, pad: int) -> int:
    return (h + 2 * pad - k) // stride + 1


def _conv_call(form: int, dtype_id: int, w: PackedWeight, geom, pad: int, dil: int = 1, relu: bool = False, c1: int = 0,
               x=None, x2=None, bias=None, residual=None, out=None, out2=None, stats=None, pro=(None, None),
               bn=(None, None, None)) -> "_l.ConvCall":
    """The descriptor of one convolution call (ffa_conv_call_t) in one constructor call.  geom = (B, Hi, Wi, Ho, Wo, Co);
    in the CONV_UPCAT form Hi, Wi and the operand's pitch describe the virtual input, in the CONV_POOLED form Ho, Wo, Co
    the virtual output; c1 is the channel split of those two forms."""
    B, Hi, Wi, Ho, Wo, Co = geom
    return _l.ConvCall(dtype_id, form, _ptr(x), _ptr(x2), w.data.data_ptr(), _ptr(bias), _ptr(residual), _ptr(out),
                       _ptr(out2), _ptr(stats), _ptr(pro[0]), _ptr(pro[1]), _ptr(bn[0]), _ptr(bn[1]), _ptr(bn[2]),
                       w.rows, w.bco, B, Hi, Wi, w.ci_pitch, Ho, Wo, Co, w.kh, w.kw, w.stride, pad, dil,
                       1 if relu else 0, c1)


def _conv_run(call: "_l.ConvCall", what: str, stats: Optional[torch.Tensor] = None, may_refuse: bool = False) -> bool:
    """Launch; False when may_refuse and the library has no kernel for this form of call on this operand.  ``stats``
    is held to the tiles of the very call that writes it (a refused call is reported by the launch)."""
    if stats is not None:
        route = _conv_route(call)
        if stats.dtype != torch.float32 or (route is not None and stats.numel() < route.ntiles * 2 * call.Co):
            raise ValueError(f"{what}: statistics buffer too small or not f32")
    rc = _l.load().ffa_conv_run(C.byref(call), _stream())
    if may_refuse and rc == _l.ERR_UNSUPPORTED:
        return False
    _l.check(rc, what)
    return True


def _conv_route(call: "_l.ConvCall", what: Optional[str] = None) -> Optional["_l.ConvRoute"]:
    """What the library would run for this call (kernel family, tile, statistics rows, grid).  A refused call gives
    None, or raises when ``what`` names the caller.  Needs no device: the router reads no tensor."""
    route = _l.ConvRoute()
    rc = _l.load().ffa_conv_route(C.byref(call), C.byref(route))
    if rc != 0 and what is not None:
        _l.check(rc, what)
    return route if rc == 0 else None


def _operand_call(dtype_id: int, w: PackedWeight, B: int, Ho: int, Wo: int, dil: int = 1, form: int = _l.CONV_PLAIN,
                  c1: int = 0, pro: bool = False, stats: bool = False, in_hw=None) -> "_l.ConvCall":
    """The call of this form that operand ``w`` was packed for, at this output size, without tensors: what the queries
    route.  in_hw: the stored input size where the output size does not fix it (stride 2)."""
    Hi, Wi = in_hw or (Ho * w.stride // dil, Wo * w.stride // dil)
    call = _conv_call(form, dtype_id, w, (B, Hi, Wi, Ho, Wo, w.rows), (w.kh - 1) // 2, dil, c1=c1)
    call.pro_scale = call.pro_shift = 1 if pro else None  # the router reads only whether an optional pointer is null
    call.stats = 1 if stats else None
    return call


def conv_is_persistent(x_dtype, B: int, Ho: int, Wo: int, w: "PackedWeight", dil: int = 1) -> bool:
    """True when conv2d runs this operand on conv3x3_persist_kernel (its own symbol in rocprofv3) rather than
    conv_igemm_kernel; used by bench.py to group launches the way a profile does."""
    route = _conv_route(_operand_call(_dtype_id(x_dtype), w, B, Ho, Wo, dil))
    return route is not None and route.kernel == _l.CONV_KERNEL_PERSIST


def conv2d(x: torch.Tensor, w: PackedWeight, pad: int, out_channels: int, bias: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, relu: bool = False, dil: int = 1,
           out_hw: Optional[Tuple[int, int]] = None, out: Optional[torch.Tensor] = None,
           stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[B,Ho,Wo,out_channels] = relu?(conv(x, w) + bias + residual).  out_channels is the stored pitch.
    ``stats`` (f32, >= conv_stat_rows * 2 * out_channels elements) receives per-tile channel sums / sums of squares
    of the stored output for a following training-mode BatchNorm (see bn_finalize)."""
    _chk_nhwc(x, "conv input")
    B, Hi, Wi, Ci = x.shape
    if Ci != w.ci_pitch:
        raise ValueError(f"conv2d: input pitch {Ci} != packed pitch {w.ci_pitch}")
    if out_hw is None:
        hv, wv = (Hi * 2, Wi * 2) if dil == 2 else (Hi, Wi)
        out_hw = (conv_out_size(hv, w.kh, w.stride, pad), conv_out_size(wv, w.kw, w.stride, pad))
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, out_channels), dtype=x.dtype, device=x.device)
    if residual is not None and residual.shape != out.shape:
        raise ValueError("conv2d: residual shape mismatch")
    if bias is not None and bias.numel() < out_channels:
        raise ValueError("conv2d: bias shorter than the output pitch")
    call = _conv_call(_l.CONV_PLAIN, _dt(x), w, (B, Hi, Wi, Ho, Wo, out_channels), pad, dil, relu, x=x, bias=bias,
                      residual=residual, out=out, stats=stats)
    _conv_run(call, "conv2d", stats)
    return out


def conv3x3_ring(x: torch.Tensor, w: PackedWeight, out_channels: int, bias: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, relu: bool = False, stats: Optional[torch.Tensor] = None,
                 pro_scale: Optional[torch.Tensor] = None, pro_shift: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The ring kernel called directly (w must be a ring-layout operand): conv3x3 pad 1 of x, or -- with pro_scale /
    pro_shift -- of relu(x * pro_scale[c] + pro_shift[c]) evaluated while the input is staged (the BatchNorm + ReLU
    of the producing layer folded into this convolution, no normalised tensor in memory)."""
    _chk_nhwc(x, "conv input")
    if not (w.bco & _l.BCO_RING):
        raise ValueError("conv3x3_ring: operand is not in the ring layout")
    B, H, W, Ci = x.shape
    if Ci != w.ci_pitch:
        raise ValueError(f"conv3x3_ring: input pitch {Ci} != packed pitch {w.ci_pitch}")
    if out is None:
        out = torch.empty((B, H, W, out_channels), dtype=x.dtype, device=x.device)
    if (pro_scale is None) != (pro_shift is None):
        raise ValueError("conv3x3_ring: prologue needs scale and shift")
    if pro_scale is not None and (pro_scale.numel() < Ci or pro_shift.numel() < Ci or
                                  pro_scale.dtype != torch.float32 or pro_shift.dtype != torch.float32):
        raise ValueError("conv3x3_ring: prologue vectors must be f32 with one entry per stored input channel")
    call = _conv_call(_l.CONV_PLAIN, _dt(x), w, (B, H, W, H, W, out_channels), 1, relu=relu, x=x, bias=bias,
                      residual=residual, out=out, stats=stats, pro=(pro_scale, pro_shift))
    _conv_run(call, "conv3x3_ring", stats)
    return out


def conv2d_upcat(lo: torch.Tensor, skip: Optional[torch.Tensor], w: PackedWeight, out_channels: int,
                 stats: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, relu: bool = False
                 ) -> Optional[torch.Tensor]:
    """3x3 pad-1 conv over cat(nearest_x2(lo), skip) without materialising it.  Returns None when the library has no
    two-source kernel for this channel split (the caller then concatenates explicitly)."""
    _chk_nhwc(lo, "upcat lo")
    B, Hl, Wl, C1 = lo.shape
    C2 = 0
    if skip is not None:
        _chk_nhwc(skip, "upcat skip")
        if skip.shape[0] != B or skip.shape[1] != 2 * Hl or skip.shape[2] != 2 * Wl or skip.dtype != lo.dtype:
            raise ValueError("conv2d_upcat: skip must be [B, 2*Hl, 2*Wl, C2] of the same dtype")
        C2 = skip.shape[3]
    if w.kh != 3 or w.kw != 3 or w.stride != 1 or w.ci_pitch != C1 + C2:
        raise ValueError("conv2d_upcat: needs a 3x3 stride-1 operand packed for C1 + C2 input channels")
    H, W = 2 * Hl, 2 * Wl
    out = torch.empty((B, H, W, out_channels), dtype=lo.dtype, device=lo.device)
    if bias is not None and bias.numel() < out_channels:
        raise ValueError("conv2d_upcat: bias shorter than the output pitch")
    call = _conv_call(_l.CONV_UPCAT, _dt(lo), w, (B, H, W, H, W, out_channels), 1, relu=relu, c1=C1, x=lo, x2=skip,
                      bias=bias, out=out, stats=stats)
    return out if _conv_run(call, "conv2d_upcat", stats, may_refuse=True) else None


# BatchNorm-backward reductions from the dgrad epilogue (conv2d_bnbwd).  Measured on MI355X, same session: 16.31 vs
# 16.24 ms/step without -- the epilogue's per-lane 16-byte reads of x (one cache line per lane) cost what the saved
# reduction pass gained -- so it stays OFF by default; FFA_FUSED_BN_BWD=1 turns it on (covered by the kernel tests).
FUSED_BN_BWD = os.environ.get("FFA_FUSED_BN_BWD", "0") == "1"


def conv2d_bnbwd(x: torch.Tensor, w: PackedWeight, pad: int, out_channels: int, bnx: torch.Tensor,
                 bn_scale: torch.Tensor, bn_shift: torch.Tensor, residual: Optional[torch.Tensor] = None, dil: int = 1,
                 out_hw: Optional[Tuple[int, int]] = None):
    """A (dgrad) convolution whose output dy is the gradient of relu(bn(bnx)): -> (dy, partials, rows) with the
    BatchNorm-backward reductions sum(g), sum(g*bnx) taken in the conv epilogue (see bn_bwd_partials)."""
    _chk_nhwc(x, "conv input")
    B, Hi, Wi, Ci = x.shape
    if out_hw is None:
        hv, wv = (Hi * 2, Wi * 2) if dil == 2 else (Hi, Wi)
        out_hw = (conv_out_size(hv, w.kh, w.stride, pad), conv_out_size(wv, w.kw, w.stride, pad))
    Ho, Wo = out_hw
    if tuple(bnx.shape) != (B, Ho, Wo, out_channels) or bnx.dtype != x.dtype or not bnx.is_contiguous():
        raise ValueError("conv2d_bnbwd: bnx must have the shape, pitch and dtype of the output")
    out = torch.empty((B, Ho, Wo, out_channels), dtype=x.dtype, device=x.device)
    call = _conv_call(_l.CONV_PLAIN, _dt(x), w, (B, Hi, Wi, Ho, Wo, out_channels), pad, dil, x=x, residual=residual,
                      out=out, bn=(bnx, bn_scale, bn_shift))
    call.stats = 1  # routed before the buffer exists: the router reads only whether the pointer is null
    rows = _conv_route(call, "conv2d_bnbwd").ntiles
    part = workspace(rows * 2 * out_channels * 4, x.device, "bnpart").view(torch.float32)
    call.stats = part.data_ptr()
    _conv_run(call, "conv2d_bnbwd")
    return out, part, rows


def bn_bwd_partials(x: torch.Tensor, dy: torch.Tensor, part: torch.Tensor, rows: int, gamma, beta, mean, rstd):
    """BatchNorm (+ReLU, mask from x) backward from the partial sums of conv2d_bnbwd -> (dx, dgamma, dbeta)"""
    lib = _l.load()
    C_ = x.shape[-1]
    dx = torch.empty_like(x)
    dgb = torch.empty((2, C_), dtype=torch.float32, device=x.device)
    ws = workspace(lib.ffa_bn_workspace_bytes(C_), x.device, "bn")
    _l.check(lib.ffa_bn_bwd_partials(_dt(x), x.data_ptr(), dy.data_ptr(), part.data_ptr(), rows, _ptr(gamma), _ptr(beta),
                                     mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), dgb[0].data_ptr(),
                                     dgb[1].data_ptr(), x.numel() // C_, C_, ws.data_ptr(), ws.numel(), _stream()),
             "bn_bwd_partials")
    return dx, dgb[0], dgb[1]


def conv2d_dgrad_upcat(dy: torch.Tensor, wt: PackedWeight, c1: int, c2: int):
    """Input gradient of conv2d_upcat -> (dlo [B,H/2,W/2,c1], dskip [B,H,W,c2] or None), or None when the channel
    split is not supported (the caller then runs the plain dgrad + upsample2x_concat_bwd)."""
    if not FUSED_UPCAT_BWD:
        return None
    _chk_nhwc(dy, "dgrad_upcat dy")
    B, H, W, Cdy = dy.shape
    if Cdy != wt.ci_pitch or wt.kh != 3 or wt.stride != 1 or H % 2 or W % 2:
        raise ValueError("conv2d_dgrad_upcat: operand / gradient mismatch")
    dlo = torch.empty((B, H // 2, W // 2, c1), dtype=dy.dtype, device=dy.device)
    dskip = torch.empty((B, H, W, c2), dtype=dy.dtype, device=dy.device) if c2 else None
    call = _conv_call(_l.CONV_POOLED, _dt(dy), wt, (B, H, W, H, W, c1 + c2), 1, c1=c1, x=dy, out=dlo, out2=dskip)
    return (dlo, dskip) if _conv_run(call, "conv2d_dgrad_upcat", may_refuse=True) else None


FUSED_BN_STATS = os.environ.get("FFA_FUSED_BN_STATS", "1") != "0"


def conv_stat_rows(B: int, Ho: int, Wo: int, w: Optional[PackedWeight] = None) -> int:
    """rows of per-tile statistics the plain convolution with operand ``w`` writes (w=None: the conv_igemm tiling).
    The functions here that take ``stats`` size and check it from the route of their own call, whatever its form."""
    w = w or _IGEMM_OPERAND
    return _conv_route(_operand_call(_dt(w.data), w, B, Ho, Wo, stats=True), "conv_stat_rows").ntiles


# any conv_igemm operand: the pixel tile of that layout depends on the output size alone
_IGEMM_OPERAND = PackedWeight(torch.empty(0, dtype=torch.bfloat16), 64, 64, 16, 64, 3, 3, 1)


def _bn_finalize(part: torch.Tensor, rows: int, npix: int, channels: int, gamma, beta, running_mean, running_var,
                 momentum: float, eps: float):
    lib = _l.load()
    dev = part.device
    out = torch.empty((4, channels), dtype=torch.float32, device=dev)
    ws = workspace(lib.ffa_bn_workspace_bytes(channels), dev, "bn")
    _l.check(lib.ffa_bn_finalize(part.data_ptr(), rows, npix, channels, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                                 _ptr(running_var), momentum, eps, out[0].data_ptr(), out[1].data_ptr(),
                                 out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), ws.numel(), _stream()),
             "bn_finalize")
    return out[0], out[1], out[2], out[3]


def conv2d_bn_stats(x: torch.Tensor, w: PackedWeight, pad: int, out_channels: int, gamma, beta, running_mean,
                    running_var, momentum: float, eps: float):
    """conv + the batch statistics of its output in one kernel: -> (y0, scale, shift, mean, rstd); the running
    buffers are updated in place.  Equivalent to conv2d followed by bn_stats, minus one pass over y0."""
    if not FUSED_BN_STATS:  # A/B switch (FFA_FUSED_BN_STATS=0): the two-kernel path
        y0 = conv2d(x, w, pad, out_channels)
        return (y0,) + tuple(bn_stats(y0, gamma, beta, running_mean, running_var, momentum, eps))
    B, Hi, Wi, _ = x.shape
    Ho, Wo = conv_out_size(Hi, w.kh, w.stride, pad), conv_out_size(Wi, w.kw, w.stride, pad)
    rows = _conv_route(_operand_call(_dt(x), w, B, Ho, Wo, stats=True, in_hw=(Hi, Wi)), "conv2d_bn_stats").ntiles
    part = workspace(rows * 2 * out_channels * 4, x.device, "bnpart").view(torch.float32)
    y0 = conv2d(x, w, pad, out_channels, stats=part)
    return (y0,) + _bn_finalize(part, rows, B * Ho * Wo, out_channels, gamma, beta, running_mean, running_var,
                                momentum, eps)


# "Normalise on load" (round 3): the BatchNorm + ReLU between two convolutions is evaluated by the CONSUMERS (the next
# conv's forward and weight gradient) while they stage their input, so the normalised tensor is never written.
# Implemented for every consumer kernel family of the U-Net (ring16, thin forward, thin / general weight gradient),
# bit-identical to the materialised form (tests/test_thin_conv_gpu.py, tests/test_ring_conv_gpu.py) -- and measured
# SLOWER in the step (same box, rocprofv3 kernel time per step 13.99 ms without, 14.36 ms with): the 21 saved
# bn_apply passes are worth 0.34 ms, the prologue costs conv3x3_ring16_kernel +10.7 us per launch (52.5 vs 41.8: an LDS
# read-modify-write of every halo piece and an earlier vmcnt drain, in a kernel that has no idle issue slots),
# conv_wgrad_kernel +12 us (68.7 vs 56.6) and the thin kernels +19 ... +51 us.  Off by default;
# FFA_NORM_ON_LOAD=1 turns it on.
NORM_ON_LOAD = os.environ.get("FFA_NORM_ON_LOAD", "0") == "1"


def pro_supported(w: "PackedWeight", dtype: torch.dtype, up: bool = False) -> bool:
    """True when conv2d_pro / conv_wgrad_pro exist for this operand: bf16, ring16 layout (>= 64 channels) or thin layout.
    The library's answer for a prologue call on the operand (ffa_conv_plan gives no ring operand fewer than 64 real
    rows); the weight-gradient kernel behind a ring operand adds whole 64-channel groups of real input channels, which
    the library does not see."""
    if dtype != torch.bfloat16 or not (w.bco & _l.BCO_THIN or (w.ch_real >= 64 and w.ci_pitch % 64 == 0)):
        return False
    form, c1 = (_l.CONV_UPCAT, w.ci_pitch) if up else (_l.CONV_PLAIN, 0)
    return _conv_route(_operand_call(_dtype_id(dtype), w, 1, 32, 32, form=form, c1=c1, pro=True)) is not None


def conv2d_pro(x: torch.Tensor, w: PackedWeight, out_channels: int, pro_scale: torch.Tensor, pro_shift: torch.Tensor,
               bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, relu: bool = False,
               stats: Optional[torch.Tensor] = None, up: bool = False) -> torch.Tensor:
    """3x3 pad-1 conv of relu(x * pro_scale + pro_shift) without the normalised tensor; up: x is the low-resolution map
    of the skip-less nearest-x2 form (thin layout)."""
    _chk_nhwc(x, "conv input")
    B, Hs, Ws, Ci = x.shape
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    if Ci != w.ci_pitch or pro_scale.numel() < Ci or pro_shift.numel() < Ci:
        raise ValueError("conv2d_pro: operand / prologue vector mismatch")
    if x.dtype != torch.bfloat16:
        raise _l.FlairHipError("conv2d_pro: bf16 only")
    out = torch.empty((B, H, W, out_channels), dtype=x.dtype, device=x.device)
    call = _conv_call(_l.CONV_UPCAT if up else _l.CONV_PLAIN, _dt(x), w, (B, H, W, H, W, out_channels), 1, relu=relu,
                      c1=Ci if up else 0, x=x, bias=bias, residual=residual, out=out, stats=stats,
                      pro=(pro_scale, pro_shift))
    _conv_run(call, "conv2d_pro", stats)
    return out


def conv2d_pro_bn_stats(x: torch.Tensor, w: PackedWeight, out_channels: int, pro_scale, pro_shift, gamma, beta,
                        running_mean, running_var, momentum: float, eps: float, up: bool = False):
    """conv2d_pro + batch statistics of its output -> (y0, scale, shift, mean, rstd)"""
    B, Hs, Ws, Ci = x.shape
    H, W = (2 * Hs, 2 * Ws) if up else (Hs, Ws)
    form, c1 = (_l.CONV_UPCAT, Ci) if up else (_l.CONV_PLAIN, 0)
    rows = _conv_route(_operand_call(_dt(x), w, B, H, W, form=form, c1=c1, pro=True, stats=True), "conv2d_pro").ntiles
    part = workspace(rows * 2 * out_channels * 4, x.device, "bnpart").view(torch.float32)
    y0 = conv2d_pro(x, w, out_channels, pro_scale, pro_shift, stats=part, up=up)
    return (y0,) + _bn_finalize(part, rows, B * H * W, out_channels, gamma, beta, running_mean, running_var, momentum, eps)


def conv_wgrad_pro(x: torch.Tensor, dy: torch.Tensor, co_real: int, ci_real: int, pro_scale: torch.Tensor,
                   pro_shift: torch.Tensor, up: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW of the 3x3 pad-1 conv whose input was relu(x * pro_scale + pro_shift) (ffa_conv_wgrad_pro)"""
    lib = _l.load()
    _chk_nhwc(x, "wgrad input")
    _chk_nhwc(dy, "wgrad dy")
    B, Hs, Ws, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    did = _dt(x)
    need = lib.ffa_conv_wgrad_workspace_bytes(did, 3, 3, 1, Co, Ci, B, Ho, Wo)
    if need < 0:
        raise _l.FlairHipError("no wgrad kernel")
    ws = workspace(need, x.device, "wgrad")
    if out is None:
        out = torch.empty((co_real, ci_real, 3, 3), dtype=torch.float32, device=x.device)
    _l.check(lib.ffa_conv_wgrad_pro(did, x.data_ptr(), dy.data_ptr(), out.data_ptr(), pro_scale.data_ptr(),
                                    pro_shift.data_ptr(), B, Ho, Wo, Ci, Ho, Wo, Co, co_real, ci_real, 1 if up else 0, 0,
                                    ws.data_ptr(), ws.numel(), _stream()), "conv_wgrad_pro")
    return out


def upcat_supported(c1: int, c2: int, dtype: torch.dtype) -> bool:
    """Channel splits the two-source kernels take (forward: C1 covers whole halo channel groups; weight gradient: C1 is
    a multiple of a block's input channels)."""
    return FUSED_UPCAT and bool(_l.load().ffa_conv_upcat_supported(_dtype_id(dtype), c1, c2))


FUSED_UPCAT_BWD = os.environ.get("FFA_FUSED_UPCAT_BWD", "1") != "0"  # A/B: plain dgrad + up2_concat_bwd
FUSED_UPCAT = os.environ.get("FFA_FUSED_UPCAT", "1") != "0"  # A/B switch: materialise the decoder concat instead


def conv2d_upcat_bn_stats(lo: torch.Tensor, skip: Optional[torch.Tensor], w: PackedWeight, out_channels: int, gamma,
                          beta, running_mean, running_var, momentum: float, eps: float):
    """conv2d_upcat + batch statistics of its output -> (y0, scale, shift, mean, rstd)"""
    B, Hl, Wl, C1 = lo.shape
    Ho, Wo = 2 * Hl, 2 * Wl
    rows = _conv_route(_operand_call(_dt(lo), w, B, Ho, Wo, form=_l.CONV_UPCAT, c1=C1, stats=True),
                       "conv2d_upcat (check upcat_supported first)").ntiles
    part = workspace(rows * 2 * out_channels * 4, lo.device, "bnpart").view(torch.float32)
    y0 = conv2d_upcat(lo, skip, w, out_channels, stats=part)
    if y0 is None:
        raise _l.FlairHipError("conv2d_upcat: unsupported channel split (check upcat_supported first)")
    return (y0,) + _bn_finalize(part, rows, B * Ho * Wo, out_channels, gamma, beta, running_mean, running_var,
                                momentum, eps)


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, co_real: int, ci_real: int, kh: int, kw: int, stride: int,
               pad: int, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """dW (OIHW f32, [co_real, ci_real, kh, kw]) from the conv input x and the output gradient dy."""
    lib = _l.load()
    _chk_nhwc(x, "wgrad input")
    _chk_nhwc(dy, "wgrad dy")
    B, Hi, Wi, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    did = _dt(x)
    need = lib.ffa_conv_wgrad_workspace_bytes(did, kh, kw, stride, Co, Ci, B, Ho, Wo)
    if need < 0:
        raise _l.FlairHipError(f"no wgrad kernel for {kh}x{kw} stride {stride}")
    ws = workspace(need, x.device, "wgrad")
    if out is None:
        out = torch.empty((co_real, ci_real, kh, kw), dtype=torch.float32, device=x.device)
    _l.check(lib.ffa_conv_wgrad(did, x.data_ptr(), dy.data_ptr(), out.data_ptr(), B, Hi, Wi, Ci, Ho, Wo, Co, co_real,
                                ci_real, kh, kw, stride, pad, 1 if accumulate else 0, ws.data_ptr(), ws.numel(),
                                _stream()), "conv_wgrad")
    return out


def conv_wgrad_upcat(lo: torch.Tensor, skip: Optional[torch.Tensor], dy: torch.Tensor, co_real: int,
                     out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """dW [co_real, C1 + C2, 3, 3] of the conv over cat(nearest_x2(lo), skip); None when unsupported."""
    lib = _l.load()
    _chk_nhwc(lo, "wgrad lo")
    _chk_nhwc(dy, "wgrad dy")
    B, Hl, Wl, C1 = lo.shape
    C2 = 0 if skip is None else skip.shape[3]
    Co = dy.shape[3]
    did = _dt(lo)
    need = lib.ffa_conv_wgrad_workspace_bytes(did, 3, 3, 1, Co, C1 + C2, B, 2 * Hl, 2 * Wl)
    if need < 0:
        return None
    ws = workspace(need, lo.device, "wgrad")
    if out is None:
        out = torch.empty((co_real, C1 + C2, 3, 3), dtype=torch.float32, device=lo.device)
    rc = lib.ffa_conv_wgrad_upcat(did, lo.data_ptr(), _ptr(skip), dy.data_ptr(), out.data_ptr(), B, Hl, Wl, C1, C2, Co,
                                  co_real, 0, ws.data_ptr(), ws.numel(), _stream())
    if rc == _l.ERR_UNSUPPORTED:
        return None
    _l.check(rc, "conv_wgrad_upcat")
    return out


# --------------------------------------------------------------------------------------------------
# normalisation / pooling

def bn_stats(x: torch.Tensor, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """Batch statistics of x (NHWC) -> (scale, shift, mean, rstd); updates the running buffers in place."""
    lib = _l.load()
    _chk_nhwc(x, "bn input")
    C_ = x.shape[-1]
    npix = x.numel() // C_
    dev = x.device
    out = torch.empty((4, C_), dtype=torch.float32, device=dev)
    ws = workspace(lib.ffa_bn_workspace_bytes(C_), dev, "bn")
    _l.check(lib.ffa_bn_stats(_dt(x), x.data_ptr(), npix, C_, _ptr(gamma), _ptr(beta), _ptr(running_mean),
                              _ptr(running_var), momentum, eps, out[0].data_ptr(), out[1].data_ptr(),
                              out[2].data_ptr(), out[3].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "bn_stats")
    return out[0], out[1], out[2], out[3]


def bn_eval_params(gamma, beta, running_mean, running_var, eps: float):
    lib = _l.load()
    C_ = running_mean.numel()
    out = torch.empty((2, C_), dtype=torch.float32, device=running_mean.device)
    _l.check(lib.ffa_bn_eval_params(C_, _ptr(gamma), _ptr(beta), running_mean.data_ptr(), running_var.data_ptr(), eps,
                                    out[0].data_ptr(), out[1].data_ptr(), _stream()), "bn_eval_params")
    return out[0], out[1]


def bn_apply(x: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, residual: Optional[torch.Tensor] = None,
             relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _l.load()
    _chk_nhwc(x, "bn_apply input")
    C_ = x.shape[-1]
    if out is None:
        out = torch.empty_like(x)
    _l.check(lib.ffa_bn_apply(_dt(x), x.data_ptr(), _ptr(residual), out.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                              x.numel() // C_, C_, 1 if relu else 0, _stream()), "bn_apply")
    return out


# one-kernel BatchNorm backward for tensors that fit the chip's registers: OFF by default (FFA_BN_BWD_COOP=1 enables).
# Measured: a grid-wide barrier across the eight XCDs costs ~20-25 us, two of them more than the two launches and
# the two passes they save (72-76 us per call whatever the tensor size, against 24-55 us for reduce + finalize +
# apply on the tensors that fit; 15.49 -> 16.81 ms per training step).  Kept as the measured negative result.
FUSED_BN_BWD_COOP = os.environ.get("FFA_BN_BWD_COOP", "0") == "1"
_COOP_SYNC = {}


def _coop_sync(device) -> torch.Tensor:
    """barrier counters of ffa_bn_bwd_fused: zeroed once per device, re-armed by every launch"""
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _COOP_SYNC.get(key)
    if t is None:
        t = _COOP_SYNC[key] = torch.zeros(4, dtype=torch.int32, device=device)
    return t


def coop_barrier_failed(device=None) -> bool:
    """True when a grid barrier of ffa_bn_bwd_fused ever timed out on this device (synchronises)"""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    t = _COOP_SYNC.get(key)
    return bool(t is not None and int(t[3].item()) != 0)


# set by bench.py's roofline pass: called as hook(run_stage, x, has_y, has_dres) instead of the single ffa_bn_bwd call
BN_BWD_STAGE_HOOK = None


def bn_bwd(x: torch.Tensor, dy: torch.Tensor, y: Optional[torch.Tensor], gamma, beta, mean, rstd, relu: bool,
           want_dres: bool, out_dgamma: Optional[torch.Tensor] = None, out_dbeta: Optional[torch.Tensor] = None):
    """-> (dx, dres or None, dgamma, dbeta).  With relu and y=None the ReLU mask is recomputed from x
    (only valid when no residual was added before the ReLU).  out_dgamma / out_dbeta (f32, C elements, contiguous):
    where the affine gradients are written -- the slots of a data-parallel gradient bucket (flairhip.nn._vec_out)."""
    lib = _l.load()
    C_ = x.shape[-1]
    dev = x.device
    dx = torch.empty_like(x)
    dres = torch.empty_like(x) if want_dres else None
    if out_dgamma is not None and out_dbeta is not None:
        for t in (out_dgamma, out_dbeta):
            if t.dtype != torch.float32 or t.numel() != C_ or not t.is_contiguous() or t.device != dev:
                raise ValueError("bn_bwd: output vectors must be contiguous f32 of C elements on the input's device")
        dgb = (out_dgamma, out_dbeta)
    else:
        dgb = torch.empty((2, C_), dtype=torch.float32, device=dev)
    ws = workspace(lib.ffa_bn_workspace_bytes(C_), dev, "bn")
    mode = 0 if not relu else (1 if y is not None else 2)
    if FUSED_BN_BWD_COOP and x.dtype == torch.bfloat16:
        sync = _coop_sync(dev)
        rc = lib.ffa_bn_bwd_fused(_dt(x), x.data_ptr(), dy.data_ptr(), _ptr(y), _ptr(gamma), _ptr(beta),
                                  mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(), _ptr(dres), dgb[0].data_ptr(),
                                  dgb[1].data_ptr(), x.numel() // C_, C_, mode, ws.data_ptr(), ws.numel(),
                                  sync.data_ptr(), _stream())
        if rc == 0:
            return dx, dres, dgb[0], dgb[1]
        if rc != _l.ERR_UNSUPPORTED:
            _l.check(rc, "bn_bwd_fused")
    args = (_dt(x), x.data_ptr(), dy.data_ptr(), _ptr(y), _ptr(gamma), _ptr(beta), mean.data_ptr(), rstd.data_ptr(),
            dx.data_ptr(), _ptr(dres), dgb[0].data_ptr(), dgb[1].data_ptr(), x.numel() // C_, C_, mode, ws.data_ptr(),
            ws.numel())
    if BN_BWD_STAGE_HOOK is not None:  # measurement harness: the two stages as separate calls (same kernels)
        BN_BWD_STAGE_HOOK(lambda stages: _l.check(lib.ffa_bn_bwd_stages(*args, stages, _stream()), "bn_bwd"),
                          x, y is not None, dres is not None)
    else:
        _l.check(lib.ffa_bn_bwd(*args, _stream()), "bn_bwd")
    return dx, dres, dgb[0], dgb[1]


def channel_sums(x: torch.Tensor):
    """Per-channel (sum, sum of squares) over all pixels of an NHWC tensor, f32."""
    lib = _l.load()
    _chk_nhwc(x, "channel_sums input")
    C_ = x.shape[-1]
    out = torch.empty((2, C_), dtype=torch.float32, device=x.device)
    ws = workspace(lib.ffa_bn_workspace_bytes(C_), x.device, "bn")
    _l.check(lib.ffa_channel_sums(_dt(x), x.data_ptr(), x.numel() // C_, C_, out[0].data_ptr(), out[1].data_ptr(),
                                  ws.data_ptr(), ws.numel(), _stream()), "channel_sums")
    return out[0], out[1]


def maxpool3x3s2_fwd(x: torch.Tensor):
    lib = _l.load()
    _chk_nhwc(x, "maxpool input")
    B, H, W, C_ = x.shape
    Ho, Wo = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    y = torch.empty((B, Ho, Wo, C_), dtype=x.dtype, device=x.device)
    idx = torch.empty((B, Ho, Wo, C_), dtype=torch.uint8, device=x.device)
    _l.check(lib.ffa_maxpool3x3s2_fwd(_dt(x), x.data_ptr(), y.data_ptr(), idx.data_ptr(), B, H, W, C_, _stream()),
             "maxpool_fwd")
    return y, idx


def maxpool3x3s2_bwd(dy: torch.Tensor, idx: torch.Tensor, in_hw: Tuple[int, int],
                     add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = route(dy, idx) (+ add: another gradient of the pooled tensor's input, summed in the same pass)"""
    lib = _l.load()
    B, _, _, C_ = dy.shape
    H, W = in_hw
    dx = torch.empty((B, H, W, C_), dtype=dy.dtype, device=dy.device)
    if add is not None and (tuple(add.shape) != tuple(dx.shape) or add.dtype != dx.dtype or not add.is_contiguous()):
        raise ValueError("maxpool3x3s2_bwd: add must be a contiguous tensor of the input's shape and dtype")
    _l.check(lib.ffa_maxpool3x3s2_bwd(_dt(dy), dy.data_ptr(), idx.data_ptr(), _ptr(add), dx.data_ptr(), B, H, W, C_,
                                      _stream()), "maxpool_bwd")
    return dx


# --------------------------------------------------------------------------------------------------
# layout / resampling

def nchw_to_nhwc(x: torch.Tensor, dtype: torch.dtype, cp: Optional[int] = None) -> torch.Tensor:
    """f32 NCHW batch tensor -> NHWC compute tensor with zero-filled pad channels."""
    lib = _l.load()
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    B, C_, H, W = x.shape
    cp = cp or pad_channels(C_)
    out = torch.empty((B, H, W, cp), dtype=dtype, device=x.device)
    _l.check(lib.ffa_nchw_to_nhwc(_dtype_id(dtype), x.data_ptr(), out.data_ptr(), B, C_, H, W, cp, _stream()),
             "nchw_to_nhwc")
    return out


def u8_nchw_to_nhwc(x: torch.Tensor, dtype: torch.dtype, mean: torch.Tensor, std: torch.Tensor,
                    cp: Optional[int] = None) -> torch.Tensor:
    """uint8 [B,C,H,W] -> NHWC compute tensor holding (x - mean[c]) / std[c]; mean / std f32 device vectors [C]"""
    lib = _l.load()
    if x.dtype != torch.uint8 or x.ndim != 4 or not x.is_contiguous():
        raise ValueError("u8_nchw_to_nhwc: contiguous uint8 [B,C,H,W] expected")
    B, C_, H, W = x.shape
    if mean.numel() < C_ or std.numel() < C_ or mean.dtype != torch.float32 or std.dtype != torch.float32:
        raise ValueError("u8_nchw_to_nhwc: mean / std must be f32 vectors with one entry per channel")
    cp = pad_channels(C_) if cp is None else cp
    out = torch.empty((B, H, W, cp), dtype=dtype, device=x.device)
    _l.check(lib.ffa_u8_nchw_to_nhwc(_dtype_id(dtype), x.data_ptr(), out.data_ptr(), B, C_, H, W, cp, mean.data_ptr(),
                                     std.data_ptr(), _stream()), "u8_nchw_to_nhwc")
    return out


RAW_SAMPLE_KINDS = {torch.uint8: 0, torch.uint16: 1, torch.int16: 2, torch.float32: 3}  # FFA_SRC_*


def raw_nchw_to_nhwc(x: torch.Tensor, dtype: torch.dtype, mean: torch.Tensor, std: torch.Tensor,
                     cp: Optional[int] = None) -> torch.Tensor:
    """raw raster samples (uint8 / uint16 / int16 / float32) [B,C,H,W] -> NHWC compute tensor holding
    (x - mean[c]) / std[c]; mean / std f32 device vectors [C]"""
    lib = _l.load()
    if x.dtype not in RAW_SAMPLE_KINDS or x.ndim != 4 or not x.is_contiguous():
        raise ValueError(f"raw_nchw_to_nhwc: contiguous [B,C,H,W] of uint8 / uint16 / int16 / float32 expected, "
                         f"got {x.dtype} {tuple(x.shape)}")
    B, C_, H, W = x.shape
    if mean.numel() < C_ or std.numel() < C_ or mean.dtype != torch.float32 or std.dtype != torch.float32:
        raise ValueError("raw_nchw_to_nhwc: mean / std must be f32 vectors with one entry per channel")
    cp = pad_channels(C_) if cp is None else cp
    out = torch.empty((B, H, W, cp), dtype=dtype, device=x.device)
    _l.check(lib.ffa_raw_nchw_to_nhwc(_dtype_id(dtype), RAW_SAMPLE_KINDS[x.dtype], x.data_ptr(), out.data_ptr(), B, C_,
                                      H, W, cp, mean.data_ptr(), std.data_ptr(), _stream()), "raw_nchw_to_nhwc")
    return out


def _d4_codes(codes: torch.Tensor, n: int, dev, what: str) -> torch.Tensor:
    """per-sample augmentation codes (flairhip.augment): uint8 [n] on the device.  Only shape and dtype are looked at:
    the values stay on the device (a captured step replays with new ones)."""
    if not torch.is_tensor(codes) or codes.dtype != torch.uint8 or codes.ndim != 1 or codes.numel() != n:
        raise ValueError(f"{what}: codes must be a uint8 vector with one entry per sample ({n})")
    if codes.device != dev:
        raise ValueError(f"{what}: codes live on {codes.device}, the data on {dev}")
    return codes.contiguous()


def d4_layout(x: torch.Tensor, dtype: torch.dtype, codes: torch.Tensor, mean: Optional[torch.Tensor] = None,
              std: Optional[torch.Tensor] = None, cp: Optional[int] = None, group: int = 1) -> torch.Tensor:
    """nchw_to_nhwc / u8_nchw_to_nhwc / raw_nchw_to_nhwc of the flipped / rotated images in one pass: image b of the
    contiguous [B,C,n,n] tensor (uint8 / uint16 / int16 with mean and std, float32 with or without) is read through the
    gather of ``codes[b // group]`` (flairhip.augment.d4_source_index).  Same values, bit for bit, as the plain kernel
    on a pre-permuted input."""
    lib = _l.load()
    if x.dtype not in RAW_SAMPLE_KINDS or x.ndim != 4 or not x.is_contiguous():
        raise ValueError(f"d4_layout: contiguous [B,C,H,W] of uint8 / uint16 / int16 / float32 expected, "
                         f"got {x.dtype} {tuple(x.shape)}")
    B, C_, H, W = x.shape
    if H != W:
        raise ValueError(f"d4_layout: rotations need square planes, got {H} x {W}")
    if group < 1 or B % group:
        raise ValueError(f"d4_layout: {B} images do not split into groups of {group}")
    if (mean is None) != (std is None) or (mean is None and x.dtype != torch.float32):
        raise ValueError("d4_layout: mean and std come together, and integer samples need them")
    if mean is not None and (mean.numel() < C_ or std.numel() < C_ or mean.dtype != torch.float32 or
                             std.dtype != torch.float32):
        raise ValueError("d4_layout: mean / std must be f32 vectors with one entry per channel")
    codes = _d4_codes(codes, B // group, x.device, "d4_layout")
    cp = pad_channels(C_) if cp is None else cp
    out = torch.empty((B, H, W, cp), dtype=dtype, device=x.device)
    _l.check(lib.ffa_d4_nchw_to_nhwc(_dtype_id(dtype), RAW_SAMPLE_KINDS[x.dtype], x.data_ptr(), out.data_ptr(), B, C_, H,
                                     W, cp, _ptr(mean), _ptr(std), codes.data_ptr(), group, _stream()), "d4_layout")
    return out


def d4_labels(t: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """uint8 class-index maps [B,n,n] -> the flipped / rotated maps (same gather as d4_layout)"""
    lib = _l.load()
    if t.dtype != torch.uint8 or t.ndim != 3 or not t.is_contiguous():
        raise ValueError("d4_labels: contiguous uint8 [B,H,W] expected")
    B, H, W = t.shape
    if H != W:
        raise ValueError(f"d4_labels: rotations need square planes, got {H} x {W}")
    codes = _d4_codes(codes, B, t.device, "d4_labels")
    out = torch.empty_like(t)
    _l.check(lib.ffa_d4_labels_u8(t.data_ptr(), out.data_ptr(), B, H, W, codes.data_ptr(), _stream()), "d4_labels")
    return out


def d4_onehot_to_index(onehot: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """onehot_to_index (first maximum) of the flipped / rotated one-hot map [B,K,n,n], in one pass"""
    lib = _l.load()
    if onehot.dtype != torch.float32 or not onehot.is_contiguous():
        onehot = onehot.float().contiguous()
    B, K, H, W = onehot.shape
    if H != W:
        raise ValueError(f"d4_onehot_to_index: rotations need square planes, got {H} x {W}")
    codes = _d4_codes(codes, B, onehot.device, "d4_onehot_to_index")
    out = torch.empty((B, H, W), dtype=torch.uint8, device=onehot.device)
    _l.check(lib.ffa_d4_onehot_to_index(onehot.data_ptr(), out.data_ptr(), B, K, H, W, codes.data_ptr(), _stream()),
             "d4_onehot_to_index")
    return out


ELEV_NONE, ELEV_DIFF, ELEV_STACK = 0, 1, 2  # FFA_ELEV_*
ELEV_CHANNELS = {ELEV_NONE: None, ELEV_DIFF: 1, ELEV_STACK: 2}


def _gather_index(index: torch.Tensor, n: int, dev, what: str) -> torch.Tensor:
    """the index vector of a gather: int32 [B] on the device.  A host tensor is validated against [0, n) here and
    copied over; the values of a device tensor stay on the device (a captured step replays with new ones: the kernels
    clamp, the caller answers for the range)."""
    if not torch.is_tensor(index) or index.dtype != torch.int32 or index.ndim != 1 or index.numel() < 1:
        raise ValueError(f"{what}: index must be a non-empty int32 vector")
    if not index.is_cuda:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= n:
            raise ValueError(f"{what}: index values {lo}..{hi} outside the store's [0, {n})")
        return index.to(dev, non_blocking=True)
    if index.device != dev:
        raise ValueError(f"{what}: index lives on {index.device}, the store on {dev}")
    return index.contiguous()


def gather_layout(store: torch.Tensor, index: torch.Tensor, dtype: torch.dtype, codes: Optional[torch.Tensor] = None,
                  mean: Optional[torch.Tensor] = None, std: Optional[torch.Tensor] = None, cp: Optional[int] = None,
                  elevation: int = ELEV_NONE, group: int = 1) -> torch.Tensor:
    """A batch from a device-resident sample store: image b of the NHWC result is image ``index[b]`` of the raw
    contiguous store [N,C,H,W] (uint8 / uint16 / int16 with mean and std, float32 with or without), read through the
    gather of ``codes[b // group]`` and normalised, in one pass.  ``codes=None`` is the identity and allows H != W.
    ``elevation``: 0 channels as stored; 1 the one channel z0 - z1 of a 2-band DEM (the reference's calc_elevation);
    2 the two channels (z0, z0 - z1) (calc_elevation_stack_dsm); mean / std then have one entry per OUTPUT channel.
    With ``elevation=0`` the result equals ``d4_layout(store[index], ...)`` bit for bit."""
    lib = _l.load()
    if not torch.is_tensor(store) or store.dtype not in RAW_SAMPLE_KINDS or store.ndim != 4 or not store.is_cuda or \
            not store.is_contiguous() or store.numel() == 0:
        raise ValueError("gather_layout: contiguous device store [N,C,H,W] of uint8 / uint16 / int16 / float32 expected")
    N, C_, H, W = store.shape
    if elevation not in ELEV_CHANNELS:
        raise ValueError(f"gather_layout: unknown elevation mode {elevation}")
    if elevation != ELEV_NONE and C_ != 2:
        raise ValueError(f"gather_layout: the elevation modes need the 2 bands of a DEM, got {C_}")
    c_out = ELEV_CHANNELS[elevation] or C_
    if codes is not None and H != W:
        raise ValueError(f"gather_layout: rotations need square planes, got {H} x {W}")
    index = _gather_index(index, N, store.device, "gather_layout")
    B = index.numel()
    if group < 1 or B % group:
        raise ValueError(f"gather_layout: {B} images do not split into groups of {group}")
    if (mean is None) != (std is None) or (mean is None and store.dtype != torch.float32):
        raise ValueError("gather_layout: mean and std come together, and integer samples need them")
    if mean is not None and (mean.numel() < c_out or std.numel() < c_out or mean.dtype != torch.float32 or
                             std.dtype != torch.float32 or mean.device != store.device or
                             std.device != store.device or not mean.is_contiguous() or not std.is_contiguous()):
        raise ValueError("gather_layout: mean / std must be contiguous f32 device vectors with one entry per output "
                         "channel")
    if codes is not None:
        codes = _d4_codes(codes, B // group, store.device, "gather_layout")
    cp = pad_channels(c_out) if cp is None else cp
    if cp % 8 or cp < c_out:
        raise ValueError(f"gather_layout: channel pitch {cp} must be a multiple of 8 and hold {c_out} channels")
    out = torch.empty((B, H, W, cp), dtype=dtype, device=store.device)
    _l.check(lib.ffa_gather_layout(_dtype_id(dtype), RAW_SAMPLE_KINDS[store.dtype], store.data_ptr(), index.data_ptr(),
                                   out.data_ptr(), N, B, C_, H, W, cp, _ptr(mean), _ptr(std), _ptr(codes), group,
                                   elevation, _stream()), "gather_layout")
    return out


def gather_labels(store: torch.Tensor, index: torch.Tensor, num_classes: int,
                  codes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 label store [N,H,W] (the raw label channel of every patch) -> uint8 class indices [B,H,W] of the samples
    ``index``, flipped / rotated by ``codes`` like the inputs.  The label rule is the reference's
    ``argmax(reshape_label_ohe(label, K))``: a value v < K stays v, and a value v >= K becomes **0** -- its one-hot
    is all false, and the argmax of an all-false vector is 0.  Such pixels train as class 0; they are not ignored."""
    lib = _l.load()
    if not torch.is_tensor(store) or store.dtype != torch.uint8 or store.ndim != 3 or not store.is_cuda or \
            not store.is_contiguous() or store.numel() == 0:
        raise ValueError("gather_labels: contiguous uint8 device store [N,H,W] expected")
    N, H, W = store.shape
    if not 1 <= int(num_classes) <= 256:
        raise ValueError(f"gather_labels: {num_classes} classes do not fit a byte")
    if codes is not None and H != W:
        raise ValueError(f"gather_labels: rotations need square planes, got {H} x {W}")
    index = _gather_index(index, N, store.device, "gather_labels")
    B = index.numel()
    if codes is not None:
        codes = _d4_codes(codes, B, store.device, "gather_labels")
    out = torch.empty((B, H, W), dtype=torch.uint8, device=store.device)
    _l.check(lib.ffa_gather_labels_u8(store.data_ptr(), index.data_ptr(), out.data_ptr(), N, B, H, W, int(num_classes),
                                      _ptr(codes), _stream()), "gather_labels")
    return out


def gather_series(store, index: torch.Tensor, T: int, dtype: torch.dtype, codes: Optional[torch.Tensor] = None,
                  cp: Optional[int] = None, fill: float = 0.0, pad_value: float = 0.0):
    """The padded batch of a U-TAE branch from a ragged flairhip.sample_store.SeriesStore: -> (nhwc [B*T,H,W,cp] of
    ``dtype``, pad uint8 [B*T]).  Image b*T + t is date t of sample ``index[b]`` read through the gather of
    ``codes[b]`` (``None``: the identity, H != W allowed), widened to f32 and converted, not normalised; the dates past
    the sample's length hold ``fill`` (what pad_collate_flair pads with).  ``pad`` is the store's flag of a stored date
    and ``fill == pad_value`` of a padded one.  Both equal, bit for bit, ``d4_layout(x, dtype, codes, cp=cp, group=T)``
    and ``detect_pad_images(x, pad_value)`` on the padded f32 batch x.  A host ``index`` is checked against the
    store's host offsets (range, longest series <= T); the values of a device ``index`` stay on the device."""
    data = getattr(store, "data", None)
    if not torch.is_tensor(data) or data.dtype not in RAW_SAMPLE_KINDS or data.ndim != 4 or \
            not data.is_contiguous() or data.numel() == 0:
        raise ValueError("gather_series: a SeriesStore with contiguous data [D,C,h,w] of uint8 / uint16 / int16 / float32 "
                         "expected")
    D, C_, H, W = data.shape
    N, T = int(store.n), int(T)
    if T < 1:
        raise ValueError(f"gather_series: T = {T} dates")
    if codes is not None and H != W:
        raise ValueError(f"gather_series: rotations need square planes, got {H} x {W}")
    if not torch.is_tensor(index) or index.dtype != torch.int32 or index.ndim != 1 or index.numel() < 1:
        raise ValueError("gather_series: index must be a non-empty int32 vector")
    if not index.is_cuda:
        lo, hi = int(index.min()), int(index.max())
        if lo < 0 or hi >= N:
            raise ValueError(f"gather_series: index values {lo}..{hi} outside the store's [0, {N})")
        longest = int(store.lengths[index.numpy()].max())
        if longest > T:
            raise ValueError(f"gather_series: the longest indexed series has {longest} dates, T = {T}")
    cp = pad_channels(C_) if cp is None else int(cp)
    if cp % 8 or cp < C_:
        raise ValueError(f"gather_series: channel pitch {cp} must be a multiple of 8 and hold {C_} channels")
    if not data.is_cuda:
        raise ValueError("gather_series: the store lives on the host; the gather runs on the device")
    lib = _l.load()
    index = _gather_index(index, N, data.device, "gather_series")
    B = index.numel()
    if codes is not None:
        codes = _d4_codes(codes, B, data.device, "gather_series")
    offsets, is_pad = store.offsets, store.is_pad
    if offsets.dtype != torch.int32 or offsets.numel() != N + 1 or offsets.device != data.device or \
            is_pad.dtype != torch.uint8 or is_pad.numel() != D or is_pad.device != data.device or \
            not offsets.is_contiguous() or not is_pad.is_contiguous():
        raise ValueError("gather_series: offsets int32 [N + 1] and is_pad uint8 [D] must live next to the data")
    out = torch.empty((B * T, H, W, cp), dtype=dtype, device=data.device)
    pad = torch.empty(B * T, dtype=torch.uint8, device=data.device)
    _l.check(lib.ffa_gather_series(_dtype_id(dtype), RAW_SAMPLE_KINDS[data.dtype], data.data_ptr(), offsets.data_ptr(),
                                   is_pad.data_ptr(), index.data_ptr(), out.data_ptr(), pad.data_ptr(), N, B, T, C_, H,
                                   W, cp, float(fill), int(float(fill) == float(pad_value)), _ptr(codes), _stream()),
             "gather_series")
    return out, pad


def nhwc_to_nchw(x: torch.Tensor, channels: int) -> torch.Tensor:
    lib = _l.load()
    _chk_nhwc(x, "nhwc_to_nchw input")
    B, H, W, cp = x.shape
    out = torch.empty((B, channels, H, W), dtype=torch.float32, device=x.device)
    _l.check(lib.ffa_nhwc_to_nchw(_dt(x), x.data_ptr(), out.data_ptr(), B, channels, H, W, cp, _stream()),
             "nhwc_to_nchw")
    return out


def upsample2x_concat_fwd(lo: torch.Tensor, skip: Optional[torch.Tensor]) -> torch.Tensor:
    lib = _l.load()
    _chk_nhwc(lo, "upsample input")
    B, Hl, Wl, C1 = lo.shape
    C2 = 0 if skip is None else skip.shape[-1]
    if skip is not None and tuple(skip.shape[:3]) != (B, 2 * Hl, 2 * Wl):
        raise ValueError(f"upsample2x_concat: skip {tuple(skip.shape)} does not match 2x of {tuple(lo.shape)}")
    out = torch.empty((B, 2 * Hl, 2 * Wl, C1 + C2), dtype=lo.dtype, device=lo.device)
    _l.check(lib.ffa_upsample_nearest2x_concat_fwd(_dt(lo), lo.data_ptr(), _ptr(skip), out.data_ptr(), B, Hl, Wl, C1,
                                                   C2, _stream()), "upsample2x_concat_fwd")
    return out


def upsample2x_concat_bwd(dcat: torch.Tensor, c1: int, skip_as_view: bool = False):
    """-> (dlo, dskip).  With ``skip_as_view`` the skip gradient is the channel slice of ``dcat`` itself (no copy):
    fine for a consumer that reads strided input, e.g. the sum with the encoder-side gradient of the same map."""
    lib = _l.load()
    _chk_nhwc(dcat, "upsample grad")
    B, H, W, C_ = dcat.shape
    c2 = C_ - c1
    dlo = torch.empty((B, H // 2, W // 2, c1), dtype=dcat.dtype, device=dcat.device)
    dskip = torch.empty((B, H, W, c2), dtype=dcat.dtype, device=dcat.device) if (c2 and not skip_as_view) else None
    _l.check(lib.ffa_upsample_nearest2x_concat_bwd(_dt(dcat), dcat.data_ptr(), dlo.data_ptr(), _ptr(dskip), B, H // 2,
                                                   W // 2, c1, c2, _stream()), "upsample2x_concat_bwd")
    if c2 and skip_as_view:
        dskip = dcat[..., c1:]
    return dlo, dskip


def bilinear_fwd(x: torch.Tensor, out_hw: Tuple[int, int]) -> torch.Tensor:
    lib = _l.load()
    _chk_nhwc(x, "bilinear input")
    B, Hi, Wi, C_ = x.shape
    Ho, Wo = out_hw
    y = torch.empty((B, Ho, Wo, C_), dtype=x.dtype, device=x.device)
    _l.check(lib.ffa_bilinear_fwd(_dt(x), x.data_ptr(), y.data_ptr(), B, Hi, Wi, Ho, Wo, C_, _stream()),
             "bilinear_fwd")
    return y


def bilinear_bwd(dy: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    lib = _l.load()
    _chk_nhwc(dy, "bilinear grad")
    B, Ho, Wo, C_ = dy.shape
    Hi, Wi = in_hw
    dx = torch.empty((B, Hi, Wi, C_), dtype=dy.dtype, device=dy.device)
    # gather-form backward: fixed summation order, no scratch image (the workspace arguments stay in the ABI)
    _l.check(lib.ffa_bilinear_bwd(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, Hi, Wi, Ho, Wo, C_, None, 0, _stream()),
             "bilinear_bwd")
    return dx


# --------------------------------------------------------------------------------------------------
# loss / prediction

def softmax_ce(logits: torch.Tensor, targets: torch.Tensor, class_weights: torch.Tensor, num_classes: int,
               grad_scale: Optional[torch.Tensor] = None, want_grad: bool = False, want_pred: bool = False,
               want_sums: bool = False):
    """Weighted-mean cross-entropy over NHWC logits [B,H,W,Cp] and uint8 targets [B,H,W].

    -> (loss[1] f32, wsum[1] f32, dlogits or None, pred uint8 or None); with want_sums (needs want_grad) a fifth value:
    the per-class sums [Cp] f32 of dlogits over all pixels (the bias gradient of the layer that produced the logits),
    or None where the library cannot take them in the same pass.
    """
    lib = _l.load()
    _chk_nhwc(logits, "logits")
    if targets.dtype != torch.uint8 or not targets.is_contiguous():
        raise ValueError("softmax_ce: targets must be contiguous uint8 class indices")
    cp = logits.shape[-1]
    npix = logits.numel() // cp
    if targets.numel() != npix:
        raise ValueError("softmax_ce: target / logit pixel count mismatch")
    dev = logits.device
    res = torch.empty(2, dtype=torch.float32, device=dev)
    dlogits = torch.empty_like(logits) if want_grad else None
    pred = torch.empty(targets.shape, dtype=torch.uint8, device=dev) if want_pred else None
    if want_grad and grad_scale is None:
        grad_scale = torch.ones(1, dtype=torch.float32, device=dev)
    ws = workspace(lib.ffa_softmax_ce_workspace_bytes(), dev, "ce")
    if want_sums:
        sums = torch.empty(cp, dtype=torch.float32, device=dev) if want_grad else None
        rc = _l.ERR_UNSUPPORTED
        if sums is not None:
            rc = lib.ffa_softmax_ce_sums(_dt(logits), logits.data_ptr(), targets.data_ptr(), class_weights.data_ptr(),
                                         _ptr(grad_scale), res[0:1].data_ptr(), res[1:2].data_ptr(), _ptr(dlogits),
                                         _ptr(pred), sums.data_ptr(), npix, num_classes, cp, ws.data_ptr(), ws.numel(),
                                         _stream())
        if rc == 0:
            return res[0:1], res[1:2], dlogits, pred, sums
        if rc != _l.ERR_UNSUPPORTED:
            _l.check(rc, "softmax_ce_sums")
    _l.check(lib.ffa_softmax_ce(_dt(logits), logits.data_ptr(), targets.data_ptr(), class_weights.data_ptr(),
                                _ptr(grad_scale), res[0:1].data_ptr(), res[1:2].data_ptr(), _ptr(dlogits), _ptr(pred),
                                npix, num_classes, cp, ws.data_ptr(), ws.numel(), _stream()), "softmax_ce")
    if want_sums:
        return res[0:1], res[1:2], dlogits, pred, None
    return res[0:1], res[1:2], dlogits, pred


def scale_inplace(x: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """x *= scale[0] (device f32 scalar) in place; the kernel returns at once when the scalar is exactly 1."""
    lib = _l.load()
    if not x.is_contiguous() or x.numel() % 8:
        raise ValueError("scale_inplace: contiguous tensor with a multiple of 8 elements expected")
    _l.check(lib.ffa_scale_inplace(_dt(x), x.data_ptr(), x.numel(), scale.data_ptr(), _stream()), "scale_inplace")
    return x


_PREDICT_MODES = {"argmax": 0, "class_prob": 1, "argmax_conf": 2}


def predict_u8(logits: torch.Tensor, num_classes: int, mode: str = "argmax", crop: Optional[Tuple[int, int, int, int]] = None
               ) -> torch.Tensor:
    """NHWC logits -> uint8 prediction of the cropped window (y0, x0, h, w).

    'argmax' -> [B, h, w];  'class_prob' -> [B, K, h, w] = rint(softmax * 255)
    (flair_zonal_detection/postprocess.py:9-30 semantics; unknown modes raise ValueError like the reference);
    'argmax_conf' -> [B, 2, h, w]: plane 0 the 'argmax' output, plane 1 the confidence rint(255 * max softmax) = the
    maximum over the bands of the 'class_prob' output, both bit for bit, from one pass over the logits.
    """
    lib = _l.load()
    _chk_nhwc(logits, "logits")
    if mode not in _PREDICT_MODES:
        raise ValueError(f"Unknown output type: {mode}")
    B, H, W, cp = logits.shape
    y0, x0, h, w = crop if crop is not None else (0, 0, H, W)
    shape = {"argmax": (B, h, w), "class_prob": (B, num_classes, h, w), "argmax_conf": (B, 2, h, w)}[mode]
    out = torch.empty(shape, dtype=torch.uint8, device=logits.device)
    _l.check(lib.ffa_predict_u8(_dt(logits), _PREDICT_MODES[mode], logits.data_ptr(), out.data_ptr(), B, H, W,
                                num_classes, cp, y0, x0, h, w, _stream()), "predict_u8")
    return out


def tta_buffer(B: int, K: int, h: int, w: int, device, cp: Optional[int] = None) -> torch.Tensor:
    """The accumulator of test-time augmentation for B windows of h x w pixels and K classes: f32 [B, h, w, cp],
    pixel-major at the logits' channel pitch ``cp`` (default pad_channels(K), the pitch of the models' logits).  K rides
    along as ``_ffa_classes``, as on the models' logits.  The contents do not matter: the first view is accumulated
    with ``first=True``."""
    cp = pad_channels(K) if cp is None else int(cp)
    if min(int(B), int(K), int(h), int(w)) < 1:
        raise ValueError(f"tta_buffer: B, K, h, w must be >= 1, got {(B, K, h, w)}")
    if cp % 8 or cp < K:
        raise ValueError(f"tta_buffer: pitch {cp} must be a multiple of 8 and hold {K} classes")
    acc = torch.empty((int(B), int(h), int(w), cp), dtype=torch.float32, device=device)
    acc._ffa_classes = int(K)
    return acc


def _chk_tta_acc(acc: torch.Tensor, num_classes: Optional[int], op: str) -> int:
    """the class count of an accumulator: ``num_classes`` when given, else what tta_buffer noted on it"""
    if not (torch.is_tensor(acc) and acc.is_cuda and acc.dtype == torch.float32 and acc.dim() == 4
            and acc.is_contiguous()):
        raise ValueError(f"{op}: the accumulator must be a contiguous f32 CUDA tensor [B, h, w, cp] (ops.tta_buffer)")
    noted = getattr(acc, "_ffa_classes", None)
    k = noted if num_classes is None else num_classes
    if k is None:
        raise ValueError(f"{op}: the accumulator does not come from ops.tta_buffer: num_classes is required")
    if noted is not None and k != noted:
        raise ValueError(f"{op}: {k} classes, but the accumulator was made for {noted}")
    if acc.shape[3] % 8 or isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= acc.shape[3]:
        raise ValueError(f"{op}: pitch {acc.shape[3]} must be a multiple of 8 and hold {k!r} classes")
    return k


def tta_accumulate_(acc: torch.Tensor, logits_nhwc: torch.Tensor, num_classes: int, code: int,
                    crop: Optional[Tuple[int, int, int, int]] = None, first: bool = False) -> torch.Tensor:
    """One view of test-time augmentation into the accumulator, in place: ``logits_nhwc`` [B, n, n, cp] (bf16 / f32) are
    the logits of the tile transformed by the forward ``code`` (flairhip.augment, 0..15), in the view's frame; their
    softmax, taken back to the tile's frame, is stored into (``first``) or added to ``acc`` [B, h, w, cp] over the crop
    window (y0, x0, h, w) of the tile's frame (default: the whole tile).  Views add up in call order, deterministically
    (flairhip.augment.tta_mean_probabilities is the definition)."""
    lib = _l.load()
    _chk_nhwc(logits_nhwc, "tta_accumulate_ logits")
    _chk_tta_acc(acc, num_classes, "tta_accumulate_")
    B, H, W, cp = logits_nhwc.shape
    if H != W:
        raise ValueError(f"tta_accumulate_: rotations need square tiles, got {H} x {W}")
    if isinstance(code, bool) or not isinstance(code, int) or not 0 <= code <= 15:
        raise ValueError(f"tta_accumulate_: code must be an int in 0..15, got {code!r}")
    y0, x0, h, w = crop if crop is not None else (0, 0, H, W)
    if not (y0 >= 0 and x0 >= 0 and h > 0 and w > 0 and y0 + h <= H and x0 + w <= W):
        raise ValueError(f"tta_accumulate_: crop {(y0, x0, h, w)} outside the {H} x {W} tile")
    if tuple(acc.shape) != (B, h, w, cp) or acc.device != logits_nhwc.device:
        raise ValueError(f"tta_accumulate_: accumulator {tuple(acc.shape)} on {acc.device} does not match "
                         f"{(B, h, w, cp)} on {logits_nhwc.device}")
    _l.check(lib.ffa_tta_accumulate(_dt(logits_nhwc), logits_nhwc.data_ptr(), acc.data_ptr(), B, H, W, num_classes, cp,
                                    y0, x0, h, w, code, int(bool(first)), _stream()), "tta_accumulate_")
    return acc


def _chk_tta_views(views: int, op: str) -> int:
    if isinstance(views, bool) or not isinstance(views, int) or views < 1:
        raise ValueError(f"{op}: views must be an int >= 1, got {views!r}")
    return views


def tta_predict_u8(acc: torch.Tensor, mode: str, views: int, num_classes: Optional[int] = None) -> torch.Tensor:
    """predict_u8's outputs from an accumulator of ``views`` views (on acc / views): 'argmax' -> [B, h, w], 'class_prob'
    -> [B, K, h, w], 'argmax_conf' -> [B, 2, h, w].  ``num_classes``: K, for an accumulator that is not tta_buffer's.
    With one identity view the outputs equal predict_u8's bit for bit."""
    lib = _l.load()
    if mode not in _PREDICT_MODES:
        raise ValueError(f"Unknown output type: {mode}")
    _chk_tta_views(views, "tta_predict_u8")
    k = _chk_tta_acc(acc, num_classes, "tta_predict_u8")
    B, h, w, cp = acc.shape
    shape = {"argmax": (B, h, w), "class_prob": (B, k, h, w), "argmax_conf": (B, 2, h, w)}[mode]
    out = torch.empty(shape, dtype=torch.uint8, device=acc.device)
    _l.check(lib.ffa_tta_predict_u8(_PREDICT_MODES[mode], acc.data_ptr(), out.data_ptr(), B, k, cp, h, w, views,
                                    _stream()), "tta_predict_u8")
    return out


def tta_probabilities(acc: torch.Tensor, views: int, num_classes: Optional[int] = None) -> torch.Tensor:
    """the mean class probabilities of an accumulator of ``views`` views: f32 [B, K, h, w]"""
    lib = _l.load()
    _chk_tta_views(views, "tta_probabilities")
    k = _chk_tta_acc(acc, num_classes, "tta_probabilities")
    B, h, w, cp = acc.shape
    out = torch.empty((B, k, h, w), dtype=torch.float32, device=acc.device)
    _l.check(lib.ffa_tta_probabilities(acc.data_ptr(), out.data_ptr(), B, k, cp, h, w, views, _stream()),
             "tta_probabilities")
    return out


def onehot_to_index(onehot: torch.Tensor) -> torch.Tensor:
    lib = _l.load()
    if onehot.dtype != torch.float32 or not onehot.is_contiguous():
        onehot = onehot.float().contiguous()
    B, K, H, W = onehot.shape
    out = torch.empty((B, H, W), dtype=torch.uint8, device=onehot.device)
    _l.check(lib.ffa_onehot_to_index(onehot.data_ptr(), out.data_ptr(), B, K, H, W, _stream()), "onehot_to_index")
    return out


def confusion_matrix_update(counts: torch.Tensor, pred: torch.Tensor, target: torch.Tensor) -> None:
    """counts[target, pred] += 1 for uint8 class maps (counts: int64 [K, K], updated in place, no host sync)."""
    lib = _l.load()
    if pred.dtype != torch.uint8 or target.dtype != torch.uint8 or not (pred.is_contiguous() and target.is_contiguous()):
        raise ValueError("confusion_matrix_update: pred / target must be contiguous uint8 tensors")
    if counts.dtype != torch.int64 or counts.dim() != 2 or counts.shape[0] != counts.shape[1]:
        raise ValueError("confusion_matrix_update: counts must be int64 [K, K]")
    _l.check(lib.ffa_confusion_matrix(pred.data_ptr(), target.data_ptr(), pred.numel(), counts.shape[0],
                                      counts.data_ptr(), _stream()), "confusion_matrix")


def eval_stats(logits_nhwc: torch.Tensor, targets_u8: torch.Tensor, num_classes: int,
               confmat: Optional[torch.Tensor] = None, want_pred: bool = True, want_class_nll: bool = True):
    """One pass over NHWC logits [B,H,W,Cp] and uint8 targets [B,H,W] for everything an evaluation needs.

    -> (pred uint8 like the targets or None, class_nll [K] float64 or None, class_count [K] int64 or None):
    pred = the first maximum over the K classes (softmax_ce's pred, byte for byte); class_count[k] = pixels with target
    k; class_nll[k] = the sum over those pixels of -log softmax[k], unweighted, in a fixed order (equal inputs give equal
    bytes).  ``confmat`` (int64 [K, K] on the logits' device) is updated in place: confmat[target, pred] += 1.  A target
    >= K contributes to nothing.  No host synchronisation.
    """
    lib = _l.load()
    _chk_nhwc(logits_nhwc, "logits")
    if targets_u8.dtype != torch.uint8 or not targets_u8.is_contiguous():
        raise ValueError("eval_stats: targets must be contiguous uint8 class indices")
    cp = logits_nhwc.shape[-1]
    npix = logits_nhwc.numel() // cp
    if targets_u8.numel() != npix:
        raise ValueError("eval_stats: target / logit pixel count mismatch")
    dev = logits_nhwc.device
    if targets_u8.device != dev:
        raise ValueError(f"eval_stats: targets on {targets_u8.device}, logits on {dev}")
    k = int(num_classes)
    if confmat is not None and not (confmat.dtype == torch.int64 and tuple(confmat.shape) == (k, k)
                                    and confmat.is_contiguous() and confmat.device == dev):
        raise ValueError(f"eval_stats: confmat must be a contiguous int64 [{k}, {k}] tensor on {dev}")
    pred = torch.empty(targets_u8.shape, dtype=torch.uint8, device=dev) if want_pred else None
    nll = cnt = ws = None
    if want_class_nll:
        nll = torch.empty(k, dtype=torch.float64, device=dev)
        cnt = torch.empty(k, dtype=torch.int64, device=dev)
        ws = workspace(lib.ffa_eval_stats_workspace_bytes(), dev, "eval_stats")
    _l.check(lib.ffa_eval_stats(_dt(logits_nhwc), logits_nhwc.data_ptr(), targets_u8.data_ptr(), npix, k, cp, _ptr(pred),
                                _ptr(confmat), _ptr(nll), _ptr(cnt), _ptr(ws), 0 if ws is None else ws.numel(),
                                _stream()), "eval_stats")
    return pred, nll, cnt


# --------------------------------------------------------------------------------------------------
# calibrated class thresholds (csrc/calibration.hip; the host side is flairhip.calibration)

def calib_hist(logits_nhwc: torch.Tensor, targets_u8: torch.Tensor, num_classes: int,
               hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The score histograms of NHWC logits [..., Cp] against uint8 targets: int64 [K, 2, 256] on the logits' device,
    hist[k, t == k, q_k] += 1 for every pixel with target t < K and every class k, q_k the byte predict_u8 'class_prob'
    writes for class k at the pixel.  ``hist`` is updated in place when given, else a zeroed one is made.  Integer
    counts: equal inputs give equal bytes.  No host synchronisation."""
    lib = _l.load()
    _chk_nhwc(logits_nhwc, "logits")
    if targets_u8.dtype != torch.uint8 or not targets_u8.is_contiguous():
        raise ValueError("calib_hist: targets must be contiguous uint8 class indices")
    cp = logits_nhwc.shape[-1]
    npix = logits_nhwc.numel() // cp
    dev = logits_nhwc.device
    if targets_u8.numel() != npix or targets_u8.device != dev:
        raise ValueError("calib_hist: targets and logits must hold the same pixels on one device")
    k = int(num_classes)
    if hist is None:
        hist = torch.zeros((k, 2, 256), dtype=torch.int64, device=dev)
    elif not (hist.dtype == torch.int64 and tuple(hist.shape) == (k, 2, 256) and hist.is_contiguous()
              and hist.device == dev):
        raise ValueError(f"calib_hist: hist must be a contiguous int64 [{k}, 2, 256] tensor on {dev}")
    _l.check(lib.ffa_calib_hist(_dt(logits_nhwc), logits_nhwc.data_ptr(), targets_u8.data_ptr(), npix, k, cp,
                                hist.data_ptr(), _stream()), "calib_hist")
    return hist


_THRESHOLDED_MODES = {"argmax": 0, "argmax_conf": 2}


def _chk_thresholds(thr: torch.Tensor, k: int, fallback: int, mode: str, device, op: str) -> int:
    if mode not in _THRESHOLDED_MODES:
        raise ValueError(f"{op}: thresholds apply to 'argmax' and 'argmax_conf' output, not to {mode!r}")
    if not (torch.is_tensor(thr) and thr.dtype == torch.uint8 and thr.dim() == 1 and thr.is_contiguous()
            and thr.device == device):
        raise ValueError(f"{op}: the thresholds must be a contiguous uint8 vector on {device}")
    if thr.numel() != k:
        raise ValueError(f"{op}: {thr.numel()} thresholds for {k} classes")
    if isinstance(fallback, bool) or not isinstance(fallback, int) or not 0 <= fallback <= 255:
        raise ValueError(f"{op}: fallback must be an int in 0..255, got {fallback!r}")
    return _THRESHOLDED_MODES[mode]


def predict_thresholded_u8(logits: torch.Tensor, num_classes: int, mode: str, thr: torch.Tensor, fallback: int,
                           crop: Optional[Tuple[int, int, int, int]] = None) -> torch.Tensor:
    """predict_u8's 'argmax' / 'argmax_conf' outputs under per-class thresholds ``thr`` (uint8 [K] on the device): class
    k passes where its 'class_prob' byte is >= thr[k]; the label is the passing class with the greatest logit (lowest
    index on a tie), ``fallback`` where none passes; the confidence plane holds the chosen class's byte, 0 where
    nothing passed.  All thresholds 0: predict_u8's outputs byte for byte."""
    lib = _l.load()
    _chk_nhwc(logits, "logits")
    m = _chk_thresholds(thr, int(num_classes), fallback, mode, logits.device, "predict_thresholded_u8")
    B, H, W, cp = logits.shape
    y0, x0, h, w = crop if crop is not None else (0, 0, H, W)
    out = torch.empty((B, h, w) if m == 0 else (B, 2, h, w), dtype=torch.uint8, device=logits.device)
    _l.check(lib.ffa_predict_thresholded_u8(_dt(logits), m, logits.data_ptr(), thr.data_ptr(), fallback,
                                            out.data_ptr(), B, H, W, int(num_classes), cp, y0, x0, h, w, _stream()),
             "predict_thresholded_u8")
    return out


def tta_predict_thresholded_u8(acc: torch.Tensor, mode: str, views: int, thr: torch.Tensor, fallback: int,
                               num_classes: Optional[int] = None) -> torch.Tensor:
    """predict_thresholded_u8's outputs from an accumulator of ``views`` views: the rule on acc / views, with the
    bytes of tta_predict_u8 'class_prob'.  With one identity view they equal predict_thresholded_u8's bit for bit."""
    lib = _l.load()
    _chk_tta_views(views, "tta_predict_thresholded_u8")
    k = _chk_tta_acc(acc, num_classes, "tta_predict_thresholded_u8")
    m = _chk_thresholds(thr, k, fallback, mode, acc.device, "tta_predict_thresholded_u8")
    B, h, w, cp = acc.shape
    out = torch.empty((B, h, w) if m == 0 else (B, 2, h, w), dtype=torch.uint8, device=acc.device)
    _l.check(lib.ffa_tta_predict_thresholded_u8(m, acc.data_ptr(), thr.data_ptr(), fallback, out.data_ptr(), B, k, cp,
                                                h, w, views, _stream()), "tta_predict_thresholded_u8")
    return out


# --------------------------------------------------------------------------------------------------
# host-side tile bookkeeping (no GPU involved)

def slice_grid(min_x, min_y, max_x, max_y, ref_left, ref_bottom, patch_size: int, margin: int, resolution: float):
    lib = _l.load()
    args = (float(min_x), float(min_y), float(max_x), float(max_y), float(ref_left), float(ref_bottom),
            int(patch_size), int(margin), float(resolution))
    n = lib.ffa_slice_grid(*args, None, 0)
    if n < 0:
        _l.check(int(n), "slice_grid")
    buf = (_l.Tile * max(n, 1))()
    n2 = lib.ffa_slice_grid(*args, buf, n)
    assert n2 == n
    return [buf[i] for i in range(n)]


def write_window(left, top, img_bounds, out_res, pred_h: int, pred_w: int):
    lib = _l.load()
    w = _l.Window()
    il, ib, ir, it = img_bounds
    _l.check(lib.ffa_write_window(float(left), float(top), float(il), float(ib), float(ir), float(it), float(out_res),
                                  int(pred_h), int(pred_w), C.byref(w)), "write_window")
    return w


# --------------------------------------------------------------------------------------------------
# polygonisation of a class raster (csrc/polygonize.hip, csrc/polygon_simplify.cpp)

def _chk_class_map(classes, background, op: str, contiguous: bool = False) -> None:
    if not (torch.is_tensor(classes) and classes.is_cuda and classes.dtype == torch.uint8 and classes.dim() == 2
            and (classes.is_contiguous() or not contiguous)):
        raise ValueError(f"{op}: a {'contiguous ' if contiguous else ''}CUDA uint8 [H, W] class map expected")
    if background is not None and not 0 <= int(background) <= 255:
        raise ValueError(f"{op}: background {background} is not a uint8 value")


def _chk_polygonize(classes, background, values, op: str):
    """the argument checks of both polygonisers; returns ``values`` contiguous (or None)"""
    _chk_class_map(classes, background, op)
    H, W = classes.shape
    if values is None:
        return None
    if not (values.is_cuda and values.dtype == torch.uint8 and tuple(values.shape) == (H, W)
            and values.device == classes.device):
        raise ValueError(f"{op}: values must be a CUDA uint8 [{H}, {W}] tensor on the device of classes")
    return values.contiguous()


def _polygon_outputs(P: int, R: int, V: int, dev):
    """the five output tensors for P polygons, R rings and V vertices"""
    return (torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int64, device=dev),
            torch.empty(P + 1, dtype=torch.int32, device=dev), torch.empty(R + 1, dtype=torch.int32, device=dev),
            torch.empty((V, 2), dtype=torch.int32, device=dev))


def _with_zonal_sums(out, values, zonal_sum):
    """``out``, followed when ``values`` are given by the int64 [P] sums that ``zonal_sum(values, P, sums)`` fills"""
    if values is None:
        return out
    sums = torch.empty(out[0].numel(), dtype=torch.int64, device=out[0].device)
    zonal_sum(values, sums.numel(), sums)
    return out + (sums,)


def polygonize(classes: torch.Tensor, background: Optional[int] = None, min_pixels: int = 1,
               values: Optional[torch.Tensor] = None):
    """Polygons of a device uint8 class map [H, W]: one per 4-connected component of equal class (``background``:
    that value is no class; None: every value is one), components of fewer than ``min_pixels`` pixels dropped.

    Returns device tensors (poly_class int32 [P], poly_pixels int64 [P], poly_ring_offsets int32 [P + 1],
    ring_vertex_offsets int32 [R + 1], vertices int32 [V, 2] as (col, row) pixel corners); layout and order as in
    include/flairhip.h.  The one host synchronisation is the read of the three counts between the two phases.
    With ``values`` (device uint8 [H, W]) a sixth tensor follows: int64 [P], the exact sum of ``values`` over the
    pixels of each polygon (ffa_polygonize_zonal_sum_u8); the first five are the same bytes either way."""
    lib = _l.load()
    values = _chk_polygonize(classes, background, values, "polygonize")
    H, W = classes.shape
    if 4 * H * W >= 1 << 31:
        raise ValueError(f"polygonize: a {H} x {W} raster exceeds the limit 4 * H * W < 2^31 (about 536 Mpx per call)")
    classes = classes.contiguous()
    nbytes = lib.ffa_polygonize_workspace_bytes(H, W)
    if nbytes < 0:
        _l.check(int(nbytes), "polygonize")
    dev = classes.device
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    st = _stream()
    _l.check(lib.ffa_polygonize_label(classes.data_ptr(), H, W, -1 if background is None else int(background),
                                      int(max(min_pixels, 0)), ws.data_ptr(), int(nbytes), counts.data_ptr(), st),
             "polygonize_label")
    P, R, V, _ = (int(v) for v in counts.cpu().tolist())
    out = _polygon_outputs(P, R, V, dev)
    # an empty tensor's pointer goes as NULL, which the bound-sized entry points take for "nothing to write"
    _l.check(lib.ffa_polygonize_emit(ws.data_ptr(), int(nbytes), H, W, P, R, V,
                                     *(t.data_ptr() if t.numel() else None for t in out), st), "polygonize_emit")
    return _with_zonal_sums(out, values, lambda v, n, sums: _l.check(lib.ffa_polygonize_zonal_sum_u8(
        ws.data_ptr(), int(nbytes), H, W, v.data_ptr(), n, _ptr(sums) if n else None, st), "polygonize_zonal_sum_u8"))


def _polygonize_size(nbytes: int) -> int:
    """a size function's answer, its FFA_ERR_ARG (a limit of the count-sized path) as ValueError"""
    if nbytes < 0:
        raise ValueError(_l.load().ffa_last_error().decode("utf-8", "replace"))
    return int(nbytes)


def polygonize_counted(classes: torch.Tensor, background: Optional[int] = None, min_pixels: int = 1,
                       values: Optional[torch.Tensor] = None):
    """``polygonize`` with workspaces sized by what the raster holds: same arguments, same returns, byte for byte.

    A count phase (labels, pixel counts, boundary edges E and polygons P; at most 16 bytes per pixel) is followed by
    one more host synchronisation, the read of E and P, and a trace phase whose workspace depends on E and P alone
    (about 42 bytes per edge).  Limits: H * W < 2^30 and E < 2^31 - 1, each a ValueError that names the numbers, raised
    before anything sized by E is allocated; a trace workspace beyond the device's free memory is a ValueError as
    well.  With E == 0 or P == 0 no trace is launched and the empty tensors are returned."""
    lib = _l.load()
    values = _chk_polygonize(classes, background, values, "polygonize_counted")
    H, W = classes.shape
    if H * W >= 1 << 30:
        raise ValueError(f"polygonize_counted: a {H} x {W} raster exceeds the limit H * W < 2^30 (about 1074 Mpx per "
                         "call)")
    px_bytes = _polygonize_size(lib.ffa_polygonize_count_bytes(H, W))
    classes = classes.contiguous()
    dev = classes.device
    minp = int(max(min_pixels, 0))
    ws_px = torch.empty(px_bytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    st = _stream()
    _l.check(lib.ffa_polygonize_count(classes.data_ptr(), H, W, -1 if background is None else int(background), minp,
                                      ws_px.data_ptr(), px_bytes, counts.data_ptr(), st), "polygonize_count")
    E, P = (int(v) for v in counts[:2].cpu().tolist())
    if E == 0 or P == 0:
        out = _polygon_outputs(0, 0, 0, dev)
        out[2].zero_()
        out[3].zero_()
        return _with_zonal_sums(out, values, lambda v, n, sums: None)
    if E >= (1 << 31) - 1:
        raise ValueError(f"polygonize_counted: the {H} x {W} raster has {E} boundary edges, beyond the limit "
                         "E < 2^31 - 1")
    tr_bytes = _polygonize_size(lib.ffa_polygonize_trace_bytes(E, P))
    free = torch.cuda.mem_get_info(dev)[0]
    if tr_bytes > free:
        raise ValueError(f"polygonize_counted: the trace workspace for {E} boundary edges and {P} polygons takes "
                         f"{tr_bytes} bytes, the device has {free} free")
    ws_tr = torch.empty(tr_bytes, dtype=torch.uint8, device=dev)
    _l.check(lib.ffa_polygonize_trace(classes.data_ptr(), H, W, minp, ws_px.data_ptr(), px_bytes, E, P,
                                      ws_tr.data_ptr(), tr_bytes, counts.data_ptr(), st), "polygonize_trace")
    P2, R, V, E2 = (int(v) for v in counts.cpu().tolist())
    if (P2, E2) != (P, E):
        raise _l.FlairHipError(f"polygonize_counted: the trace phase counted ({P2}, {E2}) polygons and edges, the "
                               f"count phase ({P}, {E})")
    out = _polygon_outputs(P, R, V, dev)
    _l.check(lib.ffa_polygonize_counted_emit(ws_px.data_ptr(), px_bytes, H, W, ws_tr.data_ptr(), tr_bytes, E, P, R, V,
                                             *(t.data_ptr() for t in out), st), "polygonize_counted_emit")
    return _with_zonal_sums(out, values, lambda v, n, sums: _l.check(lib.ffa_polygonize_counted_zonal_sum_u8(
        ws_px.data_ptr(), px_bytes, H, W, ws_tr.data_ptr(), tr_bytes, E, v.data_ptr(), n, sums.data_ptr(), st),
        "polygonize_counted_zonal_sum_u8"))


def polygon_simplify(xy, ring_vertex_offsets, poly_ring_offsets, tolerance: float, n_threads: int = 1):
    """Host: keep mask (numpy bool [V]) of topology-preserving Douglas-Peucker over float64 coordinates xy [V, 2] in
    the flat polygon layout of ``polygonize`` (csrc/polygon_simplify.cpp)."""
    import numpy as np
    lib = _l.load()
    xy = np.ascontiguousarray(xy, dtype=np.float64)
    rvo = np.ascontiguousarray(ring_vertex_offsets, dtype=np.int32)
    pro = np.ascontiguousarray(poly_ring_offsets, dtype=np.int32)
    keep = np.zeros(len(xy), dtype=np.uint8)
    P = len(pro) - 1
    if P > 0:
        _l.check(lib.ffa_polygon_simplify(xy.ctypes.data, rvo.ctypes.data, pro.ctypes.data, P, float(tolerance),
                                          int(n_threads), keep.ctypes.data), "polygon_simplify")
    return keep.astype(bool)


# --------------------------------------------------------------------------------------------------
# sieve filter on a class raster (csrc/sieve.hip)

def sieve_(classes: torch.Tensor, min_pixels: int, background: Optional[int] = None, max_rounds: int = 16) -> dict:
    """In place over a device uint8 class map [H, W]: 4-connected components of fewer than ``min_pixels`` pixels take
    the class of their greatest neighbour -- most pixels, at equal counts the smaller first pixel -- when that
    neighbour is greater than they are (``background``: that value is no class, never changes and is never a target;
    None: every value is a class).  The exact rule, one round of it, is ffa_sieve_round_u8's in include/flairhip.h;
    rounds repeat until one relabels nothing or ``max_rounds`` have run (a warning is logged when the cap cut the
    loop short).  The host reads four counters after each round.

    Returns {"rounds": rounds run (the last, idle one included), "relabelled_components", "relabelled_pixels": sums
    over the rounds, "remaining_small": small components in the raster as it is left -- at convergence those without
    a greater neighbour}.  ``min_pixels`` <= 1 and an empty raster launch nothing."""
    lib = _l.load()
    _chk_class_map(classes, background, "sieve_", contiguous=True)
    if int(min_pixels) < 0:
        raise ValueError(f"sieve_: min_pixels {min_pixels} is negative")
    if int(max_rounds) < 1:
        raise ValueError(f"sieve_: max_rounds {max_rounds} is below 1")
    H, W = classes.shape
    if 4 * H * W >= 1 << 31:
        raise ValueError(f"sieve_: a {H} x {W} raster exceeds the limit 4 * H * W < 2^31 (about 536 Mpx per call)")
    out = {"rounds": 0, "relabelled_components": 0, "relabelled_pixels": 0, "remaining_small": 0}
    if int(min_pixels) <= 1 or classes.numel() == 0:
        return out
    nbytes = lib.ffa_sieve_workspace_bytes(H, W)
    if nbytes < 0:
        _l.check(int(nbytes), "sieve_")
    dev = classes.device
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    bg = -1 if background is None else int(background)

    def one_round(target):
        _l.check(lib.ffa_sieve_round_u8(target.data_ptr(), H, W, bg, int(min_pixels), ws.data_ptr(), int(nbytes),
                                        counts.data_ptr(), _stream()), "sieve_round_u8")
        return [int(v) for v in counts.cpu().tolist()]

    moved = 0
    while out["rounds"] < int(max_rounds):
        small, comps, moved, _ = one_round(classes)
        out["rounds"] += 1
        out["relabelled_components"] += comps
        out["relabelled_pixels"] += moved
        out["remaining_small"] = small
        if moved == 0:
            break
    if moved:
        # The cap ended the loop: the small components of the raster as it is now are what one more round counts at
        # its start.  The ABI has the one entry point, so that is a whole round (vote, decide, apply) on a throw-away
        # copy: an extra H * W bytes and a round's time, paid only on this warning path, which is already the slow one.
        out["remaining_small"] = one_round(classes.clone())[0]
        logger.warning("sieve_: stopped after max_rounds = %d rounds while the last one still relabelled %d pixels; "
                       "%d small components remain", int(max_rounds), moved, out["remaining_small"])
    return out


# --------------------------------------------------------------------------------------------------
# region overlaps of two class rasters (csrc/region_overlap.hip)

@dataclass
class RegionOverlaps:
    """The region tables of two class maps and their overlap list (include/flairhip_objects.h), device tensors:
    ``a_first`` int32 / ``a_class`` int32 / ``a_pixels`` int64 [Pa] and the same for b, in ascending label order;
    ``pair_a`` int32 / ``pair_b`` int32 / ``pair_pixels`` int64 [n_pairs], sorted by (pair_a, pair_b).  ``pair_bound`` is
    the head count Q that sized the pair table (n_pairs <= Q)."""
    a_first: torch.Tensor
    a_class: torch.Tensor
    a_pixels: torch.Tensor
    b_first: torch.Tensor
    b_class: torch.Tensor
    b_pixels: torch.Tensor
    pair_a: torch.Tensor
    pair_b: torch.Tensor
    pair_pixels: torch.Tensor
    pair_bound: int = 0


def _chk_overlap_maps(a, b, dims: int, op: str) -> None:
    shape = "[B, H, W]" if dims == 3 else "[H, W]"
    for t in (a, b):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == dims):
            raise ValueError(f"{op}: CUDA uint8 {shape} class maps expected")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"{op}: the two class maps must have one shape and one device, got {tuple(a.shape)} on "
                         f"{a.device} and {tuple(b.shape)} on {b.device}")
    if a.numel() == 0:
        raise ValueError(f"{op}: empty class maps {tuple(a.shape)}")


def _overlap_backgrounds(background_a, background_b, op: str):
    for bg in (background_a, background_b):
        if bg is not None and not 0 <= int(bg) <= 255:
            raise ValueError(f"{op}: background {bg} is not a uint8 value")
    return tuple(-1 if bg is None else int(bg) for bg in (background_a, background_b))


def _region_overlaps(a: torch.Tensor, b: torch.Tensor, bgs, minps, op: str):
    """[B, H, W] maps -> list of B RegionOverlaps: the count phases back to back, one read of all counts, the pair
    phases back to back, one read of all pair counts"""
    lib = _l.load()
    B, H, W = a.shape
    if H * W >= 1 << 30:
        raise ValueError(f"{op}: a {H} x {W} raster exceeds the limit H * W < 2^30 (about 1074 Mpx per call)")
    a, b = a.contiguous(), b.contiguous()
    dev = a.device
    nbytes = _polygonize_size(lib.ffa_region_overlap_bytes(H, W))
    st = _stream()
    counts = torch.empty((B, 4), dtype=torch.int64, device=dev)
    wss = [torch.empty(nbytes, dtype=torch.uint8, device=dev) for _ in range(B)]
    for i in range(B):
        _l.check(lib.ffa_region_overlap_count(a[i].data_ptr(), b[i].data_ptr(), H, W, bgs[0], bgs[1], minps[0], minps[1],
                                              wss[i].data_ptr(), nbytes, counts[i].data_ptr(), st),
                 "region_overlap_count")
    sizes = counts.cpu().tolist()
    outs = []
    for i, (Pa, Pb, Q, _) in enumerate(sizes):
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)  # noqa: E731
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)  # noqa: E731
        out = [i32(Pa), i32(Pa), i64(Pa), i32(Pb), i32(Pb), i64(Pb), i32(Q), i32(Q), i64(Q)]
        tbytes = _polygonize_size(lib.ffa_region_overlap_table_bytes(Q))
        table = torch.empty(tbytes, dtype=torch.uint8, device=dev) if Pa and Pb and Q else None
        # an empty tensor's pointer goes as NULL, which the entry point takes for "nothing to write"
        _l.check(lib.ffa_region_overlap_pairs(wss[i].data_ptr(), nbytes, H, W, Pa, Pb, Q, _ptr(table), tbytes,
                                              *(t.data_ptr() if t.numel() else None for t in out),
                                              counts[i].data_ptr(), st), "region_overlap_pairs")
        outs.append(out)
    done = counts.cpu().tolist()
    res = []
    for (Pa, Pb, Q, _), (_, _, overflow, n_pairs), out in zip(sizes, done, outs):
        if overflow or n_pairs > Q:
            raise _l.FlairHipError(f"{op}: the pair table overflowed ({n_pairs} pairs, bound {Q}, flag {overflow})")
        pa, pb, pn = (t[:n_pairs] for t in out[6:])
        order = torch.sort(pa.to(torch.int64) * max(Pb, 1) + pb.to(torch.int64)).indices
        res.append(RegionOverlaps(*out[:6], pa[order], pb[order], pn[order], int(Q)))
    return res


def region_overlaps(a: torch.Tensor, b: torch.Tensor, background_a: Optional[int] = None,
                    background_b: Optional[int] = None, min_pixels_a: int = 1, min_pixels_b: int = 1) -> RegionOverlaps:
    """The regions of two device uint8 class maps [H, W] on one grid and the pairs of them that share pixels.

    A region is a 4-connected component of equal value (``background_*``: that value is no region; None: every value
    is a class) with at least ``min_pixels_*`` pixels: the polygoniser's meaning, and the class-sorted region table is
    ``polygonize``'s polygon order (include/flairhip_objects.h).  Returns ``RegionOverlaps``: both region tables and
    the triples (index in a, index in b, shared pixels), sorted by (index in a, index in b) -- the C ABI leaves their
    order open; after this sort equal inputs give equal bytes.  Two host synchronisations: the read of the counts
    between the two phases and the read of the number of pairs."""
    _chk_overlap_maps(a, b, 2, "region_overlaps")
    bgs = _overlap_backgrounds(background_a, background_b, "region_overlaps")
    return _region_overlaps(a[None], b[None], bgs, (int(min_pixels_a), int(min_pixels_b)), "region_overlaps")[0]


def region_overlaps_batch(a: torch.Tensor, b: torch.Tensor, background_a: Optional[int] = None,
                          background_b: Optional[int] = None, min_pixels_a: int = 1, min_pixels_b: int = 1):
    """``region_overlaps`` over [B, H, W] maps: a list of B ``RegionOverlaps``, image by image (no region crosses an
    image).  The B count phases are launched back to back, all counts read once, then the B pair phases and one more
    read: two host synchronisations per batch, not per image."""
    _chk_overlap_maps(a, b, 3, "region_overlaps_batch")
    bgs = _overlap_backgrounds(background_a, background_b, "region_overlaps_batch")
    return _region_overlaps(a, b, bgs, (int(min_pixels_a), int(min_pixels_b)), "region_overlaps_batch")


# --------------------------------------------------------------------------------------------------
# geozone clipping on the pixel grid (csrc/zone_mask.hip)

ZONE_WORKSPACE_SLOT = "zone_mask"


def rasterize_zone(rings_pix, ring_offsets, H: int, W: int, out: Optional[torch.Tensor] = None,
                   accumulate: bool = False) -> torch.Tensor:
    """Inside mask (device uint8 [H, W], 0 / 1) of polygon rings given in pixel coordinates: float64 [V, 2] pairs
    (px, py), ring k = vertices ring_offsets[k] .. ring_offsets[k + 1] - 1.  A pixel is inside when its centre is,
    even-odd over all rings of the call (holes are further rings); the exact rule is in include/flairhip.h.  With
    ``accumulate`` the result is ORed into ``out`` (union of several polygons, one call each); otherwise ``out`` is
    overwritten, or allocated on the current device when None."""
    import numpy as np
    lib = _l.load()
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"rasterize_zone: raster {H} x {W} outside 1 <= H, W")
    xy = rings_pix.detach().cpu().numpy() if torch.is_tensor(rings_pix) else np.asarray(rings_pix)
    xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
    ro = ring_offsets.detach().cpu().numpy() if torch.is_tensor(ring_offsets) else np.asarray(ring_offsets)
    ro = np.ascontiguousarray(ro, dtype=np.int64).reshape(-1)
    if len(ro) < 1 or ro[0] != 0 or ro[-1] != len(xy) or np.any(np.diff(ro) < 0):
        raise ValueError(f"rasterize_zone: ring_offsets must rise from 0 to the vertex count {len(xy)}, got {ro.tolist()}")
    if not np.all(np.isfinite(xy)):
        raise ValueError("rasterize_zone: non-finite ring coordinate")
    if accumulate and out is None:
        raise ValueError("rasterize_zone: accumulate needs the mask to accumulate into (out=)")
    if out is None:
        out = torch.empty((H, W), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    elif not (out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (H, W) and out.is_contiguous()):
        raise ValueError(f"rasterize_zone: out must be a contiguous CUDA uint8 [{H}, {W}] tensor")
    dev = out.device
    n_rings = len(ro) - 1
    nbytes = lib.ffa_zone_mask_workspace_bytes(H, W, len(xy))
    if nbytes < 0:
        _l.check(int(nbytes), "rasterize_zone")
    ws = workspace(int(nbytes), dev, ZONE_WORKSPACE_SLOT)
    xy_d = torch.from_numpy(xy).to(dev) if len(xy) else None
    ro_d = torch.from_numpy(ro.astype(np.int32)).to(dev)
    _l.check(lib.ffa_zone_mask_u8(_ptr(xy_d), ro_d.data_ptr(), n_rings if len(xy) else 0, H, W, out.data_ptr(),
                                  1 if accumulate else 0, ws.data_ptr(), int(ws.numel()), _stream()), "zone_mask_u8")
    return out


def zone_clip_(classes: torch.Tensor, mask: Optional[torch.Tensor], keep_classes=None, fill: int = 0) -> torch.Tensor:
    """In place over a device uint8 class map: pixels where ``mask`` (device uint8, same shape; None = everywhere
    inside) is 0, and pixels whose class is not in ``keep_classes`` (iterable of ints; None = all), become ``fill``."""
    lib = _l.load()
    if not (classes.is_cuda and classes.dtype == torch.uint8 and classes.is_contiguous()):
        raise ValueError("zone_clip_: a contiguous CUDA uint8 class map expected")
    if not 0 <= int(fill) <= 255:
        raise ValueError(f"zone_clip_: fill {fill} is not a uint8 value")
    if mask is not None:
        if not (mask.is_cuda and mask.dtype == torch.uint8 and mask.shape == classes.shape
                and mask.device == classes.device):
            raise ValueError(f"zone_clip_: mask must be a CUDA uint8 {tuple(classes.shape)} tensor on the device of classes")
        mask = mask.contiguous()
    lut = None
    if keep_classes is not None:
        keep = sorted({int(c) for c in keep_classes})
        if keep and not (0 <= keep[0] and keep[-1] <= 255):
            raise ValueError(f"zone_clip_: class ids must be uint8 values, got {keep}")
        table = torch.full((256,), int(fill), dtype=torch.uint8)
        if keep:
            idx = torch.tensor(keep, dtype=torch.long)
            table[idx] = idx.to(torch.uint8)
        lut = table.to(classes.device)
    _l.check(lib.ffa_zone_clip_u8(classes.data_ptr(), _ptr(mask), _ptr(lut), classes.numel(), int(fill), _stream()),
             "zone_clip_u8")
    return classes


def zone_window_counts(mask: torch.Tensor, windows) -> torch.Tensor:
    """Device int64 [N]: the number of non-zero pixels of ``mask`` (device uint8 [H, W]) in each pixel rectangle
    ``windows[n] = (r0, c0, r1, c1)`` (rows r0 .. r1 - 1, columns c0 .. c1 - 1, clamped to the raster)."""
    import numpy as np
    lib = _l.load()
    if not (mask.is_cuda and mask.dtype == torch.uint8 and mask.dim() == 2):
        raise ValueError("zone_window_counts: a CUDA uint8 [H, W] mask expected")
    mask = mask.contiguous()
    if torch.is_tensor(windows):
        win = windows.to(device=mask.device, dtype=torch.int32).reshape(-1, 4).contiguous()
    else:
        w = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
        win = torch.from_numpy(np.clip(w, -(1 << 30), 1 << 30).astype(np.int32)).to(mask.device)
    counts = torch.zeros(win.shape[0], dtype=torch.int64, device=mask.device)
    H, W = mask.shape
    _l.check(lib.ffa_zone_window_counts(mask.data_ptr(), H, W, _ptr(win) if len(win) else None, int(win.shape[0]),
                                        _ptr(counts) if len(win) else None, _stream()), "zone_window_counts")
    return counts


# --------------------------------------------------------------------------------------------------
# zonal statistics: class counts and confidence sums per zone (csrc/zone_stats.hip)

ZONE_STATS_CHUNK_WORDS = 2048   # FFA_ZONE_STATS_CHUNK_WORDS: plane words per tabulation chunk (a wave each)
ZONE_STATS_NARROW_WORDS = 8     # FFA_ZONE_STATS_NARROW_WORDS: up to this many words per row the scan takes a lane per row
ZONE_STATS_WORKSPACE_SLOT = "zone_stats"
# the default plane budget of zone_class_stats: this share of the device memory that is free at the call.  A quarter
# leaves room for the rasters of the caller's next step and for the allocator's fragmentation; the planes of 10^5
# parcels on a 25 Mpx raster take 14 MB, so the budget only binds for many large overlapping zones
ZONE_STATS_MEMORY_FRACTION = 0.25


def zone_stats_flatten(zones_pix):
    """(float64 [V, 2] vertices, int32 [R + 1] ring offsets, int32 [Z + 1] ring offsets of the zones) of a list of
    zones, each a list of [n, 2] rings in pixel coordinates."""
    import numpy as np
    rings, zro = [], [0]
    for z, zone in enumerate(zones_pix):
        for ring in zone:
            r = np.asarray(ring, dtype=np.float64)
            if r.ndim != 2 or r.shape[1] != 2:
                raise ValueError(f"zone_class_stats: zone {z}: a ring must be an [n, 2] array, got shape {r.shape}")
            rings.append(r)
        zro.append(len(rings))
    xy = np.ascontiguousarray(np.concatenate(rings)) if rings else np.zeros((0, 2), dtype=np.float64)
    ro = np.concatenate([[0], np.cumsum([len(r) for r in rings], dtype=np.int64)])
    if len(xy) >= (1 << 31) - 1:
        raise ValueError(f"zone_class_stats: {len(xy)} vertices, fewer than 2^31 - 1 expected")
    return xy, ro.astype(np.int32), np.asarray(zro, dtype=np.int32)


def zone_stats_windows(xy, ring_offsets, zone_ring_offsets, H: int, W: int):
    """int32 [Z, 4] windows (r0, c0, r1, c1) by the conservative rule of include/flairhip_zonestats.h, clamped to the
    raster, c0 rounded down to a multiple of 32.  A zone without a vertex, or whose bounds miss the raster, gets an
    empty window (r1 <= r0 or c1 <= c0)."""
    import numpy as np
    ro = np.asarray(ring_offsets, dtype=np.int64)
    zv = ro[np.asarray(zone_ring_offsets, dtype=np.int64)]  # the first vertex of each zone, and V
    Z = len(zv) - 1
    win = np.zeros((Z, 4), dtype=np.int32)
    some = np.flatnonzero(np.diff(zv) > 0)
    if len(some) == 0:
        return win
    starts = zv[some]
    xmin, xmax = np.minimum.reduceat(xy[:, 0], starts), np.maximum.reduceat(xy[:, 0], starts)
    ymin, ymax = np.minimum.reduceat(xy[:, 1], starts), np.maximum.reduceat(xy[:, 1], starts)

    def clamp(v, hi):
        return np.clip(v, 0, hi).astype(np.int32)  # clipped as float64 first: far-off coordinates must not wrap

    win[some, 0] = clamp(np.floor(ymin - 0.5), H)
    win[some, 1] = clamp(np.floor(xmin - 0.5), W) & ~31
    win[some, 2] = clamp(np.ceil(ymax - 0.5) + 1, H)
    win[some, 3] = clamp(np.floor(xmax - 0.5) + 2, W)
    return win


def zone_stats_plane_words(windows):
    """(rows, words per row, plane words) of each window, int64 [Z] each; all 0 for an empty window"""
    import numpy as np
    w = np.asarray(windows, dtype=np.int64).reshape(-1, 4)
    rows = np.maximum(w[:, 2] - w[:, 0], 0)
    ww = np.where(w[:, 3] > w[:, 1], (w[:, 3] - w[:, 1] + 31) // 32, 0)
    ww = np.where(rows > 0, ww, 0)
    rows = np.where(ww > 0, rows, 0)
    return rows, ww, rows * ww


def zone_stats_plan(windows, chunk_words: int = ZONE_STATS_CHUNK_WORDS):
    """The tables ffa_zone_stats_u8 takes beside the windows: (plane_offsets int64 [Z], plane_words, scan_starts int64
    [Z + 1], chunks int32 [n, 3] = (zone, first word, words)).  The chunks cover every plane word once, none crosses
    a zone and none holds more than ``chunk_words`` words."""
    import numpy as np
    rows, ww, words = zone_stats_plane_words(windows)
    Z = len(words)
    if Z and int(words.max()) >= 1 << 31:
        raise ValueError(f"zone_class_stats: zone {int(words.argmax())} needs a plane of {int(words.max())} words, "
                         "fewer than 2^31 expected")
    ends = np.cumsum(words)
    plane_offsets = (ends - words).astype(np.int64)
    items = np.where(ww == 0, 0, np.where(ww <= ZONE_STATS_NARROW_WORDS, (rows + 63) // 64, rows))
    scan_starts = np.concatenate([[0], np.cumsum(items)]).astype(np.int64)
    per_zone = (words + chunk_words - 1) // chunk_words
    zone = np.repeat(np.arange(Z, dtype=np.int64), per_zone)
    first = (np.arange(len(zone), dtype=np.int64) - np.repeat(np.cumsum(per_zone) - per_zone, per_zone)) * chunk_words
    chunks = np.stack([zone, first, np.minimum(chunk_words, words[zone] - first)], axis=1).astype(np.int32)
    return plane_offsets, int(ends[-1]) if Z else 0, scan_starts, np.ascontiguousarray(chunks.reshape(-1, 3))


def zone_stats_batches(plane_words, max_workspace_bytes: int):
    """Consecutive zone ranges [(a, b), ...] whose planes (4 bytes a word) fit ``max_workspace_bytes`` each, as few as
    a greedy walk gives.  A zone whose own plane exceeds the budget raises ValueError naming it."""
    import numpy as np
    words = np.asarray(plane_words, dtype=np.int64)
    budget = int(max_workspace_bytes) // 4
    if len(words) and int(words.max()) > budget:
        z = int(np.flatnonzero(words > budget)[0])
        raise ValueError(f"zone_class_stats: zone {z} alone needs a plane of {4 * int(words[z])} bytes, more than "
                         f"max_workspace_bytes = {int(max_workspace_bytes)}")
    ends = np.cumsum(words)
    out, a = [], 0
    while a < len(words):
        before = int(ends[a] - words[a])
        b = max(int(np.searchsorted(ends, before + budget, side="right")), a + 1)
        out.append((a, b))
        a = b
    return out


def _zone_stats_calls(xy, ro, zro, H: int, W: int, dev, max_workspace_bytes, name: str):
    """The per-batch part shared by zone_class_stats and zone_transition_stats: windows and batches of the flattened
    zones, then per batch of zones [a, b) the planning in numpy, the workspace and the uploads.  Yields (a, b, the
    thirteen table arguments of ffa_zone_stats_u8 from xy_pix to n_chunks, the workspace tensor); the uploaded tables
    stay alive until the next batch is asked for."""
    import numpy as np
    windows = zone_stats_windows(xy, ro, zro, H, W)
    words = zone_stats_plane_words(windows)[2]
    if max_workspace_bytes is None:
        max_workspace_bytes = int(torch.cuda.mem_get_info(dev)[0] * ZONE_STATS_MEMORY_FRACTION)
    batches = zone_stats_batches(words, max_workspace_bytes)
    lib = _l.load()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    for a, b in batches:
        r0, r1 = int(zro[a]), int(zro[b])
        v0, v1 = int(ro[r0]), int(ro[r1])
        plane_offsets, plane_words, scan_starts, chunks = zone_stats_plan(windows[a:b])
        nbytes = lib.ffa_zone_stats_workspace_bytes(v1 - v0, plane_words, len(chunks))
        if nbytes < 0:
            _l.check(int(nbytes), name)
        ws = workspace(int(nbytes), dev, ZONE_STATS_WORKSPACE_SLOT)
        tables = [up(xy[v0:v1]) if v1 > v0 else None, up(ro[r0:r1 + 1] - ro[r0]), up(zro[a:b + 1] - zro[a]),
                  up(windows[a:b]), up(plane_offsets), up(scan_starts), up(chunks) if len(chunks) else None]
        yield a, b, (_ptr(tables[0]), v1 - v0, tables[1].data_ptr(), r1 - r0, tables[2].data_ptr(), b - a,
                     tables[3].data_ptr(), tables[4].data_ptr(), plane_words, tables[5].data_ptr(),
                     int(scan_starts[-1]), _ptr(tables[6]), len(chunks)), ws


def zone_class_stats(cls: torch.Tensor, zones_pix, n_classes: int, conf: Optional[torch.Tensor] = None,
                     max_workspace_bytes: Optional[int] = None):
    """Per-zone class counts of a device uint8 class raster [H, W]: (counts, conf_sums), device int64 [Z, K + 1] each,
    K = ``n_classes`` in 1..256.  ``zones_pix`` is a list of zones, each a list of float64 [n, 2] rings in pixel
    coordinates (a MultiPolygon is one zone holding the rings of all its parts).  A pixel belongs to a zone when its
    centre is inside, even-odd over the zone's rings, by the rule of ``rasterize_zone``; zones may overlap.
    counts[z, k] is the number of pixels of zone z with class k, column K collects the classes >= K.  With ``conf``
    (device uint8 [H, W]) conf_sums holds the sums of its bytes over the same pixels, else it is None.

    Each zone gets a bit plane over its own window; when all planes together exceed ``max_workspace_bytes`` the zones
    are split into consecutive batches (the results are the same bytes: zones are independent).  The default budget is
    ZONE_STATS_MEMORY_FRACTION of the free device memory.  A single zone beyond the budget raises ValueError."""
    import numpy as np
    K = int(n_classes)
    if not 1 <= K <= 256:
        raise ValueError(f"zone_class_stats: n_classes {n_classes} outside 1..256")
    if not (torch.is_tensor(cls) and cls.is_cuda and cls.dtype == torch.uint8 and cls.dim() == 2 and cls.numel() > 0):
        raise ValueError("zone_class_stats: a CUDA uint8 [H, W] class raster expected")
    if conf is not None and not (torch.is_tensor(conf) and conf.is_cuda and conf.dtype == torch.uint8
                                 and conf.shape == cls.shape and conf.device == cls.device):
        raise ValueError(f"zone_class_stats: conf must be a CUDA uint8 {tuple(cls.shape)} tensor on the device of cls")
    H, W = (int(v) for v in cls.shape)
    dev = cls.device
    xy, ro, zro = zone_stats_flatten(zones_pix)
    if not np.all(np.isfinite(xy)):
        raise ValueError("zone_class_stats: non-finite ring coordinate")
    Z = len(zro) - 1
    counts = torch.empty((Z, K + 1), dtype=torch.int64, device=dev)
    sums = torch.empty((Z, K + 1), dtype=torch.int64, device=dev) if conf is not None else None
    if Z == 0:
        return counts, sums
    lib = _l.load()
    cls = cls.contiguous()
    conf = conf.contiguous() if conf is not None else None
    for a, b, tables, ws in _zone_stats_calls(xy, ro, zro, H, W, dev, max_workspace_bytes, "zone_class_stats"):
        _l.check(lib.ffa_zone_stats_u8(cls.data_ptr(), _ptr(conf), H, W, K, *tables, counts[a:b].data_ptr(),
                                       _ptr(sums[a:b]) if sums is not None else None, ws.data_ptr(), int(ws.numel()),
                                       _stream()), "zone_stats_u8")
    return counts, sums


# --------------------------------------------------------------------------------------------------
# land-cover change between two class rasters on one grid: per-zone transition matrices (csrc/zone_stats.hip) and
# change codes (csrc/change.hip)

CHANGE_MAX_CLASSES = 32  # FFA_CHANGE_MAX_CLASSES: the per-wave transition tables of (K + 1)^2 entries must fit LDS


def zone_transition_stats(before: torch.Tensor, after: torch.Tensor, zones_pix, n_classes: int,
                          conf: Optional[torch.Tensor] = None, max_workspace_bytes: Optional[int] = None):
    """Per-zone class transitions between two device uint8 class rasters [H, W] on one grid: (counts, conf_sums),
    device int64 [Z, K + 1, K + 1] each, K = ``n_classes`` in 1..32.  counts[z, a, b] is the number of pixels of zone z
    with min(before, K) == a and min(after, K) == b: row and column K collect the values >= K.  With ``conf`` (device
    uint8 [H, W], the confidence of the *after* run) conf_sums holds the sums of its bytes over the same pixels, else it
    is None.  Zones, membership, batching beyond ``max_workspace_bytes`` and the workspace slot are those of
    ``zone_class_stats``; the marginals of counts are its counts for ``before`` (sum over b) and ``after`` (over a)."""
    import numpy as np
    name = "zone_transition_stats"
    K = int(n_classes)
    if not 1 <= K <= CHANGE_MAX_CLASSES:
        raise ValueError(f"{name}: n_classes {n_classes} outside 1..{CHANGE_MAX_CLASSES}")
    for what, t in (("before", before), ("after", after)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.numel() > 0):
            raise ValueError(f"{name}: {what} must be a CUDA uint8 [H, W] class raster")
    if before.shape != after.shape or before.device != after.device:
        raise ValueError(f"{name}: before is {tuple(before.shape)} on {before.device}, after {tuple(after.shape)} on "
                         f"{after.device}: one grid on one device expected")
    if conf is not None and not (torch.is_tensor(conf) and conf.is_cuda and conf.dtype == torch.uint8
                                 and conf.shape == after.shape and conf.device == after.device):
        raise ValueError(f"{name}: conf must be a CUDA uint8 {tuple(after.shape)} tensor on the device of the rasters")
    H, W = (int(v) for v in after.shape)
    dev = after.device
    xy, ro, zro = zone_stats_flatten(zones_pix)
    if not np.all(np.isfinite(xy)):
        raise ValueError(f"{name}: non-finite ring coordinate")
    Z = len(zro) - 1
    counts = torch.empty((Z, K + 1, K + 1), dtype=torch.int64, device=dev)
    sums = torch.empty((Z, K + 1, K + 1), dtype=torch.int64, device=dev) if conf is not None else None
    if Z == 0:
        return counts, sums
    lib = _l.load()
    before, after = before.contiguous(), after.contiguous()
    conf = conf.contiguous() if conf is not None else None
    for a, b, tables, ws in _zone_stats_calls(xy, ro, zro, H, W, dev, max_workspace_bytes, name):
        _l.check(lib.ffa_zone_change_u8(before.data_ptr(), after.data_ptr(), _ptr(conf), H, W, K, *tables,
                                        counts[a:b].data_ptr(), _ptr(sums[a:b]) if sums is not None else None,
                                        ws.data_ptr(), int(ws.numel()), _stream()), "zone_change_u8")
    return counts, sums


def _byte_range(t: torch.Tensor):
    return t.data_ptr(), t.data_ptr() + t.numel()


def change_codes(before: torch.Tensor, after: torch.Tensor, lut, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = lut[min(before, K), min(after, K)] element by element: ``before`` and ``after`` are device uint8 tensors of
    one shape (contiguous; views at any byte offset are fine), ``lut`` a host or device uint8 array [K + 1, K + 1] with
    K in 1..32 (change.transition_lut makes one).  ``out``: None for a new tensor, or a contiguous device uint8 tensor of
    the same shape -- ``before`` or ``after`` itself for an in-place recode; any other overlap with an input raises
    ValueError."""
    import numpy as np
    name = "change_codes"
    for what, t in (("before", before), ("after", after)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError(f"{name}: {what} must be a contiguous CUDA uint8 tensor")
    if before.shape != after.shape or before.device != after.device:
        raise ValueError(f"{name}: before is {tuple(before.shape)} on {before.device}, after {tuple(after.shape)} on "
                         f"{after.device}: one shape on one device expected")
    dev = after.device
    if torch.is_tensor(lut):
        if lut.dtype != torch.uint8:
            raise ValueError(f"{name}: lut must be uint8, got {lut.dtype}")
        d_lut = lut.to(dev).contiguous()
    else:
        h = np.asarray(lut)
        if h.dtype != np.uint8:
            raise ValueError(f"{name}: lut must be uint8, got {h.dtype}")
        d_lut = torch.from_numpy(np.ascontiguousarray(h)).to(dev)
    if d_lut.dim() != 2 or d_lut.shape[0] != d_lut.shape[1]:
        raise ValueError(f"{name}: lut must be [K + 1, K + 1], got {tuple(d_lut.shape)}")
    K = int(d_lut.shape[0]) - 1
    if not 1 <= K <= CHANGE_MAX_CLASSES:
        raise ValueError(f"{name}: a lut of {K + 1} x {K + 1} means n_classes {K}, outside 1..{CHANGE_MAX_CLASSES}")
    if out is None:
        out = torch.empty_like(after)
    else:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and out.shape == after.shape and out.device == dev):
            raise ValueError(f"{name}: out must be a contiguous CUDA uint8 {tuple(after.shape)} tensor on {dev}")
        o0, o1 = _byte_range(out)
        for what, t in (("before", before), ("after", after)):
            t0, t1 = _byte_range(t)
            if o0 < t1 and t0 < o1 and o0 != t0:  # the same bytes are fine: a lane reads its bytes before it writes them
                raise ValueError(f"{name}: out overlaps {what} without being it")
    n = int(after.numel())
    if n:
        _l.check(_l.load().ffa_change_code_u8(before.data_ptr(), after.data_ptr(), n, K, d_lut.data_ptr(),
                                              out.data_ptr(), _stream()), "change_code_u8")
    return out


# --------------------------------------------------------------------------------------------------
# overview pyramid of a uint8 raster (csrc/overview.hip)

OVERVIEW_METHODS = {"nearest": 0, "mode": 1, "average": 2}


def overview_levels(H: int, W: int, block: int = 512) -> int:
    """Number of overviews of an H x W raster: the smallest L with max(ceil(H / 2^L), ceil(W / 2^L)) <= block."""
    if int(H) < 1 or int(W) < 1 or int(block) < 1:
        raise ValueError(f"overview_levels: raster {H} x {W}, block {block} outside 1 <= H, W, block")
    return int(_l.load().ffa_overview_levels(int(H), int(W), int(block)))


def overview_pyramid(base: torch.Tensor, block: int = 512, method: str = "nearest", ignore: Optional[int] = None):
    """Overviews of a device uint8 raster [bands, H, W]: the list of the levels 1 .. L, level l of shape
    [bands, ceil(H / 2^l), ceil(W / 2^l)], each halving the one before by ``method`` ("nearest", "mode", "average")
    over 2 x 2 blocks; L = overview_levels(H, W, block).  ``ignore`` (mode only): a value
    that does not vote.  The exact rule is ffa_overview_pyramid_u8's in include/flairhip.h.  The levels are views into
    one allocation; a raster that fits one block gives an empty list."""
    lib = _l.load()
    if not (torch.is_tensor(base) and base.is_cuda and base.dtype == torch.uint8 and base.dim() == 3
            and base.is_contiguous()):
        raise ValueError("overview_pyramid: a contiguous CUDA uint8 [bands, H, W] raster expected")
    if method not in OVERVIEW_METHODS:
        raise ValueError(f"overview_pyramid: method {method!r} is not one of {sorted(OVERVIEW_METHODS)}")
    if ignore is not None and not 0 <= int(ignore) <= 255:
        raise ValueError(f"overview_pyramid: ignore {ignore} is not a uint8 value")
    if ignore is not None and method == "average":
        raise ValueError("overview_pyramid: the average has no ignore value")
    bands, H, W = (int(v) for v in base.shape)
    if bands < 1 or H < 1 or W < 1:
        raise ValueError(f"overview_pyramid: empty raster {tuple(base.shape)}")
    if bands * H * W >= 1 << 31:
        raise ValueError(f"overview_pyramid: {bands} bands of {H} x {W} exceed the limit bands * H * W < 2^31 per call "
                         "(bands are independent: pass them one at a time)")
    L = overview_levels(H, W, block)
    if L == 0:
        return []
    nbytes = int(lib.ffa_overview_pyramid_bytes(bands, H, W, L))
    if nbytes < 0:
        _l.check(nbytes, "overview_pyramid")
    pyr = torch.empty(nbytes, dtype=torch.uint8, device=base.device)
    with torch.cuda.device(base.device):
        _l.check(lib.ffa_overview_pyramid_u8(base.data_ptr(), pyr.data_ptr(), bands, H, W, L, OVERVIEW_METHODS[method],
                                             -1 if ignore is None or method != "mode" else int(ignore), _stream()),
                 "overview_pyramid_u8")
    out, pos = [], 0
    for l in range(1, L + 1):
        h, w = -(-H // (1 << l)), -(-W // (1 << l))
        out.append(pyr[pos:pos + bands * h * w].view(bands, h, w))
        pos += bands * h * w
    return out


# --------------------------------------------------------------------------------------------------
# points between coordinate reference systems (csrc/crs_transform.hip)

def _ffa_crs(p) -> "_l.Crs":
    return _l.Crs(int(p.kind), float(p.a), float(p.inv_flattening), float(p.lon0), float(p.lat0), float(p.lat1),
                  float(p.lat2), float(p.k0), float(p.false_easting), float(p.false_northing))


def reproject_points(xy, src, dst, out=None):
    """Points xy (float64 [N, 2], x = easting or longitude, y = northing or latitude) from the CRS ``src`` to the CRS
    ``dst`` (anything flair_zonal_detection.crs.parse accepts), one pass of ffa_crs_transform_f64; the definition,
    the datum rule and the NaN rule are in include/flairhip.h.

    A contiguous CUDA tensor is transformed on its device into ``out`` (same shape, dtype and device; ``out is xy``
    transforms in place; None allocates) and a tensor is returned.  A numpy array goes to the current device, through
    the kernel and back: a new array (or ``out``, a float64 [N, 2] array) is returned.  Anything that is not
    contiguous float64 [N, 2] raises ValueError.  N == 0, or two CRSs crs.same calls equal, launch nothing: the input
    is returned (copied into ``out`` when that is given)."""
    import numpy as np
    from flair_zonal_detection import crs as _crs
    s, d = _crs.parse(src), _crs.parse(dst)
    is_tensor = torch.is_tensor(xy)
    if not is_tensor and not isinstance(xy, np.ndarray):
        raise ValueError(f"reproject_points: a torch tensor or a numpy array expected, got {type(xy).__name__}")

    def ok(t):
        contiguous = t.is_contiguous() if torch.is_tensor(t) else t.flags["C_CONTIGUOUS"]
        f64 = t.dtype == (torch.float64 if torch.is_tensor(t) else np.float64)
        return f64 and t.ndim == 2 and t.shape[1] == 2 and contiguous

    if not ok(xy):
        raise ValueError(f"reproject_points: contiguous float64 [N, 2] points expected, got {xy.dtype} "
                         f"{tuple(xy.shape)}")
    if out is not None:
        if torch.is_tensor(out) != is_tensor or not ok(out) or tuple(out.shape) != tuple(xy.shape):
            raise ValueError(f"reproject_points: out must be contiguous float64 {tuple(xy.shape)} of the kind of xy")
        if is_tensor and out.device != xy.device:
            raise ValueError("reproject_points: out must be on the device of xy")
    if is_tensor and not xy.is_cuda:
        raise ValueError("reproject_points: a CUDA tensor (or a numpy array) expected")
    if xy.shape[0] == 0 or _crs.same(s, d):
        if out is None or out is xy:
            return xy
        if is_tensor:
            out.copy_(xy)
        else:
            out[...] = xy
        return out
    lib = _l.load()
    if is_tensor:
        src_d = xy
        dst_d = torch.empty_like(xy) if out is None else out
    else:
        src_d = dst_d = torch.from_numpy(xy).to(torch.device("cuda", torch.cuda.current_device()))
    if src_d.data_ptr() % 16 or dst_d.data_ptr() % 16:
        raise ValueError("reproject_points: the points must be 16-byte aligned")
    with torch.cuda.device(src_d.device):
        _l.check(lib.ffa_crs_transform_f64(src_d.data_ptr(), dst_d.data_ptr(), int(xy.shape[0]), C.byref(_ffa_crs(s)),
                                           C.byref(_ffa_crs(d)), _stream()), "crs_transform_f64")
    if is_tensor:
        return dst_d
    res = dst_d.cpu().numpy()
    if out is None:
        return res
    out[...] = res
    return out


# --------------------------------------------------------------------------------------------------
# U-TAE Sentinel branch (flair_hub/models/multitemp_model.py): small kernels around conv2d
# The kernels index their small operands (pad flags, affine vectors, attention masks) without bounds of their own, so the
# wrappers refuse what would make them read past the end.

def _chk_pad(pad: torch.Tensor, n: int, ref: torch.Tensor, op: str) -> None:
    if not (pad.dtype == torch.uint8 and pad.is_contiguous() and pad.numel() == n and pad.device == ref.device):
        raise ValueError(f"{op}: pad must be a contiguous uint8 tensor of B * T = {n} elements on {ref.device}, got "
                         f"{pad.dtype} {tuple(pad.shape)} on {pad.device}")


def _chk_f32_vec(t: torch.Tensor, n: int, ref: torch.Tensor, op: str, name: str) -> None:
    if not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n and t.device == ref.device):
        raise ValueError(f"{op}: {name} must be contiguous f32 of {n} elements on {ref.device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")


def _chk_masks(t: Optional[torch.Tensor], shape, ref: torch.Tensor, op: str, name: str) -> None:
    if t is None:
        return
    if not (t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape) and
            t.device == ref.device):
        raise ValueError(f"{op}: {name} must be contiguous f32 [n_head, B, T, h*w] = {list(shape)} on {ref.device}, got "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")


def _chk_like(t: Optional[torch.Tensor], shape, ref: torch.Tensor, op: str, name: str) -> None:
    if t is None:
        return
    if not (t.dtype == ref.dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape) and t.device == ref.device):
        raise ValueError(f"{op}: {name} must be contiguous {ref.dtype} {list(shape)} on {ref.device}, got {t.dtype} "
                         f"{tuple(t.shape)} on {t.device}")


def _chk_group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, op: str) -> int:
    _chk_nhwc(x, f"{op} input")
    C = x.shape[-1]
    if groups <= 0 or C % groups:
        raise ValueError(f"{op}: {C} channels do not split into {groups} groups")
    _chk_f32_vec(gamma, C, x, op, "gamma")
    _chk_f32_vec(beta, C, x, op, "beta")
    return C


def _chk_ltae(k: torch.Tensor, v: torch.Tensor, Q: torch.Tensor, pad: torch.Tensor, B: int, T: int, op: str):
    _chk_nhwc(k, "ltae keys")
    _chk_nhwc(v, "ltae values")
    N, h, w, KC = k.shape
    if Q.dim() != 2:
        raise ValueError(f"{op}: Q must be [n_head, d_k], got {tuple(Q.shape)}")
    n_head, d_k = Q.shape
    _chk_f32_vec(Q, n_head * d_k, k, op, "Q")
    if N != B * T:
        raise ValueError(f"{op}: leading size {N} is not B * T = {B * T}")
    if KC != n_head * d_k or v.shape[-1] % n_head or v.shape[:3] != k.shape[:3] or v.dtype != k.dtype:
        raise ValueError(f"{op}: inconsistent shapes: keys {tuple(k.shape)} {k.dtype}, values {tuple(v.shape)} {v.dtype}, "
                         f"Q {tuple(Q.shape)} (keys need n_head * d_k channels, values a multiple of n_head)")
    _chk_pad(pad, N, k, op)
    return h, w, n_head, d_k, v.shape[-1] // n_head


def _chk_ltae_train(d_k: int, d_v: int, op: str) -> None:
    if d_k > 8 or d_v > 32:
        raise ValueError(f"{op}: d_k = {d_k}, d_v = {d_v} exceed the kernel's register arrays (d_k <= 8, d_v <= 32)")


def _chk_aggregate(x: torch.Tensor, attn: torch.Tensor, pad: torch.Tensor, B: int, T: int, op: str) -> int:
    _chk_nhwc(x, f"{op} input")
    N, H, W, C = x.shape
    if N != B * T:
        raise ValueError(f"{op}: leading size {N} is not B * T = {B * T}")
    if attn.dim() != 4:
        raise ValueError(f"{op}: attn must be [n_head, B, T, h*w], got {tuple(attn.shape)}")
    n_head = attn.shape[0]
    if C % n_head:
        raise ValueError(f"{op}: {C} channels do not split into {n_head} heads")
    _chk_masks(attn, (n_head, B, T, H * W), x, op, "attn")
    _chk_pad(pad, N, x, op)
    return n_head


def reflect_pad1(x: torch.Tensor) -> torch.Tensor:
    """[N,H,W,C] -> [N,H+2,W+2,C], reflect padding by one pixel (nn.Conv2d(padding_mode='reflect'))"""
    _chk_nhwc(x, "reflect_pad1 input")
    N, H, W, C = x.shape
    out = torch.empty((N, H + 2, W + 2, C), dtype=x.dtype, device=x.device)
    _l.check(_l.load().ffa_reflect_pad1(_dt(x), x.data_ptr(), out.data_ptr(), N, H, W, C, _stream()), "reflect_pad1")
    return out


def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, relu: bool = False,
               residual: Optional[torch.Tensor] = None, eps: float = 1e-5) -> torch.Tensor:
    """nn.GroupNorm over each image of an NHWC tensor: y = [residual +] relu?(gn(x))"""
    _chk_group_norm(x, gamma, beta, groups, "group_norm")
    _chk_like(residual, x.shape, x, "group_norm", "residual")
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    _l.check(_l.load().ffa_group_norm(_dt(x), x.data_ptr(), _ptr(residual), y.data_ptr(), gamma.data_ptr(),
                                      beta.data_ptr(), N, 1, H * W * C, 0, H * W, C, C, groups, eps, 1 if relu else 0,
                                      _stream()), "group_norm")
    return y


def group_norm_seq(x: torch.Tensor, B: int, T: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                   eps: float = 1e-5) -> torch.Tensor:
    """nn.GroupNorm over the T dates of every pixel: x is [B*T, h, w, C] (image n = b*T + t); statistics per
    (b, pixel, group) over T x C/groups values (LTAE2d.in_norm / out_norm with T = 1)"""
    _chk_group_norm(x, gamma, beta, groups, "group_norm_seq")
    N, h, w, C = x.shape
    if N != B * T:
        raise ValueError(f"group_norm_seq: leading size {N} is not B * T = {B * T}")
    y = torch.empty_like(x)
    P = h * w
    _l.check(_l.load().ffa_group_norm(_dt(x), x.data_ptr(), None, y.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      B * P, P, T * P * C, C, T, P * C, C, groups, eps, 0, _stream()), "group_norm")
    return y


def positional_encoding(pos: torch.Tensor, d: int, repeat: int, period: float = 1000.0) -> torch.Tensor:
    """pos f32 [n] -> f32 [n, d * repeat] (PositionalEncoder)"""
    pos = pos.reshape(-1).float().contiguous()
    out = torch.empty((pos.numel(), d * repeat), dtype=torch.float32, device=pos.device)
    _l.check(_l.load().ffa_positional_encoding(pos.data_ptr(), out.data_ptr(), pos.numel(), d, repeat, period,
                                               _stream()), "positional_encoding")
    return out


def add_rowvec_(x: torch.Tensor, vec: torch.Tensor) -> torch.Tensor:
    """x[n, :, :, c] += vec[n, c] in place"""
    _chk_nhwc(x, "add_rowvec input")
    N, H, W, C = x.shape
    if tuple(vec.shape) != (N, C) or vec.dtype != torch.float32 or not vec.is_contiguous():
        raise ValueError("add_rowvec: vec must be contiguous f32 [N, C]")
    _l.check(_l.load().ffa_add_rowvec(_dt(x), x.data_ptr(), vec.data_ptr(), N, H * W, C, _stream()), "add_rowvec")
    return x


def ltae_attention(k: torch.Tensor, v: torch.Tensor, Q: torch.Tensor, pad: torch.Tensor, B: int, T: int):
    """-> (out [B,h,w,n_head*d_v], attn f32 [n_head,B,T,h*w]); k / v are [B*T,h,w,n_head*d_k / n_head*d_v]"""
    h, w, n_head, d_k, d_v = _chk_ltae(k, v, Q, pad, B, T, "ltae_attention")
    out = torch.empty((B, h, w, n_head * d_v), dtype=v.dtype, device=v.device)
    attn = torch.empty((n_head, B, T, h * w), dtype=torch.float32, device=v.device)
    _l.check(_l.load().ffa_ltae_attention(_dt(v), k.data_ptr(), v.data_ptr(), Q.data_ptr(), pad.data_ptr(),
                                          out.data_ptr(), attn.data_ptr(), B, T, h * w, n_head, d_k, d_v, _stream()),
             "ltae_attention")
    return out, attn


def temporal_aggregate(x: torch.Tensor, attn: torch.Tensor, pad: torch.Tensor, B: int, T: int, use_pad: bool
                       ) -> torch.Tensor:
    """x [B*T,H,W,C], attn f32 [n_head,B,T,H*W] -> [B,H,W,C] (Temporal_Aggregator 'att_group')"""
    n_head = _chk_aggregate(x, attn, pad, B, T, "temporal_aggregate")
    N, H, W, C = x.shape
    out = torch.empty((B, H, W, C), dtype=x.dtype, device=x.device)
    _l.check(_l.load().ffa_temporal_aggregate(_dt(x), x.data_ptr(), attn.data_ptr(), pad.data_ptr(), out.data_ptr(), B,
                                              T, H * W, C, n_head, 1 if use_pad else 0, _stream()),
             "temporal_aggregate")
    return out


def detect_pad_images(x: torch.Tensor, value: float = 0.0) -> torch.Tensor:
    """x f32 [N, ...] -> u8 [N]: 1 where every element of image n equals `value`"""
    x = x.contiguous()
    N = x.shape[0]
    pad = torch.empty(N, dtype=torch.uint8, device=x.device)
    _l.check(_l.load().ffa_detect_pad_images(x.data_ptr(), pad.data_ptr(), N, x.numel() // N, value, _stream()),
             "detect_pad_images")
    return pad


def mask_images_(x: torch.Tensor, pad: torch.Tensor, value: float = 0.0) -> torch.Tensor:
    """x[n] = value in place for every image n with pad[n] != 0"""
    if not (x.is_cuda and x.dim() >= 1 and x.is_contiguous()):
        raise ValueError("mask_images: input must be a contiguous CUDA tensor [N, ...]")
    N = x.shape[0]
    _chk_pad(pad, N, x, "mask_images")
    _l.check(_l.load().ffa_mask_images(_dt(x), x.data_ptr(), pad.data_ptr(), N, x.numel() // N, value, _stream()),
             "mask_images")
    return x


# --------------------------------------------------------------------------------------------------
# Swin-Transformer / UPerNet (csrc/transformer.hip, csrc/gemm.hip)

# The kernels index gamma / beta / stats / the qkv bias / the bias table / row_scale and the gradient operands without
# bounds of their own, so the wrappers refuse what would make them read past the end (as the U-TAE block above does).

ACT_NONE, ACT_GELU, ACT_DGELU, ACT_RELU = 0, 1, 2, 3


def _chk_contig(t: torch.Tensor, op: str, name: str = "input") -> None:
    if not t.is_contiguous():
        raise ValueError(f"{op}: {name} must be contiguous")


def _chk_stats(stats: Optional[torch.Tensor], rows: int, ref: torch.Tensor, op: str) -> None:
    if stats is None:
        return
    if not (stats.dtype == torch.float32 and stats.is_contiguous() and tuple(stats.shape) == (rows, 2) and
            stats.device == ref.device):
        raise ValueError(f"{op}: stats must be contiguous f32 [{rows}, 2] on {ref.device}, got {stats.dtype} "
                         f"{tuple(stats.shape)} on {stats.device}")


def _chk_row_scale(row_scale: torch.Tensor, rows: int, rows_per_scale: int, ref: torch.Tensor, op: str) -> None:
    need = -(-rows // rows_per_scale) if rows_per_scale > 0 else -1
    if not (rows_per_scale > 0 and row_scale.dtype == torch.float32 and row_scale.is_contiguous() and
            row_scale.numel() >= need and row_scale.device == ref.device):
        raise ValueError(f"{op}: row_scale must be contiguous f32 on {ref.device} with one entry per rows_per_scale = "
                         f"{rows_per_scale} rows (at least {need} for {rows} rows), got {row_scale.dtype} "
                         f"{tuple(row_scale.shape)} on {row_scale.device}")


def _chk_window_attention(qkv: torch.Tensor, qkv_bias: torch.Tensor, table: torch.Tensor, heads: int, ws: int, op: str):
    _chk_nhwc(qkv, f"{op} input")
    B, H, W, C3 = qkv.shape
    if C3 % 3:
        raise ValueError(f"{op}: {C3} channels are not q | k | v")
    if not (table.dim() == 2 and tuple(table.shape) == ((2 * ws - 1) ** 2, heads) and table.dtype == torch.float32 and
            table.is_contiguous() and table.device == qkv.device):
        raise ValueError(f"{op}: relative position bias table must be contiguous f32 [(2ws-1)^2, heads] = "
                         f"[{(2 * ws - 1) ** 2}, {heads}] on {qkv.device}, got {table.dtype} {tuple(table.shape)} on "
                         f"{table.device}")
    _chk_f32_vec(qkv_bias, C3, qkv, op, "qkv_bias")
    return B, H, W, C3 // 3


def linear_plan(dtype: torch.dtype, M: int, K: int, N: int) -> int:
    """the kernel ``linear`` launches for [M, K] x [N, K]: 0 f32 parity kernel, 1 gemm_bf16_kernel<2> (64-token tile),
    2 gemm_bf16_kernel<4> (128-token tile), 3 gemm256_bf16_kernel.  Launches nothing."""
    return int(_l.load().ffa_linear_plan(_dtype_id(dtype), M, K, N))


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
           residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
           aux: Optional[torch.Tensor] = None, row_scale: Optional[torch.Tensor] = None,
           rows_per_scale: int = 0) -> torch.Tensor:
    """nn.Linear on the last dimension of a token tensor [..., K]: act(x w^T + bias) * row_scale + residual.
    w: [N, K] in x's dtype (nn.Linear.weight's layout), bias f32 [N].  aux ([..., N] bf16): with ACT_GELU it RECEIVES the
    pre-activation, with ACT_DGELU it supplies it (out = (x w^T) * gelu'(aux)).  row_scale f32 [M / rows_per_scale]."""
    if x.dtype not in (torch.bfloat16, torch.float32) or w.dtype != x.dtype:
        raise ValueError("linear: bf16 (MFMA token GEMM) or f32 (parity mode, plain FMA) operands of one dtype")
    if not x.is_contiguous() or not w.is_contiguous():
        raise ValueError("linear: operands must be contiguous")
    K = x.shape[-1]
    N = w.shape[0]
    if w.shape[1] != K:
        raise ValueError(f"linear: weight {tuple(w.shape)} does not match K = {K}")
    M = x.numel() // K
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=x.dtype, device=x.device)
    for name, t in (("residual", residual), ("aux", aux)):
        if t is not None and (t.shape != out.shape or not t.is_contiguous() or t.dtype != x.dtype):
            raise ValueError(f"linear: {name} must be contiguous bf16 and shaped like the output")
    if row_scale is not None:
        _chk_row_scale(row_scale, M, rows_per_scale, x, "linear")
    _l.check(_l.load().ffa_linear_ex(_dt(x), x.data_ptr(), K, w.data_ptr(), _ptr(bias), _ptr(residual), N,
                                     out.data_ptr(), N, M, K, N, act, _ptr(aux), N, _ptr(row_scale), rows_per_scale,
                                     _stream()), "linear")
    return out


def space_to_depth(x: torch.Tensor, ps: int) -> torch.Tensor:
    """[B,H,W,C] -> [B,H/ps,W/ps,ps*ps*C], channel order (dy, dx, c)"""
    _chk_nhwc(x, "space_to_depth input")
    B, H, W, C = x.shape
    if H % ps or W % ps:
        raise ValueError(f"space_to_depth: {H}x{W} is not a multiple of the patch size {ps}")
    out = torch.empty((B, H // ps, W // ps, ps * ps * C), dtype=x.dtype, device=x.device)
    _l.check(_l.load().ffa_space_to_depth(_dt(x), x.data_ptr(), out.data_ptr(), B, H // ps, W // ps, C, ps, _stream()),
             "space_to_depth")
    return out


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
               stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.LayerNorm over the last dimension; ``stats`` (f32 [rows, 2]) receives (mean, rstd) for layer_norm_bwd"""
    _chk_contig(x, "layer_norm")
    C = x.shape[-1]
    _chk_f32_vec(gamma, C, x, "layer_norm", "gamma")
    _chk_f32_vec(beta, C, x, "layer_norm", "beta")
    _chk_stats(stats, x.numel() // C, x, "layer_norm")
    out = torch.empty_like(x)
    _l.check(_l.load().ffa_layer_norm(_dt(x), x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                      _ptr(stats), x.numel() // C, C, eps, _stream()), "layer_norm")
    return out


def layer_norm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, stats: torch.Tensor,
                   dres: Optional[torch.Tensor] = None):
    """-> (dx [+ dres], dgamma f32, dbeta f32)"""
    _chk_contig(x, "layer_norm_bwd")
    C = x.shape[-1]
    rows = x.numel() // C
    _chk_like(dy, x.shape, x, "layer_norm_bwd", "dy")
    _chk_like(dres, x.shape, x, "layer_norm_bwd", "dres")
    _chk_f32_vec(gamma, C, x, "layer_norm_bwd", "gamma")
    _chk_stats(stats, rows, x, "layer_norm_bwd")
    lib = _l.load()
    dx = torch.empty_like(x)
    dg = torch.empty(C, dtype=torch.float32, device=x.device)
    db = torch.empty(C, dtype=torch.float32, device=x.device)
    nb = lib.ffa_layer_norm_bwd_workspace_bytes(rows, C)
    ws = workspace(nb, x.device, "ln_bwd")
    _l.check(lib.ffa_layer_norm_bwd(_dt(x), x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), stats.data_ptr(),
                                    _ptr(dres), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows, C, ws.data_ptr(), ws.numel(),
                                    _stream()), "layer_norm_bwd")
    return dx, dg, db


def patch_merge_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
                     stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    """PatchMerging's gather + LayerNorm(4C): [B,H,W,C] -> [B,H/2,W/2,4C]"""
    _chk_nhwc(x, "patch_merge input")
    B, H, W, C = x.shape
    if H % 2 or W % 2:
        raise ValueError(f"patch_merge_norm: odd map {H} x {W} (the padded variant is not implemented)")
    _chk_f32_vec(gamma, 4 * C, x, "patch_merge_norm", "gamma")
    _chk_f32_vec(beta, 4 * C, x, "patch_merge_norm", "beta")
    _chk_stats(stats, B * (H // 2) * (W // 2), x, "patch_merge_norm")
    out = torch.empty((B, H // 2, W // 2, 4 * C), dtype=x.dtype, device=x.device)
    _l.check(_l.load().ffa_patch_merge_norm(_dt(x), x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                                            _ptr(stats), B, H, W, C, eps, _stream()), "patch_merge_norm")
    return out


def patch_merge_norm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, stats: torch.Tensor):
    """x [B,H,W,C] (the forward's input), dy [B,H/2,W/2,4C] -> (dx [B,H,W,C], dgamma, dbeta)"""
    _chk_nhwc(x, "patch_merge_norm_bwd input")
    B, H, W, C = x.shape
    if H % 2 or W % 2:
        raise ValueError(f"patch_merge_norm_bwd: odd map {H} x {W} (the padded variant is not implemented)")
    rows = B * (H // 2) * (W // 2)
    _chk_like(dy, (B, H // 2, W // 2, 4 * C), x, "patch_merge_norm_bwd", "dy")
    _chk_f32_vec(gamma, 4 * C, x, "patch_merge_norm_bwd", "gamma")
    _chk_stats(stats, rows, x, "patch_merge_norm_bwd")
    lib = _l.load()
    dx = torch.empty_like(x)
    dg = torch.empty(4 * C, dtype=torch.float32, device=x.device)
    db = torch.empty(4 * C, dtype=torch.float32, device=x.device)
    nb = lib.ffa_layer_norm_bwd_workspace_bytes(rows, 4 * C)
    ws = workspace(nb, x.device, "ln_bwd")
    _l.check(lib.ffa_patch_merge_norm_bwd(_dt(x), x.data_ptr(), dy.data_ptr(), gamma.data_ptr(), stats.data_ptr(),
                                          dx.data_ptr(), dg.data_ptr(), db.data_ptr(), B, H, W, C, ws.data_ptr(),
                                          ws.numel(), _stream()), "patch_merge_norm_bwd")
    return dx, dg, db


def window_attention(qkv: torch.Tensor, qkv_bias: torch.Tensor, table: torch.Tensor, heads: int, ws: int, shift: int,
                     scale: float) -> torch.Tensor:
    """qkv [B,H,W,3C] -> [B,H,W,C]; table f32 [(2ws-1)^2, heads]"""
    B, H, W, C = _chk_window_attention(qkv, qkv_bias, table, heads, ws, "window_attention")
    out = torch.empty((B, H, W, C), dtype=qkv.dtype, device=qkv.device)
    _l.check(_l.load().ffa_window_attention(_dt(qkv), qkv.data_ptr(), out.data_ptr(), qkv_bias.data_ptr(),
                                            table.data_ptr(), B, H, W, C, heads, ws, shift, scale, _stream()),
             "window_attention")
    return out


def gelu(x: torch.Tensor) -> torch.Tensor:
    _chk_contig(x, "gelu")
    out = torch.empty_like(x)
    _l.check(_l.load().ffa_gelu(_dt(x), x.data_ptr(), out.data_ptr(), x.numel(), _stream()), "gelu")
    return out


def adaptive_avg_pool(x: torch.Tensor, size: int) -> torch.Tensor:
    _chk_nhwc(x, "adaptive_avg_pool input")
    B, H, W, C = x.shape
    out = torch.empty((B, size, size, C), dtype=x.dtype, device=x.device)
    _l.check(_l.load().ffa_adaptive_avg_pool(_dt(x), x.data_ptr(), out.data_ptr(), B, H, W, C, size, _stream()),
             "adaptive_avg_pool")
    return out


def bilinear_slice(x: torch.Tensor, out_hw: Tuple[int, int], out: Optional[torch.Tensor] = None, offset: int = 0,
                   addend: Optional[torch.Tensor] = None, align_corners: bool = False) -> torch.Tensor:
    """F.interpolate(x, out_hw, 'bilinear', align_corners) (+ addend) into out[..., offset:offset + C]"""
    _chk_nhwc(x, "bilinear_slice input")
    B, Hi, Wi, C = x.shape
    Ho, Wo = out_hw
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=x.dtype, device=x.device)
    if out.shape[:3] != (B, Ho, Wo) or not out.is_contiguous() or out.dtype != x.dtype:
        raise ValueError("bilinear_slice: destination does not match")
    if addend is not None and (addend.shape != (B, Ho, Wo, C) or not addend.is_contiguous()):
        raise ValueError("bilinear_slice: addend must be dense [B,Ho,Wo,C]")
    _l.check(_l.load().ffa_bilinear_slice(_dt(x), x.data_ptr(), _ptr(addend), out.data_ptr(), B, Hi, Wi, Ho, Wo, C,
                                          out.shape[-1], offset, 1 if align_corners else 0, _stream()),
             "bilinear_slice")
    return out


def window_attention_bwd(qkv: torch.Tensor, dout: torch.Tensor, qkv_bias: torch.Tensor, table: torch.Tensor, heads: int,
                         ws: int, shift: int, scale: float):
    """-> (dqkv [B,H,W,3C], dtable f32 [(2ws-1)^2, heads], dbias_pad f32 [3C]: what reaches the qkv bias through the
    padding tokens of the window grid)"""
    B, H, W, C = _chk_window_attention(qkv, qkv_bias, table, heads, ws, "window_attention_bwd")
    C3 = 3 * C
    _chk_like(dout, (B, H, W, C), qkv, "window_attention_bwd", "dout")
    lib = _l.load()
    dqkv = torch.empty_like(qkv)
    dtable = torch.empty_like(table)
    dbias = torch.empty(C3, dtype=torch.float32, device=qkv.device)
    wsp = workspace(lib.ffa_window_attention_bwd_workspace_bytes(B, H, W, C, heads, ws), qkv.device, "attn_bwd")
    _l.check(lib.ffa_window_attention_bwd(_dt(qkv), qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                          qkv_bias.data_ptr(), table.data_ptr(), dtable.data_ptr(), dbias.data_ptr(), B,
                                          H, W, C, heads, ws, shift, scale, wsp.data_ptr(), wsp.numel(), _stream()),
             "window_attention_bwd")
    return dqkv, dtable, dbias


def bilinear_slice_bwd(dy: torch.Tensor, in_hw: Tuple[int, int], channels: int, offset: int = 0,
                       align_corners: bool = False) -> torch.Tensor:
    """gradient of bilinear_slice w.r.t. its input: dy [B,Ho,Wo,pitch] (slice [offset, offset+channels)) -> [B,Hi,Wi,channels]"""
    _chk_nhwc(dy, "bilinear_slice_bwd dy")
    B, Ho, Wo, P = dy.shape
    Hi, Wi = in_hw
    if channels <= 0 or offset < 0 or offset + channels > P:
        raise ValueError(f"bilinear_slice_bwd: slice [{offset}, {offset + channels}) does not fit dy's {P} channels")
    dx = torch.empty((B, Hi, Wi, channels), dtype=dy.dtype, device=dy.device)
    _l.check(_l.load().ffa_bilinear_slice_bwd(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, Hi, Wi, Ho, Wo, channels, P,
                                              offset, 1 if align_corners else 0, _stream()), "bilinear_slice_bwd")
    return dx


def adaptive_avg_pool_bwd(dy: torch.Tensor, in_hw: Tuple[int, int]) -> torch.Tensor:
    _chk_nhwc(dy, "adaptive_avg_pool_bwd dy")
    B, S, S2, C = dy.shape
    if S != S2:
        raise ValueError(f"adaptive_avg_pool_bwd: dy must be [B, S, S, C], got {tuple(dy.shape)}")
    H, W = in_hw
    dx = torch.empty((B, H, W, C), dtype=dy.dtype, device=dy.device)
    _l.check(_l.load().ffa_adaptive_avg_pool_bwd(_dt(dy), dy.data_ptr(), dx.data_ptr(), B, H, W, C, S, _stream()),
             "adaptive_avg_pool_bwd")
    return dx


def scale_rows(x: torch.Tensor, row_scale: torch.Tensor, rows_per_scale: int) -> torch.Tensor:
    _chk_contig(x, "scale_rows")
    C = x.shape[-1]
    _chk_row_scale(row_scale, x.numel() // C, rows_per_scale, x, "scale_rows")
    out = torch.empty_like(x)
    _l.check(_l.load().ffa_scale_rows(_dt(x), x.data_ptr(), out.data_ptr(), row_scale.data_ptr(), x.numel() // C, C,
                                      rows_per_scale, _stream()), "scale_rows")
    return out


def column_sums(x: torch.Tensor) -> torch.Tensor:
    """f32 [C]: sum over every row of a contiguous [..., C] tensor (nn.Linear's bias gradient)"""
    if not x.is_contiguous():
        raise ValueError("column_sums: input must be contiguous")
    C = x.shape[-1]
    rows = x.numel() // C
    lib = _l.load()
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = workspace(lib.ffa_column_sums_workspace_bytes(rows, C), x.device, "colsum")
    _l.check(lib.ffa_column_sums(_dt(x), x.data_ptr(), out.data_ptr(), rows, C, ws.data_ptr(), ws.numel(), _stream()),
             "column_sums")
    return out


def updown2x_slice(x: torch.Tensor, channels: int, x_offset: int = 0, out: Optional[torch.Tensor] = None,
                   offset: int = 0) -> torch.Tensor:
    """bilinear x2 then bilinear x1/2 (align_corners=False) of x[..., x_offset:x_offset+channels] in one pass, written to
    out[..., offset:offset+channels] (dense output when out is None); the operator is symmetric (its own backward)"""
    _chk_nhwc(x, "updown2x_slice input")
    B, H, W, P = x.shape
    if out is None:
        out = torch.empty((B, H, W, channels), dtype=x.dtype, device=x.device)
    if out.shape[:3] != (B, H, W) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("updown2x_slice: destination does not match")
    _l.check(_l.load().ffa_updown2x_slice(_dt(x), x.data_ptr(), out.data_ptr(), B, H, W, channels, P, x_offset,
                                          out.shape[-1], offset, _stream()), "updown2x_slice")
    return out


def linear_wgrad(x: torch.Tensor, dy: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                 with_bias: bool = False):
    """dW f32 [N, K] = dy^T x over all rows of the contiguous bf16 tensors x [..., K] and dy [..., N]; with_bias also
    returns db f32 [N] = column sums of dy from the same pass: (dW, db)"""
    if x.dtype not in (torch.bfloat16, torch.float32) or dy.dtype != x.dtype or not x.is_contiguous() or \
            not dy.is_contiguous():
        raise ValueError("linear_wgrad: contiguous bf16 or f32 operands of one dtype")
    K, N = x.shape[-1], dy.shape[-1]
    M = x.numel() // K
    if dy.numel() // N != M:
        raise ValueError("linear_wgrad: x and dy must have the same number of rows")
    lib = _l.load()
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=x.device)
    # accumulate adds to whatever dbias holds as well: a fresh db must start from 0
    db = (torch.zeros if accumulate else torch.empty)(N, dtype=torch.float32, device=x.device) if with_bias else None
    ws = workspace(lib.ffa_linear_wgrad_workspace_bytes(M, N, K), x.device, "lin_wgrad")
    _l.check(lib.ffa_linear_wgrad(_dt(x), x.data_ptr(), K, dy.data_ptr(), N, out.data_ptr(), _ptr(db), M, K, N,
                                  1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream()), "linear_wgrad")
    return (out, db) if with_bias else out


# --------------------------------------------------------------------------------------------------
# U-TAE training (backward kernels of csrc/temporal.hip)

def reflect_pad1_bwd(dpad: torch.Tensor) -> torch.Tensor:
    _chk_nhwc(dpad, "reflect_pad1_bwd input")
    N, Hp, Wp, C = dpad.shape
    dx = torch.empty((N, Hp - 2, Wp - 2, C), dtype=dpad.dtype, device=dpad.device)
    _l.check(_l.load().ffa_reflect_pad1_bwd(_dt(dpad), dpad.data_ptr(), dx.data_ptr(), N, Hp - 2, Wp - 2, C, _stream()),
             "reflect_pad1_bwd")
    return dx


def _group_norm_bwd(x, dy, gamma, beta, groups, relu, geom, samples, eps):
    lib = _l.load()
    C = x.shape[-1]
    dx = torch.empty_like(x)
    partial = torch.empty((samples, 2 * C), dtype=torch.float32, device=x.device)
    Q, stride_hi, stride_lo, inner, inner_stride = geom
    _l.check(lib.ffa_group_norm_bwd(_dt(x), x.data_ptr(), dy.data_ptr(), dx.data_ptr(), gamma.data_ptr(),
                                    beta.data_ptr(), partial.data_ptr(), samples, Q, stride_hi, stride_lo, inner,
                                    inner_stride, C, groups, eps, 1 if relu else 0, _stream()), "group_norm_bwd")
    sums = column_sums(partial)
    return dx, sums[:C].clone(), sums[C:].clone()


def group_norm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                   relu: bool = False, eps: float = 1e-5):
    """backward of group_norm (per image): -> (dx, dgamma, dbeta); a residual's gradient is dy itself"""
    _chk_group_norm(x, gamma, beta, groups, "group_norm_bwd")
    dy = dy.contiguous()
    _chk_like(dy, x.shape, x, "group_norm_bwd", "dy")
    N, H, W, C = x.shape
    return _group_norm_bwd(x, dy, gamma, beta, groups, relu, (1, H * W * C, 0, H * W, C), N, eps)


def group_norm_seq_bwd(x: torch.Tensor, dy: torch.Tensor, B: int, T: int, gamma: torch.Tensor, beta: torch.Tensor,
                       groups: int, eps: float = 1e-5):
    """backward of group_norm_seq (per pixel over the T dates)"""
    _chk_group_norm(x, gamma, beta, groups, "group_norm_seq_bwd")
    dy = dy.contiguous()
    _chk_like(dy, x.shape, x, "group_norm_seq_bwd", "dy")
    N, h, w, C = x.shape
    if N != B * T:
        raise ValueError(f"group_norm_seq_bwd: leading size {N} is not B * T = {B * T}")
    P = h * w
    return _group_norm_bwd(x, dy, gamma, beta, groups, False, (P, T * P * C, C, T, P * C), B * P, eps)


def ltae_attention_train(k: torch.Tensor, v: torch.Tensor, Q: torch.Tensor, pad: torch.Tensor, B: int, T: int,
                         drop: Optional[torch.Tensor] = None):
    """-> (out [B,h,w,n_head*d_v], attn f32 [n_head,B,T,h*w] after the attention dropout, prob: the clean softmax)"""
    h, w, n_head, d_k, d_v = _chk_ltae(k, v, Q, pad, B, T, "ltae_attention_train")
    _chk_ltae_train(d_k, d_v, "ltae_attention_train")
    _chk_masks(drop, (n_head, B, T, h * w), k, "ltae_attention_train", "drop")
    out = torch.empty((B, h, w, n_head * d_v), dtype=v.dtype, device=v.device)
    attn = torch.empty((n_head, B, T, h * w), dtype=torch.float32, device=v.device)
    prob = torch.empty_like(attn)
    _l.check(_l.load().ffa_ltae_attention_train(_dt(v), k.data_ptr(), v.data_ptr(), Q.data_ptr(), pad.data_ptr(),
                                                _ptr(drop), out.data_ptr(), attn.data_ptr(), prob.data_ptr(), B, T,
                                                h * w, n_head, d_k, d_v, _stream()), "ltae_attention_train")
    return out, attn, prob


def ltae_attention_bwd(k, v, Q, pad, drop, prob, dout, dattn_ext, B: int, T: int):
    """-> (dk, dv, dQ f32 [n_head, d_k])"""
    lib = _l.load()
    h, w, n_head, d_k, d_v = _chk_ltae(k, v, Q, pad, B, T, "ltae_attention_bwd")
    _chk_ltae_train(d_k, d_v, "ltae_attention_bwd")
    masks = (n_head, B, T, h * w)
    _chk_masks(drop, masks, k, "ltae_attention_bwd", "drop")
    _chk_masks(prob, masks, k, "ltae_attention_bwd", "prob")
    _chk_masks(dattn_ext, masks, k, "ltae_attention_bwd", "dattn_ext")
    _chk_like(dout, (B, h, w, n_head * d_v), v, "ltae_attention_bwd", "dout")
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    nblk = lib.ffa_ltae_attention_bwd_blocks(B, h * w, n_head)
    pitch = (n_head * d_k + 7) // 8 * 8  # the kernel pads its rows with zeros to column_sums' 8 columns
    part = torch.empty((nblk, pitch), dtype=torch.float32, device=k.device)
    _l.check(lib.ffa_ltae_attention_bwd(_dt(v), k.data_ptr(), v.data_ptr(), Q.data_ptr(), pad.data_ptr(), _ptr(drop),
                                        prob.data_ptr(), dout.data_ptr(), _ptr(dattn_ext), dk.data_ptr(), dv.data_ptr(),
                                        part.data_ptr(), B, T, h * w, n_head, d_k, d_v, _stream()), "ltae_attention_bwd")
    dq = column_sums(part)[:n_head * d_k].view(n_head, d_k)
    return dk, dv, dq


def temporal_aggregate_bwd(x: torch.Tensor, attn: torch.Tensor, pad: torch.Tensor, dout: torch.Tensor, B: int, T: int,
                           use_pad: bool):
    """-> (dx like x, dattn f32 like attn)"""
    n_head = _chk_aggregate(x, attn, pad, B, T, "temporal_aggregate_bwd")
    N, H, W, C = x.shape
    _chk_like(dout, (B, H, W, C), x, "temporal_aggregate_bwd", "dout")
    dx = torch.empty_like(x)
    dattn = torch.empty_like(attn)
    _l.check(_l.load().ffa_temporal_aggregate_bwd(_dt(x), x.data_ptr(), attn.data_ptr(), pad.data_ptr(), dout.data_ptr(),
                                                  dx.data_ptr(), dattn.data_ptr(), B, T, H * W, C, n_head,
                                                  1 if use_pad else 0, _stream()), "temporal_aggregate_bwd")
    return dx, dattn


def mean_stack(xs, divisor: Optional[float] = None) -> torch.Tensor:
    """(xs[0] + ... + xs[-1]) / divisor (default: their number) -- torch.mean(torch.stack(xs), 0) in one pass"""
    import ctypes as C
    xs = list(xs)
    if not 1 <= len(xs) <= 4:
        raise ValueError("mean_stack: 1 to 4 operands")
    x0 = xs[0]
    for x in xs:
        if x.shape != x0.shape or x.dtype != x0.dtype or not x.is_contiguous():
            raise ValueError("mean_stack: operands must be contiguous tensors of one shape and dtype")
    y = torch.empty_like(x0)
    ptrs = (C.c_void_p * len(xs))(*[x.data_ptr() for x in xs])
    _l.check(_l.load().ffa_mean_stack(_dt(x0), ptrs, len(xs), float(len(xs) if divisor is None else divisor), y.data_ptr(),
                                      x0.numel(), _stream()), "mean_stack")
    return y


def mul(x: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    if x.shape != m.shape or x.dtype != m.dtype or not x.is_contiguous() or not m.is_contiguous():
        raise ValueError("mul: operands must be contiguous tensors of one shape and dtype")
    y = torch.empty_like(x)
    _l.check(_l.load().ffa_mul(_dt(x), x.data_ptr(), m.data_ptr(), y.data_ptr(), x.numel(), _stream()), "mul")
    return y
