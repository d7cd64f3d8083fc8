"""In-situ checks of the kernels of a training step ("teacher forcing at the op level").

``Recorder`` patches the kernel-launching functions of ``flairhip.ops`` while a real training step runs.  Every
outermost call is checked as it happens: the call's own inputs (cloned before the call, so in-place updates can be
checked too) go through a float64 reference of the same operation, and the product's outputs are compared element by
element -- or, in projection mode, through seeded random projections over the channels (a Freivalds check) -- against
a bound made of the rounding of the stored output plus an f32 summation term:

    stored activations:          |o - r| <= ulp_stored(r) + REL * a    (ulp_bf16 or ulp_f32, by the output's own type)
    f32 sums (dW, statistics):   |o - r| <= REL * a

with ``a`` the same linear operation on absolute values.  The inputs are exactly what the kernel saw, so an error in
one layer does not avalanche into the next one's check.  Only summaries are kept.

The rounding unit follows the stored type (``ulp_stored``), so the fp32 programs (``hardware.precision: fp32``) are held
to 2^-16 a + ulp_f32(r): two orders of magnitude above honest f32 summation, and 128 times below what a kernel that is
f32 only in name (bf16 operands, a bf16 detour of the output) produces.  Their operands are the f32 master weights as
they are, folded in eval mode as the packer folds them (w * scale in f32, csrc/conv_pack.hip).

The eval step (zonal inference) is covered the same way: ``nn._eval_folded`` is hooked so that a conv call on an
operand with the BatchNorm scale folded in is checked against ``bf16(w * scale)`` as the packer forms it, with the
product's own scale vector -- which is itself checked, as the output of ``bn_eval_params``, against float64 -- and the
uint8 outputs (``predict_u8``, ``tta_accumulate_``, ``tta_predict_u8``, ``tta_probabilities``) against the float64
softmax of the call's own logits: labels exactly (first maximum), bands and confidence under the half-integer rule.

The U-TAE time-series branch (flairhip/utae.py on csrc/temporal.hip) is covered the same way: ``HipUTAE._packed`` is
hooked so that every operand it hands out is known with its master weight (Conv1d / Linear weights as 1x1 OIHW), the
column slice, the transpose flag and, in eval mode, the product's own checked ``bn_eval_params`` scale; the temporal ops
(GroupNorm over images and over the dates of a pixel, the L-TAE attention with its dropout mask, saved probabilities
and ``dattn_ext`` as call inputs, the temporal aggregation, reflect padding, the date encoding, column sums) have
float64 restatements of the reference's multitemp_model.py; a transposed operand is held to ``F.conv_transpose2d`` of
the master weight, whatever the product uses it for; ``dattn_ext`` must be the sum of what the aggregators sent back.

The references work on any device (CPU for tests/test_insitu_checker.py, the GPU in float64 for the step).
"""
from __future__ import annotations

import inspect
from collections import defaultdict
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

REL = 2.0 ** -16          # f32 summation term, relative to the magnitude bound a
AMBIG_REL = 2.0 ** -20    # |pre-activation| below this * (|x*s| + |t|): the ReLU mask may go either way
AMBIG_MAX_FRACTION = 1e-4
ADAM_K = 8                # roundings per quantity of the AdamW update, in units of 2^-24 (Checker.adamw counts them)
F64 = torch.float64

BCO_RING, BCO_THIN, BCO_STEM = 0x1000, 0x2000, 0x8000

# functions of flairhip.ops that launch no kernel of their own (or only packers, covered through the conv results)
HELPERS = {
    "pad_channels", "conv_out_size", "conv_stat_rows", "workspace", "upcat_supported", "pro_supported",
    "conv_is_persistent", "pack_conv_weight", "coop_barrier_failed", "slice_grid", "write_window",
    "linear_plan", "tta_buffer",
}

# uint8 bands / confidence (rint(255 p)): a value may differ from rint(255 p64) only where 255 p64 lies within HALF_OPEN
# of a half-integer, and then by 1 (tests/test_tta_gpu.py::test_views_against_float64); at most OPEN_MAX_SHARE of a
# call's values may be left open like that, which is decided on the float64 reference alone
HALF_OPEN = 1e-3
OPEN_MAX_SHARE = 0.01
BN_EVAL_ULPS = 6.0        # bn_eval_params: one add, sqrtf, an f32 divide and a multiply (HIP documents 1 and 2.5 ulp)
PREDICT_MODES = ("argmax", "class_prob", "argmax_conf")


def layout_of(pw) -> str:
    if pw.bco & BCO_STEM:
        return "stem"
    if pw.bco & BCO_THIN:
        return "thin"
    if pw.bco & BCO_RING:
        return "ring16"
    return "igemm"


# --------------------------------------------------------------------------------------------------
# rounding units

def ulp_bf16(r: torch.Tensor) -> torch.Tensor:
    """unit in the last place of a bf16 number of the magnitude of r (8 significant bits)"""
    _, e = torch.frexp(r.abs())
    u = torch.ldexp(torch.ones_like(r), (e - 8).to(torch.int32))
    return torch.clamp(torch.where(r == 0, torch.zeros_like(r), u), min=2.0 ** -133)


def ulp_f32(r: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(r.abs())
    u = torch.ldexp(torch.ones_like(r), (e - 24).to(torch.int32))
    return torch.clamp(torch.where(r == 0, torch.zeros_like(r), u), min=2.0 ** -149)


def ulp_stored(r: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """rounding unit of a value of the magnitude of r in the type the output is stored in"""
    if dtype == torch.bfloat16:
        return ulp_bf16(r)
    if dtype == torch.float32:
        return ulp_f32(r)
    raise TypeError(f"no rounding unit for outputs stored as {dtype}")


def bf16_round(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(F64)


# --------------------------------------------------------------------------------------------------
# float64 references of the linear operations (NHWC activations, OIHW weights)

def conv_gather(x: torch.Tensor, w: torch.Tensor, stride: int, pad: int, ho: int, wo: int) -> torch.Tensor:
    """forward convolution: out[b,y,x,o] = sum x[b, y*s - p + ky, x*s - p + kx, i] w[o,i,ky,kx]"""
    B, H, W, I = x.shape
    O, _, kh, kw = w.shape
    hp = max(H + 2 * pad, kh - 1 + stride * (ho - 1) + 1)
    wp = max(W + 2 * pad, kw - 1 + stride * (wo - 1) + 1)
    xp = x.new_zeros((B, hp, wp, I))
    xp[:, pad:pad + H, pad:pad + W] = x
    out = x.new_zeros((B, ho, wo, O))
    for ky in range(kh):
        for kx in range(kw):
            sl = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            out += sl @ w[:, :, ky, kx].t()
    return out


def conv_scatter(dy: torch.Tensor, w: torch.Tensor, stride: int, pad: int, hi: int, wi: int) -> torch.Tensor:
    """input gradient of conv_gather (out channels = w's input channels)"""
    B, ho, wo, O = dy.shape
    _, I, kh, kw = w.shape
    hp = max(hi + 2 * pad, kh - 1 + stride * (ho - 1) + 1)
    wp = max(wi + 2 * pad, kw - 1 + stride * (wo - 1) + 1)
    dxp = dy.new_zeros((B, hp, wp, I))
    for ky in range(kh):
        for kx in range(kw):
            dxp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] += dy @ w[:, :, ky, kx]
    return dxp[:, pad:pad + hi, pad:pad + wi]


def conv_wgrad_ref(x: torch.Tensor, dy: torch.Tensor, kh: int, kw: int, stride: int, pad: int) -> torch.Tensor:
    """dW[o,i,ky,kx] = sum dy[b,y,x,o] x[b, y*s - p + ky, x*s - p + kx, i]"""
    B, H, W, I = x.shape
    _, ho, wo, O = dy.shape
    hp = max(H + 2 * pad, kh - 1 + stride * (ho - 1) + 1)
    wp = max(W + 2 * pad, kw - 1 + stride * (wo - 1) + 1)
    xp = x.new_zeros((B, hp, wp, I))
    xp[:, pad:pad + H, pad:pad + W] = x
    d = dy.reshape(-1, O).t()
    out = x.new_zeros((O, I, kh, kw))
    for ky in range(kh):
        for kx in range(kw):
            sl = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride]
            out[:, :, ky, kx] = d @ sl.reshape(-1, I)
    return out


def up2(t: torch.Tensor) -> torch.Tensor:
    return t.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def pool2_sum(t: torch.Tensor) -> torch.Tensor:
    B, H, W, C = t.shape
    return t.reshape(B, H // 2, 2, W // 2, 2, C).sum(dim=(2, 4))


def upcat(lo, skip):
    u = up2(lo)
    return u if skip is None else torch.cat([u, skip], dim=-1)


def source_coordinate_f32(n_in: int, n_out: int, device=None) -> torch.Tensor:
    """[n_out] float64 holding f32 values: ATen's area_pixel_compute_source_index for f32 tensors, as bilinear_src of
    csrc/resample_loss.hip evaluates it -- scale = f32(n_in) / f32(n_out) rounded to f32, then
    src = max(0, fmaf(scale, dst + 0.5, -0.5)): the multiply and the subtraction are ONE fma there (one rounding), as
    GPU compilers contract ATen's expression too.  dst + 0.5 is exact in f32 and the product of two f32 numbers is
    exact in float64, so one rounding of the float64 value is that fma.  (ATen's CPU build rounds the product first:
    at 32 -> 48 two of the 48 coordinates then differ by one f32 ulp, which moves a tap weight by 2^-20 or so.)"""
    scale = (torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)).to(F64)
    dst = torch.arange(n_out, dtype=F64)
    return (scale * (dst + 0.5) - 0.5).float().clamp_min(0.0).to(F64).to(device)


def bilinear_matrix(n_in: int, n_out: int, device=None, f32_coordinate: bool = False) -> torch.Tensor:
    """[n_out, n_in] float64: the bilinear resize of one axis with align_corners=False as ATen defines it -- source
    coordinate max(0, (dst + 0.5) * n_in / n_out - 0.5) taken in float64 (f32_coordinate: in f32, as ATen and the
    kernel take it for f32 tensors, source_coordinate_f32), taps floor(src) and the next index clamped to the last one,
    weights 1 - frac and frac in float64.  The backward of the resize is the transpose of this matrix."""
    if f32_coordinate:
        src = source_coordinate_f32(n_in, n_out, device)
    else:
        dst = torch.arange(n_out, dtype=F64, device=device)
        src = ((dst + 0.5) * (float(n_in) / float(n_out)) - 0.5).clamp_min(0.0)
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0.to(F64)
    m = torch.zeros((n_out, n_in), dtype=F64, device=device)
    m.scatter_add_(1, i0.unsqueeze(1), (1.0 - l1).unsqueeze(1))
    m.scatter_add_(1, i1.unsqueeze(1), l1.unsqueeze(1))
    return m


def resize2(t: torch.Tensor, my: torch.Tensor, mx: torch.Tensor) -> torch.Tensor:
    """t [B,H,W,C] float64 -> [B, my.rows, mx.rows, C]: rows through my [Ho,H], columns through mx [Wo,W]"""
    return torch.einsum("px,boxc->bopc", mx, torch.einsum("oy,byxc->boxc", my, t))


def d4_gather(planes: torch.Tensor, code: int) -> torch.Tensor:
    """[..., n, n] -> the flipped / rotated planes of augmentation code `code` (flairhip.augment.d4_source_index)"""
    from flairhip.augment import d4_source_index
    si, sj = d4_source_index(int(code), planes.shape[-1])
    si, sj = (torch.from_numpy(v).to(planes.device) for v in (si, sj))
    return planes[..., si, sj]


def samples_f64(x: torch.Tensor) -> torch.Tensor:
    """raster samples of any accepted type (uint8 / uint16 / int16 / float32) as float64"""
    if x.dtype == torch.uint16:
        return (x.view(torch.int16).to(torch.int32) & 0xFFFF).to(F64)
    return x.to(F64)


def folded_weight(w: torch.Tensor, scale: torch.Tensor, bf16: bool) -> torch.Tensor:
    """the operand values of an eval-mode fold as the packer defines them (csrc/conv_pack.hip): w[co] * scale[co] in
    f32, then the storage rounding.  Not taken in float64: rounding the exact product once differs from the packer's
    two roundings on rare weights."""
    wf = w.float() * scale.float()[:, None, None, None]
    return bf16_round(wf) if bf16 else wf.to(F64)


def first_max(z: torch.Tensor) -> torch.Tensor:
    """index of the first maximum along the last axis, as numpy.argmax gives it (torch.argmax promises no order)"""
    K = z.shape[-1]
    idx = torch.arange(K, device=z.device).expand(z.shape)
    return torch.where(z == z.max(-1, keepdim=True).values, idx, torch.full_like(idx, K)).min(-1).values


def top_two_ties(z: torch.Tensor) -> int:
    """number of positions whose two largest values along the last axis are equal"""
    if z.shape[-1] < 2:
        return 0
    t = torch.topk(z, 2, dim=-1).values
    return int((t[..., 0] == t[..., 1]).sum().item())


def crop_window(t: torch.Tensor, crop) -> torch.Tensor:
    """[B, H, W, ...] -> the window (y0, x0, h, w) of axes 1 and 2"""
    if crop is None:
        return t
    y0, x0, h, w = (int(v) for v in crop)
    return t[:, y0:y0 + h, x0:x0 + w]


# --------------------------------------------------------------------------------------------------
# comparison

class Result(dict):
    """one checked quantity: op, module, what, shape, worst (error / bound), fail (count), n, where, block, ..."""

    @property
    def ok(self) -> bool:
        return self["fail"] == 0 and not self.get("error")

    def line(self) -> str:
        s = f"{self['op']}[{self.get('module', '')}] {self['what']} {self.get('shape')}: worst err/bound {self['worst']:.3g}"
        if self["fail"]:
            s += f", {self['fail']} of {self['n']} outside the bound, worst at {self.get('where')}, " \
                 f"worst 16x16x16 block at {self.get('block')} ({self.get('block_fail')} failing)"
        if self.get("error"):
            s += f" -- {self['error']}"
        return s


def _compare(o: torch.Tensor, r: torch.Tensor, tol: torch.Tensor, what: str, exclude: Optional[torch.Tensor] = None):
    """-> Result fields for |o - r| <= tol (elementwise, exclude: mask of elements left out)"""
    err = (o.to(F64) - r).abs()
    bad = err > tol
    if exclude is not None:
        bad = bad & ~exclude
        err = torch.where(exclude, torch.zeros_like(err), err)
    ratio = torch.where(tol > 0, err / torch.where(tol > 0, tol, torch.ones_like(tol)),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    nfail = int(bad.sum().item())
    res = {"what": what, "shape": tuple(o.shape), "n": o.numel(), "fail": nfail,
           "worst": float(ratio.max().item()) if ratio.numel() else 0.0}
    if nfail:
        flat = int(torch.argmax(torch.where(bad, ratio, torch.zeros_like(ratio))).item())
        res["where"] = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), o.shape))
        res["got"], res["want"], res["bound"] = float(o.reshape(-1)[flat]), float(r.reshape(-1)[flat]), float(tol.reshape(-1)[flat])
        if o.dim() == 4:  # (image, row, col, channel): count failures per 16 x 16 pixel x 16 channel block
            B, H, W, C = o.shape
            pb = bad.to(torch.int32)
            pb = F.pad(pb, (0, (-C) % 16, 0, (-W) % 16, 0, (-H) % 16))
            Hb, Wb, Cb = pb.shape[1] // 16, pb.shape[2] // 16, pb.shape[3] // 16
            cnt = pb.reshape(B, Hb, 16, Wb, 16, Cb, 16).sum(dim=(2, 4, 6))
            k = int(torch.argmax(cnt).item())
            b, by, bx, bc = (int(v) for v in torch.unravel_index(torch.tensor(k), cnt.shape))
            res["block"] = (b, by * 16, bx * 16, bc * 16)
            res["block_fail"] = int(cnt.reshape(-1)[k])
    return res


def _exact_zero(t: torch.Tensor, what: str):
    nz = t != 0
    res = {"what": what, "shape": tuple(t.shape), "n": t.numel(), "fail": int(nz.sum().item()), "worst": 0.0}
    if res["fail"]:
        res["worst"] = float("inf")
        flat = int(torch.argmax(nz.reshape(-1).to(torch.int8)).item())
        res["where"] = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), t.shape))
        res["got"] = float(t.reshape(-1)[flat])
    return res


def _merge(parts: List[dict], what: str):
    """combine the Result fields of chunks (batch slices) of one comparison; `where` / `block` carry the image offset"""
    out = {"what": what, "n": sum(p["n"] for p in parts), "fail": sum(p["fail"] for p in parts),
           "worst": max((p["worst"] for p in parts), default=0.0)}
    out["shape"] = parts[0]["shape"] if len(parts) == 1 else (parts[0].get("full_shape") or parts[0]["shape"])
    failing = [p for p in parts if p["fail"]]
    if failing:
        w = max(failing, key=lambda p: p["worst"])
        for k in ("where", "block", "block_fail", "got", "want", "bound"):
            if k in w:
                out[k] = w[k]
    return out


def _shift(res: dict, b0: int, full_shape) -> dict:
    res["full_shape"] = tuple(full_shape)
    for k in ("where", "block"):
        if k in res:
            res[k] = (res[k][0] + b0,) + tuple(res[k][1:])
    return res


# --------------------------------------------------------------------------------------------------
# the checker: references per op

class Checker:
    """mode "full": elementwise; "proj": conv-family outputs through random projections over the channels.
    weights: id(PackedWeight) -> dict(name, transpose, weight (f32 OIHW master at pack time)); for a column block of a
    fusion 1x1 weight: master (the whole weight), off, c instead of weight."""

    def __init__(self, mode: str = "full", chunk: int = 2, seed: int = 1234, nproj: int = 2):
        assert mode in ("full", "proj")
        self.mode, self.chunk, self.nproj = mode, chunk, nproj
        self.gen_seed = seed
        self.weights: Dict[int, dict] = {}
        self.results: List[Result] = []
        self.calls: List[dict] = []  # one summary per checked call: op, module, layout, family flags
        self.grad_sources: List[tuple] = []  # (tag, f32 tensor) outputs that autograd hands to parameters
        self.sum_sources: List[torch.Tensor] = []  # checked channel_sums outputs (a bias gradient is a prefix of one)
        self.ambiguous = [0, 0]  # ReLU mask: ambiguous elements, elements
        self.open = defaultdict(lambda: [0, 0])  # uint8 codes, per kind: values left open by the half-integer rule, values
        self.ties = defaultdict(int)  # per op: positions with an exact tie of the top two whose label was checked

    # ---- helpers -------------------------------------------------------------------------------

    def _u(self, n: int, device) -> torch.Tensor:
        g = torch.Generator().manual_seed(self.gen_seed + n)
        self.gen_seed += 1
        return torch.randn(n, self.nproj, generator=g, dtype=F64).to(device)

    def _add(self, call: dict, res: dict):
        r = Result(call)
        r.update(res)
        self.results.append(r)
        return r

    def _weight(self, pw):
        info = self.weights.get(id(pw))
        if info is None:
            raise KeyError("operand not produced by HipConv2d.packed or _fusion_slice during the recording")
        return info

    def register_operand(self, pw, weight: torch.Tensor, transpose: bool = False, stride: int = 1, padding: int = 0,
                         name: str = "?"):
        """make a hand-packed operand known (ops.pack_conv_weight called directly, as the kernel tests do): pw the
        PackedWeight, weight the f32 OIHW master it was packed from, transpose / stride / padding those of the layer.
        The entry is what HipConv2d.packed leaves under the recording; the master is copied, and the operand is held
        so that its id cannot pass to another object while the checker lives.  -> pw"""
        if weight.dtype != torch.float32 or weight.dim() != 4:
            raise ValueError(f"master weight must be f32 OIHW, got {weight.dtype} {tuple(weight.shape)}")
        O, I, kh, kw = weight.shape
        want = (I if transpose else O, kh, kw, 1 if transpose else int(stride))
        if (pw.rows_real, pw.kh, pw.kw, pw.stride) != want:
            raise ValueError(f"operand (rows, kh, kw, stride) = {(pw.rows_real, pw.kh, pw.kw, pw.stride)} was not packed "
                             f"from this weight as stated: {want}")
        self.weights[id(pw)] = {"name": name, "transpose": bool(transpose), "weight": weight.detach().clone(),
                                "stride": int(stride), "padding": int(padding), "operand": pw}
        return pw

    def _chunks(self, B: int):
        c = max(1, self.chunk)
        return [(b, min(B, b + c)) for b in range(0, B, c)]

    # ---- conv family ---------------------------------------------------------------------------

    def _check_linear(self, call, o, real_c, ref_fn, what, B, extra=None, force_full=False):
        """o [B,H,W,pitch] bf16 product output whose first real_c channels are ref_fn(b0, b1, wsel) where wsel maps the
        op's output channels (None: all, else a [real_c, k] matrix to contract them with) -> (r, a) chunk tensors.
        extra(b0, b1) -> (add, add_abs) over all real channels (bias / residual), or None"""
        parts = []
        pitch = o.shape[-1]
        if pitch > real_c:
            self._add(call, _exact_zero(o[..., real_c:], what + " pad channels"))
        full = self.mode == "full" or force_full
        if full:
            for b0, b1 in self._chunks(B):
                r, a = ref_fn(b0, b1, None)
                if extra is not None:
                    e, ea = extra(b0, b1)
                    r, a = r + e, a + ea
                oc = o[b0:b1, ..., :real_c]
                parts.append(_shift(_compare(oc, r, ulp_stored(r, o.dtype) + REL * a, what), b0, o.shape))
        else:
            u = self._u(real_c, o.device)
            for b0, b1 in self._chunks(B):
                r, a = ref_fn(b0, b1, u)
                if extra is not None:
                    e, ea = extra(b0, b1)
                    r, a = r + e @ u, a + ea @ u.abs()
                oc = o[b0:b1, ..., :real_c].to(F64)
                tol = ulp_stored(oc, o.dtype) @ u.abs() + REL * a
                parts.append(_shift(_compare(oc @ u, r, tol, what), b0, o.shape))
        return self._add(call, _merge(parts, what + ("" if full else " (projected)")))

    def conv_forward(self, call, x, w64, stride, pad, o, bias=None, residual=None, relu=False):
        """o = relu?(conv(x, w) + bias + residual): x [B,H,W,Ipitch] (bf16 values), w64 [O,I,k,k] float64 (bf16 values)"""
        O, I = w64.shape[:2]
        B, Ho, Wo = o.shape[:3]
        wa = w64.abs()

        def ref(b0, b1, u):
            xc = x[b0:b1, ..., :I].to(F64)
            if u is None:
                return conv_gather(xc, w64, stride, pad, Ho, Wo), conv_gather(xc.abs(), wa, stride, pad, Ho, Wo)
            wu = torch.einsum("oikl,oj->jikl", w64, u)
            wua = torch.einsum("oikl,oj->jikl", wa, u.abs())
            return conv_gather(xc, wu, stride, pad, Ho, Wo), conv_gather(xc.abs(), wua, stride, pad, Ho, Wo)

        extra = None
        if bias is not None or residual is not None:
            def extra(b0, b1):
                e = o.new_zeros((b1 - b0, Ho, Wo, O), dtype=F64)
                if bias is not None:
                    e = e + bias[:O].to(F64)
                ea = e.abs()
                if residual is not None:
                    rr = residual[b0:b1, ..., :O].to(F64)
                    e, ea = e + rr, ea + rr.abs()
                return e, ea
        if not relu:
            return self._check_linear(call, o, O, ref, "out", B, extra=extra)

        def ref_relu(b0, b1, u):  # not linear: always elementwise
            r, a = ref(b0, b1, None)
            if extra is not None:
                e, ea = extra(b0, b1)
                r, a = r + e, a + ea
            return r.clamp_min(0), a
        return self._check_linear(call, o, O, ref_relu, "out", B, force_full=True)

    def conv_dgrad(self, call, dy, w64, stride, pad, o, residual=None):
        """o = conv_scatter(dy, w) (+ residual): the input gradient of a conv with weight w64 [O,I,k,k]"""
        O, I = w64.shape[:2]
        B, Hi, Wi = o.shape[:3]
        wa = w64.abs()

        def ref(b0, b1, u):
            d = dy[b0:b1, ..., :O].to(F64)
            if u is None:
                return conv_scatter(d, w64, stride, pad, Hi, Wi), conv_scatter(d.abs(), wa, stride, pad, Hi, Wi)
            wu = torch.einsum("oikl,ij->ojkl", w64, u)
            wua = torch.einsum("oikl,ij->ojkl", wa, u.abs())
            return conv_scatter(d, wu, stride, pad, Hi, Wi), conv_scatter(d.abs(), wua, stride, pad, Hi, Wi)

        extra = None
        if residual is not None:
            def extra(b0, b1):
                rr = residual[b0:b1, ..., :I].to(F64)
                return rr, rr.abs()
        return self._check_linear(call, o, I, ref, "dx", B, extra=extra)

    def conv_wgrad(self, call, x, dy, kh, kw, stride, pad, o, before=None):
        """o [co, ci, kh, kw] f32 = wgrad(x[..., :ci], dy[..., :co]) (+ before when accumulating)"""
        co, ci = o.shape[:2]
        B = x.shape[0]
        if self.mode == "full":
            r = o.new_zeros(o.shape, dtype=F64)
            a = o.new_zeros(o.shape, dtype=F64)
            for b0, b1 in self._chunks(B):
                xc, dc = x[b0:b1, ..., :ci].to(F64), dy[b0:b1, ..., :co].to(F64)
                r += conv_wgrad_ref(xc, dc, kh, kw, stride, pad)
                a += conv_wgrad_ref(xc.abs(), dc.abs(), kh, kw, stride, pad)
            if before is not None:
                r, a = r + before.to(F64), a + before.to(F64).abs()
            return self._add(call, _compare(o, r, REL * a, "dW"))
        u, v = self._u(co, o.device), self._u(ci, o.device)
        rl = o.new_zeros((self.nproj, ci, kh, kw), dtype=F64)
        al = torch.zeros_like(rl)
        rr = o.new_zeros((co, self.nproj, kh, kw), dtype=F64)
        ar = torch.zeros_like(rr)
        for b0, b1 in self._chunks(B):
            xc, dc = x[b0:b1, ..., :ci].to(F64), dy[b0:b1, ..., :co].to(F64)
            rl += conv_wgrad_ref(xc, dc @ u, kh, kw, stride, pad)
            al += conv_wgrad_ref(xc.abs(), dc.abs() @ u.abs(), kh, kw, stride, pad)
            rr += conv_wgrad_ref(xc @ v, dc, kh, kw, stride, pad)
            ar += conv_wgrad_ref(xc.abs() @ v.abs(), dc.abs(), kh, kw, stride, pad)
        o64 = o.to(F64)
        if before is not None:
            b64 = before.to(F64)
            rl += torch.einsum("oikl,oj->jikl", b64, u)
            al += torch.einsum("oikl,oj->jikl", b64.abs(), u.abs())
            rr += torch.einsum("oikl,ij->ojkl", b64, v)
            ar += torch.einsum("oikl,ij->ojkl", b64.abs(), v.abs())
        self._add(call, _compare(torch.einsum("oikl,oj->jikl", o64, u), rl, REL * al, "u^T dW (projected)"))
        return self._add(call, _compare(torch.einsum("oikl,ij->ojkl", o64, v), rr, REL * ar, "dW v (projected)"))

    # ---- BatchNorm -----------------------------------------------------------------------------

    def bn_stats(self, call, y0, gamma, beta, rm0, rv0, rm1, rv1, momentum, eps, scale, shift, mean, rstd):
        """statistics of the stored conv output y0 as the finalize kernel takes them; rm0/rv0 before, rm1/rv1 after"""
        C = y0.shape[-1]
        s1 = y0.new_zeros(C, dtype=F64)
        s2 = y0.new_zeros(C, dtype=F64)
        sa = y0.new_zeros(C, dtype=F64)
        for b0, b1 in self._chunks(y0.shape[0]):
            v = y0[b0:b1].to(F64).reshape(-1, C)
            s1 += v.sum(0)
            s2 += (v * v).sum(0)
            sa += v.abs().sum(0)
        n = y0.numel() // C
        m = s1 / n
        var = (s2 / n - m * m).clamp_min(0)
        t_m = REL * sa / n + ulp_f32(m)
        t_v = REL * s2 / n
        rs = 1.0 / torch.sqrt(var + eps)
        t_rs = 0.5 * rs ** 3 * t_v + ulp_f32(rs)
        g = gamma.to(F64) if gamma is not None else torch.ones_like(m)
        bt = beta.to(F64) if beta is not None else torch.zeros_like(m)
        sc = g * rs
        t_sc = g.abs() * t_rs + ulp_f32(sc)
        sh = bt - m * sc
        t_sh = sc.abs() * t_m + m.abs() * t_sc + 2 * ulp_f32(bt.abs() + (m * sc).abs())
        self._add(call, _compare(mean, m, t_m, "mean"))
        self._add(call, _compare(rstd, rs, t_rs, "rstd"))
        self._add(call, _compare(scale, sc, t_sc, "scale"))
        self._add(call, _compare(shift, sh, t_sh, "shift"))
        if rm1 is not None:
            mo = float(momentum)
            unb = var * n / (n - 1) if n > 1 else var
            rm = (1 - mo) * rm0.to(F64) + mo * m
            rv = (1 - mo) * rv0.to(F64) + mo * unb
            self._add(call, _compare(rm1, rm, mo * t_m + 2 * ulp_f32(rm.abs() + rm0.to(F64).abs()), "running_mean"))
            self._add(call, _compare(rv1, rv, mo * t_v * n / max(n - 1, 1) + 2 * ulp_f32(rv.abs() + rv0.to(F64).abs()),
                                     "running_var"))

    def bn_apply(self, call, x, scale, shift, residual, relu, o):
        C = x.shape[-1]
        s, t = scale[:C].to(F64), shift[:C].to(F64)
        parts = []
        for b0, b1 in self._chunks(x.shape[0]):
            xc = x[b0:b1].to(F64)
            r = xc * s + t
            a = (xc * s).abs() + t.abs()
            if residual is not None:
                rr = residual[b0:b1].to(F64)
                r, a = r + rr, a + rr.abs()
            if relu:
                r = r.clamp_min(0)
            parts.append(_shift(_compare(o[b0:b1], r, ulp_stored(r, o.dtype) + REL * a, "y"), b0, o.shape))
        return self._add(call, _merge(parts, "y"))

    def bn_bwd(self, call, x, dy, y, gamma, beta, mean, rstd, relu, dx, dres, dgamma, dbeta, raw_x=False):
        """raw_x: the sums came as (sum g, sum g*x) and the finalize formed dgamma = rstd * (sum g*x - mean * sum g)
        (ffa_bn_bwd_partials): the summation term of dgamma is then stated in what was summed,
        REL * rstd * (sum |g*x| + |mean| * sum |g|), which does not shrink where the two sums cancel."""
        C = x.shape[-1]
        mode = 0 if not relu else (1 if y is not None else 2)
        n = x.numel() // C
        g64 = gamma.to(F64) if gamma is not None else x.new_ones(C, dtype=F64)
        mu, rs = mean.to(F64), rstd.to(F64)
        # the kernel's forward affine for the mask of mode 2: f32 gamma * rstd, beta - mean * scale
        sc32 = (gamma if gamma is not None else torch.ones_like(rstd)) * rstd
        sh32 = (beta if beta is not None else torch.zeros_like(mean)) - mean * sc32
        sc, sh = sc32.to(F64), sh32.to(F64)

        def masks(b0, b1):
            xc, dc = x[b0:b1].to(F64), dy[b0:b1].to(F64)
            amb = None
            if mode == 0:
                gm = dc
            elif mode == 1:
                gm = torch.where(y[b0:b1] > 0, dc, torch.zeros_like(dc))
            else:
                pre = xc * sc + sh
                gm = torch.where(pre > 0, dc, torch.zeros_like(dc))
                # where dy is 0 the mask decides nothing (the zero pad channels of a class-score layer at the logits pitch)
                amb = (pre.abs() <= AMBIG_REL * ((xc * sc).abs() + sh.abs())) & (dc != 0)
            return xc, dc, gm, amb

        sb, sg, ab, ag, xb, xg = (x.new_zeros(C, dtype=F64) for _ in range(6))
        namb = 0
        for b0, b1 in self._chunks(x.shape[0]):
            xc, dc, gm, amb = masks(b0, b1)
            xh = (xc - mu) * rs
            sb += gm.reshape(-1, C).sum(0)
            sg += (gm * xh).reshape(-1, C).sum(0)
            ab += gm.abs().reshape(-1, C).sum(0)
            ag += ((gm * xc).abs() if raw_x else (gm * xh).abs()).reshape(-1, C).sum(0)
            if amb is not None:
                namb += int(amb.sum().item())
                xb += torch.where(amb, dc.abs(), torch.zeros_like(dc)).reshape(-1, C).sum(0)
                xg += torch.where(amb, (dc * xh).abs(), torch.zeros_like(dc)).reshape(-1, C).sum(0)
        if mode == 2:
            self.ambiguous[0] += namb
            self.ambiguous[1] += x.numel()
            if namb > AMBIG_MAX_FRACTION * x.numel():
                self._add(call, {"what": "ambiguous ReLU masks", "shape": tuple(x.shape), "n": x.numel(), "fail": namb,
                                 "worst": float("inf"), "error": f"{namb} ambiguous of {x.numel()}"})
        if raw_x:
            ag = rs * (ag + mu.abs() * ab)
        t_b = REL * ab + xb + ulp_f32(sb)
        t_g = REL * ag + xg + ulp_f32(sg)
        self._add(call, dict(_compare(dbeta, sb, t_b, "dbeta"), ambiguous=namb))
        self._add(call, _compare(dgamma, sg, t_g, "dgamma"))
        self.grad_sources += [("dgamma", dgamma.detach().clone()), ("dbeta", dbeta.detach().clone())]
        kg = g64.abs() * rs
        pdx, pres = [], []
        for b0, b1 in self._chunks(x.shape[0]):
            xc, dc, gm, amb = masks(b0, b1)
            xh = (xc - mu) * rs
            r = g64 * rs * (gm - sb / n - xh * sg / n)
            a = kg * (gm.abs() + sb.abs() / n + rs * (xc.abs() + mu.abs()) * sg.abs() / n)
            tol = ulp_stored(r, dx.dtype) + REL * a + kg * (t_b / n + xh.abs() * t_g / n)
            pdx.append(_shift(_compare(dx[b0:b1], r, tol, "dx", exclude=amb), b0, dx.shape))
            if dres is not None:
                pres.append(_shift(_compare(dres[b0:b1], gm, torch.zeros_like(gm), "dres", exclude=amb), b0, dx.shape))
        self._add(call, _merge(pdx, "dx"))
        if dres is not None:
            self._add(call, _merge(pres, "dres"))

    def channel_sums(self, call, x, s, q):
        C = x.shape[-1]
        v = x.to(F64).reshape(-1, C)
        self._add(call, _compare(s, v.sum(0), REL * v.abs().sum(0), "sum"))
        self._add(call, _compare(q, (v * v).sum(0), REL * (v * v).sum(0), "sum of squares"))

    # ---- optimizer -------------------------------------------------------------------------------

    def adamw(self, call, p0, g, m0, v0, step, lr, p1, m1, v1, betas, eps, weight_decay, decoupled=True,
              maximize=False):
        """One tensor of ffa_adamw_multi (csrc/optim.hip): the update restated in float64 from the f32 p0, g, m0, v0, lr
        and step the kernel received (eps and weight_decay as the f32 values its arguments hold; the betas are doubles
        there), against the p1, m1, v1 it left, per element.

        Bounds, u = 2^-24, ADAM_K = 8 roundings at most per quantity (the kernel forbids contraction, so every f32
        operation rounds once; counted from the kernel, HIP's documented 1 ulp for sqrtf and the f32 divide as 2 u each):
          g' = g + wd p  (Adam's L2 branch only)   wd p, the sum: 2        t_g = K u (|g| + wd |p|)
          m  = m + b1w (g' - m)      b1w = f32(1 - beta1), the difference, the product, the sum: 4
                                     t_m = ulp + K u (|m| + (1 - beta1)(|g'| + |m|)) + (1 - beta1) t_g
          v  = b2 v + b2w g' g'      b2 and its product: 2 on b2 v; b2w and two products: 3 on b2w g'^2; the sum 1: 4 at most
                                     t_v = ulp + K u v + (1 - beta2)(2 |g'| t_g + t_g^2)
          den = sqrtf(v) / f32(sqrt(bc2)) + eps    sqrtf 2, the constant 1, the divide 2, the sum 1: 6
                                     t_den = (sqrt(v + t_v) - sqrt(v)) / sqrt(bc2) + K u den
          p  = p - lr wd p (AdamW) - f32(lr / bc1) m / den    lr wd, its product with p, the difference: 3 on a_p = |p| +
               lr wd |p|;  the step size 1, its product with m 1, the divide 2, the difference 1: 5 on q = ss |m| / den
                                     t_p = ulp + K u (a_p + q) + ss t_m / den + ss (|m| + t_m) t_den / (den den_lo)
        The error of m, v and den is carried into p: |m'/den' - m/den| <= t_m / den + |m'| |den - den'| / (den den') with
        |m'| <= |m| + t_m and den' >= den_lo = max(den - t_den, eps): the bound holds where g + wd p nearly cancels and den
        comes down to eps, where the quotient magnifies the error of that sum."""
        u, K = 2.0 ** -24, ADAM_K
        b1, b2 = float(betas[0]), float(betas[1])
        lr64 = float(torch.as_tensor(lr).to(torch.float32).reshape(()).item())
        s = float(torch.as_tensor(step).reshape(()).item())
        wd = float(torch.tensor(float(weight_decay), dtype=torch.float32).item())
        ep = float(torch.tensor(float(eps), dtype=torch.float32).item())
        p, gg, m, v = (t.detach().to(F64) for t in (p0, g, m0, v0))
        if maximize:
            gg = -gg
        ap = p.abs()
        t_g = torch.zeros_like(p)
        if decoupled:
            pd, a_p, ag = p - lr64 * wd * p, ap + lr64 * wd * ap, gg.abs()
        else:
            pd, a_p, ag = p, ap, gg.abs()
            if wd != 0.0:
                ag = ag + wd * ap
                gg = gg + wd * p
                t_g = K * u * ag
        rm = m + (1 - b1) * (gg - m)
        a_m = m.abs() + (1 - b1) * (ag + m.abs())
        rv = b2 * v + (1 - b2) * gg * gg
        bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
        den = rv.sqrt() / bc2 ** 0.5 + ep
        ss = lr64 / bc1
        rp = pd - ss * rm / den
        t_m = ulp_f32(rm) + K * u * a_m + (1 - b1) * t_g
        t_v = ulp_f32(rv) + K * u * rv + (1 - b2) * (2 * gg.abs() * t_g + t_g * t_g)
        t_den = ((rv + t_v).sqrt() - rv.sqrt()) / bc2 ** 0.5 + K * u * den
        q = ss * rm.abs() / den
        den_lo = torch.clamp(den - t_den, min=ep * (1 - K * u))  # the kernel's denominator is never below f32(eps)
        t_p = ulp_f32(rp) + K * u * (a_p + q) + ss * t_m / den + ss * (rm.abs() + t_m) / (den * den_lo) * t_den
        out = [self._add(call, _compare(p1.detach(), rp, t_p, "p")),
               self._add(call, _compare(m1.detach(), rm, t_m, "exp_avg")),
               self._add(call, _compare(v1.detach(), rv, t_v, "exp_avg_sq"))]
        return out

    # ---- pooling, loss, layout -------------------------------------------------------------------

    def maxpool_fwd(self, call, x, y, idx):
        B, H, W, C = x.shape
        Ho, Wo = y.shape[1:3]
        hp, wp = max(H + 2, 2 * Ho + 1), max(W + 2, 2 * Wo + 1)
        xp = F.pad(x.to(F64), (0, 0, 1, wp - W - 1, 1, hp - H - 1), value=float("-inf"))
        taps = torch.stack([xp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r in range(3) for s in range(3)])
        r = taps.max(0).values
        self._add(call, _compare(y, r, torch.zeros_like(r), "pooled max"))
        il = idx.long()
        picked = torch.gather(taps, 0, il.clamp(0, 8).unsqueeze(0)).squeeze(0)
        bad = (il > 8) | (picked != y.to(F64))
        res = _exact_zero(bad.to(torch.int8), "x[idx] == pooled")
        self._add(call, res)

    def maxpool_bwd(self, call, dy, idx, in_hw, add, dx):
        B, Ho, Wo, C = dy.shape
        H, W = in_hw
        hp, wp = max(H + 2, 2 * Ho + 1), max(W + 2, 2 * Wo + 1)
        parts = []
        for b0, b1 in self._chunks(B):
            d = dy[b0:b1].to(F64)
            il = idx[b0:b1]
            acc = d.new_zeros((b1 - b0, hp, wp, C))
            acca = torch.zeros_like(acc)
            for t in range(9):
                r, s = divmod(t, 3)
                v = torch.where(il == t, d, torch.zeros_like(d))
                acc[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += v
                acca[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] += v.abs()
            ref, a = acc[:, 1:1 + H, 1:1 + W], acca[:, 1:1 + H, 1:1 + W]
            if add is not None:
                ad = add[b0:b1].to(F64)
                ref, a = ref + ad, a + ad.abs()
            parts.append(_shift(_compare(dx[b0:b1], ref, ulp_stored(ref, dx.dtype) + REL * a, "dx"), b0, dx.shape))
        return self._add(call, _merge(parts, "dx"))

    def softmax_ce(self, call, logits, targets, weights, K, grad_scale, out):
        loss, wsum, dlogits, pred = out[:4]
        sums = out[4] if len(out) > 4 else None
        Cp = logits.shape[-1]
        gs = 1.0 if grad_scale is None else float(grad_scale.reshape(-1)[0])
        w = weights.to(F64)
        tot_w = tot_l = tot_la = 0.0
        parts_d, parts_p = [], []
        s_ref = logits.new_zeros(Cp, dtype=F64)
        s_abs = logits.new_zeros(Cp, dtype=F64)
        B = logits.shape[0]
        chunks = self._chunks(B)
        wp_list = []
        for b0, b1 in chunks:
            z = logits[b0:b1, ..., :K].to(F64)
            t = targets[b0:b1].long()
            wp = w[t.clamp(max=K - 1)] * (t < K)
            lse = torch.logsumexp(z, dim=-1)
            zt = torch.gather(z, -1, t.clamp(max=K - 1).unsqueeze(-1)).squeeze(-1)
            tot_w += float(wp.sum())
            tot_l += float((wp * (lse - zt)).sum())
            tot_la += float((wp * (lse.abs() + zt.abs())).sum())
            wp_list.append(wp)
            if pred is not None:
                zb = logits[b0:b1, ..., :K].to(F64)
                pk = pred[b0:b1].long()
                ok = (pk < K) & (torch.gather(zb, -1, pk.clamp(max=K - 1).unsqueeze(-1)).squeeze(-1) == zb.max(-1).values)
                parts_p.append(_shift(_exact_zero((~ok).to(torch.int8), "pred is a maximiser"), b0, pred.shape))
        if tot_w == 0.0:
            # no pixel counts: the weighted mean is 0 / 0, NaN in torch.nn.CrossEntropyLoss and here; the label and the
            # gradient's pad channels are still defined, the gradient itself (0 * inf) is not
            self._add(call, _exact_zero(wsum, "wsum without a counted pixel"))
            self._add(call, _exact_zero((~loss.isnan()).to(torch.int8), "loss is NaN without a counted pixel"))
            if parts_p:
                self._add(call, _merge(parts_p, "pred"))
            if dlogits is not None and Cp > K:
                self._add(call, _exact_zero(dlogits[..., K:], "dlogits pad channels"))
            return
        self._add(call, _compare(wsum, torch.tensor([tot_w], dtype=F64, device=wsum.device),
                                 torch.tensor([REL * tot_w], dtype=F64, device=wsum.device), "wsum"))
        self._add(call, _compare(loss, torch.tensor([tot_l / tot_w], dtype=F64, device=loss.device),
                                 torch.tensor([REL * tot_la / tot_w], dtype=F64, device=loss.device), "loss"))
        if parts_p:
            self._add(call, _merge(parts_p, "pred"))
        if dlogits is not None:
            for (b0, b1), wp in zip(chunks, wp_list):
                z = logits[b0:b1, ..., :K].to(F64)
                t = targets[b0:b1].long()
                p = torch.softmax(z, dim=-1)
                oh = F.one_hot(t.clamp(max=K - 1), K).to(F64)
                f = (gs / tot_w) * wp.unsqueeze(-1)
                r = f * (p - oh)
                a = f.abs() * (p + oh)
                o = dlogits[b0:b1]
                parts_d.append(_shift(_compare(o[..., :K], r, ulp_stored(r, o.dtype) + REL * a, "dlogits"), b0, dlogits.shape))
                if Cp > K:
                    parts_d.append(_shift(_exact_zero(o[..., K:], "dlogits pad channels"), b0, dlogits.shape))
                parts_d.append(_shift(_exact_zero(torch.where((wp == 0).unsqueeze(-1), o, torch.zeros_like(o)),
                                                  "dlogits on zero-weight pixels"), b0, dlogits.shape))
                ov = o.to(F64).reshape(-1, Cp)
                s_ref += ov.sum(0)
                s_abs += ov.abs().sum(0)
            self._add(call, _merge([p for p in parts_d if p["what"] == "dlogits"], "dlogits"))
            self._add(call, _merge([p for p in parts_d if p["what"] != "dlogits"], "dlogits exact zeros"))
        if sums is not None:
            self._add(call, _compare(sums, s_ref, REL * s_abs, "per-class sums of the stored dlogits"))
            self.grad_sources.append(("dlogit sums", sums[:K].detach().clone()))

    def scale_inplace(self, call, before, scale, after):
        s = float(scale.reshape(-1)[0])
        r = before.to(F64) * s
        tol = torch.zeros_like(r) if s == 1.0 else ulp_stored(r, before.dtype)
        return self._add(call, _compare(after, r, tol, "x * s"))

    def nchw_to_nhwc(self, call, x, out):
        C = x.shape[1]
        r = x.float().permute(0, 2, 3, 1).to(out.dtype).to(F64)
        self._add(call, _compare(out[..., :C], r, torch.zeros_like(r), "values"))
        if out.shape[-1] > C:
            self._add(call, _exact_zero(out[..., C:], "pad channels"))

    def nhwc_to_nchw(self, call, x, channels, out):
        r = x[..., :channels].permute(0, 3, 1, 2).to(F64)
        self._add(call, _compare(out, r, torch.zeros_like(r), "values"))

    def bilinear(self, call, src, o, transpose):
        """forward: o [B,Ho,Wo,C] = resize of src [B,Hi,Wi,C] (align_corners=False, float64 source index);
        transpose: o [B,Hi,Wi,C] = the transposed map of src = dy [B,Ho,Wo,C].  The taps are non-negative, so the
        magnitude bound a is the same map on |src|.  A channel that is zero in all of src (the pad channels) must be
        exactly zero in o.  The kernel, like ATen for f32 tensors, takes the source coordinate in f32: at ratios that
        are no power of two that is a few 1e-6 of the step between two taps, far inside a bf16 ulp, but up to 2.9 times
        the f32 bound REL * a where the taps nearly cancel (tests/test_kernels_gpu.py::test_bilinear).  So f32 tensors
        are checked against the operation the kernel defines: the taps in float64 from the coordinate evaluated in
        f32 (source_coordinate_f32); bf16 tensors keep the float64 coordinate."""
        what = "dx" if transpose else "y"
        f32c = o.dtype == torch.float32
        if transpose:
            my = bilinear_matrix(o.shape[1], src.shape[1], src.device, f32c).t()
            mx = bilinear_matrix(o.shape[2], src.shape[2], src.device, f32c).t()
        else:
            my = bilinear_matrix(src.shape[1], o.shape[1], src.device, f32c)
            mx = bilinear_matrix(src.shape[2], o.shape[2], src.device, f32c)
        parts = []
        for b0, b1 in self._chunks(src.shape[0]):
            s = src[b0:b1].to(F64)
            r, a = resize2(s, my, mx), resize2(s.abs(), my, mx)
            tol = REL * a + (ulp_bf16(r) if o.dtype == torch.bfloat16 else 0.0)
            parts.append(_shift(_compare(o[b0:b1], r, tol, what), b0, o.shape))
        self._add(call, _merge(parts, what))
        dead = (src == 0).reshape(-1, src.shape[-1]).all(0)
        if bool(dead.any()):
            self._add(call, _exact_zero(o[..., dead], what + " pad channels"))

    def mean_stack(self, call, xs, divisor, o):
        d = float(len(xs) if divisor is None else divisor)
        r = sum(x.to(F64) for x in xs) / d
        a = sum(x.to(F64).abs() for x in xs) / abs(d)
        tol = REL * a + (ulp_bf16(r) if o.dtype == torch.bfloat16 else 0.0)
        return self._add(call, _compare(o, r, tol, "sum / divisor"))

    def layout_norm(self, call, x, mean, std, out, codes=None, group=1):
        """out [B,H,W,pitch] = ((x - mean[c]) / std[c]) of the raster samples x [B,C,H,W], image b flipped / rotated by
        codes[b // group] first; without mean / std the values themselves, rounded once to the stored type"""
        B, C = x.shape[:2]
        if out.shape[-1] > C:
            self._add(call, _exact_zero(out[..., C:], "pad channels"))
        parts = []
        for b0, b1 in self._chunks(B):
            xc = samples_f64(x[b0:b1])
            if codes is not None:
                xc = torch.stack([d4_gather(xc[i], int(codes[(b0 + i) // group])) for i in range(b1 - b0)])
            xc = xc.permute(0, 2, 3, 1)
            oc = out[b0:b1, ..., :C]
            if mean is None:
                r = xc.to(out.dtype).to(F64)
                parts.append(_shift(_compare(oc, r, torch.zeros_like(r), "values"), b0, out.shape))
                continue
            m, s = mean[:C].to(F64), std[:C].to(F64)
            r = (xc - m) / s
            a = (xc.abs() + m.abs()) / s.abs()
            tol = REL * a + (ulp_bf16(r) if out.dtype == torch.bfloat16 else 0.0)
            parts.append(_shift(_compare(oc, r, tol, "(x - mean) / std"), b0, out.shape))
        return self._add(call, _merge(parts, parts[0]["what"]))

    def d4_labels(self, call, t, codes, out):
        r = torch.stack([d4_gather(t[b], int(codes[b])) for b in range(t.shape[0])])
        self._add(call, _exact_zero((out != r).to(torch.int8), "labels"))

    def head_bias_grad(self, call, sums, abs_sums, db):
        """db [K] f32, the bias gradient of the layer that produced the logits, handed over as the loss kernel's
        per-class sums times the upstream gradient.  sums [Cp] float64: the column sums of the FINAL dlogits buffer
        (after the rescale, as the consuming node saw it); abs_sums [Cp] float64: the magnitude term of the softmax_ce
        sums check (sums of |stored dlogits|) times |upstream gradient|; one f32 rounding for the product."""
        K = db.shape[0]
        r = sums[:K]
        return self._add(call, _compare(db, r, REL * abs_sums[:K] + ulp_f32(r), "bias gradient from the loss sums"))

    def confusion(self, call, before, after, pred, target):
        """after = before + one count per pixel at [target, pred]; a pixel whose target or prediction is >= K (an
        ignored label, a label of a wider class set) contributes nothing: the kernel's contract (csrc/resample_loss.hip)"""
        K = before.shape[0]
        t, p = target.reshape(-1).long(), pred.reshape(-1).long()
        if t.numel() != p.numel():
            raise ValueError(f"{p.numel()} predictions for {t.numel()} targets")
        valid = (t < K) & (p < K)
        idx = t[valid] * K + p[valid]
        r = before + torch.bincount(idx, minlength=K * K).view(K, K).to(before.device)
        self._add(call, _exact_zero((after != r).to(torch.int8), "counts"))

    def onehot_to_index(self, call, onehot, out):
        """out [B,H,W] uint8 = the first maximum over the class axis of onehot [B,K,H,W]: no tolerance"""
        z = onehot.to(F64).permute(0, 2, 3, 1)
        if tuple(out.shape) != tuple(z.shape[:-1]):
            raise ValueError(f"indices of shape {tuple(out.shape)} for a one-hot map {tuple(onehot.shape)}")
        self._add(call, _exact_zero((out.long() != first_max(z)).to(torch.int8), "index"))


    # ---- the eval step: folded BatchNorm, uint8 outputs, test-time augmentation ------------------

    def bn_eval_params(self, call, gamma, beta, rm, rv, eps, scale, shift):
        """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale, both f32 vectors"""
        m, v = rm.to(F64), rv.to(F64)
        g = gamma.to(F64) if gamma is not None else torch.ones_like(m)
        bt = beta.to(F64) if beta is not None else torch.zeros_like(m)
        sc = g / torch.sqrt(v + float(eps))
        sh = bt - m * sc
        self._add(call, _compare(scale, sc, BN_EVAL_ULPS * ulp_f32(sc), "scale"))
        self._add(call, _compare(shift, sh, BN_EVAL_ULPS * ulp_f32(bt.abs() + (m * sc).abs()), "shift"))

    def _labels(self, call, z, out, op):
        """out (uint8) must be the first maximum of z [..., K] over the last axis: no exclusion, no tolerance"""
        n = top_two_ties(z)
        self.ties[op] += n
        call["ties"] = n
        if tuple(out.shape) != tuple(z.shape[:-1]):
            raise ValueError(f"labels of shape {tuple(out.shape)} for scores {tuple(z.shape)}")
        return self._add(call, _exact_zero((out.long() != first_max(z)).to(torch.int8), "label"))

    def _u8_codes(self, call, p64, out, what, kind):
        """out (uint8) against rint(255 p64): it may differ only where 255 p64 lies within HALF_OPEN of a half-integer,
        and then by 1.  The share of such values is capped on p64 alone, before out is looked at."""
        if tuple(out.shape) != tuple(p64.shape):
            raise ValueError(f"{what} of shape {tuple(out.shape)} for probabilities {tuple(p64.shape)}")
        scaled = 255.0 * p64
        open_ = (scaled - scaled.floor() - 0.5).abs() <= HALF_OPEN
        n_open, n = int(open_.sum().item()), open_.numel()
        self.open[kind][0] += n_open
        self.open[kind][1] += n
        if n_open > OPEN_MAX_SHARE * n:
            return self._add(call, {"what": what, "shape": tuple(p64.shape), "n": n, "fail": n_open, "worst": float("inf"),
                                    "error": f"{n_open} of {n} values within {HALF_OPEN} of a half-integer: more than "
                                             f"{OPEN_MAX_SHARE:.0%}, the reference decides too little"})
        return self._add(call, _compare(out, torch.round(scaled), open_.to(F64), what))

    def _u8_outputs(self, call, scores, p64, mode, out, op):
        """the three uint8 outputs of predict_u8 / tta_predict_u8: scores [B,h,w,K] decide the label (their first
        maximum), p64 [B,h,w,K] the bands; argmax_conf = the label plane and the largest band"""
        if mode not in PREDICT_MODES:
            raise ValueError(f"unknown output mode {mode!r}")
        if mode == "argmax":
            return self._labels(call, scores, out, op)
        if mode == "class_prob":
            return self._u8_codes(call, p64.permute(0, 3, 1, 2), out, "bands", "band")
        if out.dim() != 4 or out.shape[1] != 2:
            raise ValueError(f"argmax_conf output of shape {tuple(out.shape)}")
        self._labels(call, scores, out[:, 0], op)
        return self._u8_codes(call, p64.max(-1).values, out[:, 1], "confidence", "confidence")

    def predict_u8(self, call, logits, K, mode, crop, out):
        """out = the uint8 outputs of the window `crop` (y0, x0, h, w) of NHWC logits with K real classes"""
        z = crop_window(logits, crop)[..., :K].to(F64)
        return self._u8_outputs(call, z, torch.softmax(z, dim=-1), mode, out, "predict_u8")

    def tta_accumulate(self, call, acc0, logits, K, code, crop, first, acc1):
        """acc1 [B,h,w,Cp] f32 = (first ? 0 : acc0) + the float64 softmax of the view's logits [B,n,n,Cp] (made with the
        forward `code`) taken back to the tile's frame with inverse_code, over the window `crop`;
        flairhip.augment.tta_mean_probabilities of the one view is the definition.  csrc/tta.hip: "pad channels hold 0"."""
        from flairhip.augment import tta_mean_probabilities
        z = logits[..., :K].to(F64)
        call["logit_ties"] = top_two_ties(z)
        p = tta_mean_probabilities([z.permute(0, 3, 1, 2).cpu().numpy()], [int(code)])
        p = crop_window(torch.from_numpy(p).to(logits.device).permute(0, 2, 3, 1), crop)
        if tuple(acc1.shape[:3]) != tuple(p.shape[:3]):
            raise ValueError(f"accumulator {tuple(acc1.shape)} for a window of {tuple(p.shape[1:3])}")
        if first:
            r, mag = p, p
        else:
            before = acc0[..., :K].to(F64)
            r, mag = before + p, before.abs() + p
        self._add(call, _compare(acc1[..., :K], r, ulp_f32(r) + REL * mag, "accumulator"))
        if acc1.shape[-1] > K:
            self._add(call, _exact_zero(acc1[..., K:], "pad channels"))

    def tta_predict_u8(self, call, acc, mode, views, K, out):
        """the uint8 outputs of an accumulator of `views` views: labels from the accumulator itself, bands from acc / views"""
        a = acc[..., :K].to(F64)
        return self._u8_outputs(call, a, a / float(views), mode, out, "tta_predict_u8")

    def tta_probabilities(self, call, acc, views, K, out):
        r = (acc[..., :K].to(F64) / float(views)).permute(0, 3, 1, 2)
        if tuple(out.shape) != tuple(r.shape):
            raise ValueError(f"probabilities of shape {tuple(out.shape)} for an accumulator {tuple(acc.shape)}")
        return self._add(call, _compare(out, r, 2 * ulp_f32(r), "mean probabilities"))

    # ---- the U-TAE time-series branch (csrc/temporal.hip, flairhip/utae.py) -----------------------
    # Every kernel there keeps f32 between its loads and its single store, so the bound is the stored rounding plus
    # REL * a, with the first-order effect of a REL-relative error in each f32 intermediate (mean and rstd, the scores
    # and the softmax denominator, the argument of the encoding) added where the op forms one.  No bf16 rounding point
    # inside a kernel was found, so no 2^-8 term appears.

    def conv_transposed(self, call, x, w64, pad, o, bias=None, relu=False, what="out"):
        """o = relu?(F.conv_transpose2d(x, w, stride 1, padding=pad) + bias) for the weight w64 [in, out, k, k] of an
        nn.ConvTranspose2d -- which is also the input gradient of the convolution with OIHW weight w64 (pad = that
        convolution's padding; the output may be larger than the input).  Taken on the CPU: the tensors are small."""
        ci, co = w64.shape[:2]
        xc = x[..., :ci].to(F64).permute(0, 3, 1, 2).cpu()
        wc = w64.cpu()
        r = F.conv_transpose2d(xc, wc, padding=pad).permute(0, 2, 3, 1).to(x.device)
        a = F.conv_transpose2d(xc.abs(), wc.abs(), padding=pad).permute(0, 2, 3, 1).to(x.device)
        if tuple(r.shape[:3]) != tuple(o.shape[:3]):
            raise ValueError(f"transposed conv: output {tuple(o.shape)} where the reference gives {tuple(r.shape)}")
        if bias is not None:
            bb = bias[:co].to(F64)
            r, a = r + bb, a + bb.abs()
        if relu:
            r = r.clamp_min(0)
        if o.shape[-1] > co:
            self._add(call, _exact_zero(o[..., co:], what + " pad channels"))
        return self._add(call, _compare(o[..., :co], r, ulp_stored(r, o.dtype) + REL * a, what))

    def reflect_pad1(self, call, x, o):
        r = F.pad(x.permute(0, 3, 1, 2).to(F64), (1, 1, 1, 1), mode="reflect").permute(0, 2, 3, 1)
        if tuple(r.shape) != tuple(o.shape):
            raise ValueError(f"reflect_pad1: output {tuple(o.shape)} for an input {tuple(x.shape)}")
        return self._add(call, _compare(o, r, torch.zeros_like(r), "padded copy"))

    def reflect_pad1_bwd(self, call, dpad, o):
        """o[n, y, x] = the sum of dpad over the padded positions that read (y, x): the float64 adjoint of reflect_pad1"""
        def adjoint(t):
            t = t.clone()
            t[:, 2] += t[:, 0]
            t[:, -3] += t[:, -1]
            t = t[:, 1:-1]
            t[:, :, 2] += t[:, :, 0]
            t[:, :, -3] += t[:, :, -1]
            return t[:, :, 1:-1]
        d = dpad.to(F64)
        r, a = adjoint(d), adjoint(d.abs())
        if tuple(r.shape) != tuple(o.shape):
            raise ValueError(f"reflect_pad1_bwd: output {tuple(o.shape)} for a gradient {tuple(dpad.shape)}")
        return self._add(call, _compare(o, r, ulp_stored(r, o.dtype) + REL * a, "dx"))

    @staticmethod
    def _gn_rows(t, groups, seq):
        """[S, inner, G, C/G] view of an NHWC tensor whose GroupNorm statistics run over axes 1 and 3: one sample per
        image (seq None, nn.GroupNorm on [N,C,H,W]) or per pixel of each series (seq = (B, T): images n = b * T + t,
        nn.GroupNorm on [B*h*w, C, T] as LTAE2d builds it -- padded dates included)"""
        C = t.shape[-1]
        if seq is None:
            return t.reshape(t.shape[0], -1, groups, C // groups)
        B, T = seq
        if t.shape[0] != B * T:
            raise ValueError(f"group norm over sequences: {t.shape[0]} images for B * T = {B * T}")
        return t.reshape(B, T, -1, groups, C // groups).permute(0, 2, 1, 3, 4).reshape(-1, T, groups, C // groups)

    def _gn_stats(self, x, groups, seq, eps):
        """float64 statistics of the kernel's two passes and what a REL-relative error of its f32 sums does to them:
        mean (t_m), the centred squares (REL var, plus the f32 rounding of x - mean where |x| >> |x - mean|), rstd"""
        xg = self._gn_rows(x.to(F64), groups, seq)
        m = xg.mean((1, 3), keepdim=True)
        d = xg - m
        var = (d * d).mean((1, 3), keepdim=True)
        rs = 1.0 / torch.sqrt(var + float(eps))
        t_m = REL * xg.abs().mean((1, 3), keepdim=True) + ulp_f32(m)
        t_v = REL * var + 2.0 ** -23 * (d.abs() * (xg.abs() + m.abs())).mean((1, 3), keepdim=True)
        t_rs = 0.5 * rs ** 3 * t_v + ulp_f32(rs)
        return xg, m, d, rs, t_m, t_rs

    def group_norm(self, call, x, gamma, beta, groups, eps, relu, residual, o, seq=None):
        """o = [residual +] relu?((x - mean) * rstd * gamma + beta), biased statistics per (sample, group)"""
        xg, m, d, rs, t_m, t_rs = self._gn_stats(x, groups, seq, eps)
        g, b = gamma.to(F64).reshape(groups, -1), beta.to(F64).reshape(groups, -1)
        r = d * rs * g + b
        a = (xg.abs() + m.abs()) * rs * g.abs() + b.abs()
        if relu:
            r = r.clamp_min(0)
        if residual is not None:
            rr = self._gn_rows(residual.to(F64), groups, seq)
            r, a = r + rr, a + rr.abs()
        tol = ulp_stored(r, o.dtype) + REL * a + g.abs() * (rs * t_m + d.abs() * t_rs)
        return self._add(call, _compare(self._gn_rows(o, groups, seq), r, tol, "y"))

    def group_norm_bwd(self, call, x, dy, gamma, beta, groups, eps, relu, dx, dgamma, dbeta, seq=None):
        """g = dy * [pre > 0] * gamma, dx = rstd (g - mean(g) - xhat mean(g xhat)) per (sample, group);
        dgamma = sum dy' xhat, dbeta = sum dy' over samples and positions.  The ReLU mask follows the AMBIG_REL rule of
        bn_bwd: elements whose pre-activation is within AMBIG_REL of zero (and whose dy is not 0) may go either way."""
        xg, m, d, rs, t_m, t_rs = self._gn_stats(x, groups, seq, eps)
        dg = self._gn_rows(dy.to(F64), groups, seq)
        g, b = gamma.to(F64).reshape(groups, -1), beta.to(F64).reshape(groups, -1)
        n = xg.shape[1] * xg.shape[3]
        xh = d * rs
        t_xh = rs * t_m + d.abs() * t_rs
        amb, namb = None, 0
        gm = dg
        if relu:
            pre = xh * g + b
            amb = (pre.abs() <= AMBIG_REL * ((xh * g).abs() + b.abs())) & (dg != 0)
            gm = torch.where(pre > 0, dg, torch.zeros_like(dg))
            namb = int(amb.sum().item())
            self.ambiguous[0] += namb
            self.ambiguous[1] += x.numel()
            if namb > AMBIG_MAX_FRACTION * x.numel():
                self._add(call, {"what": "ambiguous ReLU masks", "shape": tuple(x.shape), "n": x.numel(), "fail": namb,
                                 "worst": float("inf"), "error": f"{namb} ambiguous of {x.numel()}"})
        open_ = torch.zeros_like(dg) if amb is None else torch.where(amb, dg.abs(), torch.zeros_like(dg))
        sb, sg = gm.sum((0, 1)).reshape(-1), (gm * xh).sum((0, 1)).reshape(-1)
        t_b = REL * gm.abs().sum((0, 1)).reshape(-1) + open_.sum((0, 1)).reshape(-1) + ulp_f32(sb)
        t_g = (REL * (gm * xh).abs().sum((0, 1)) + (gm.abs() * t_xh).sum((0, 1)) + (open_ * xh.abs()).sum((0, 1))
               ).reshape(-1) + ulp_f32(sg)
        self._add(call, dict(_compare(dbeta, sb, t_b, "dbeta"), ambiguous=namb))
        self._add(call, _compare(dgamma, sg, t_g, "dgamma"))
        self.grad_sources += [("dgamma", dgamma.detach().clone()), ("dbeta", dbeta.detach().clone())]
        gg = gm * g
        mean = lambda t: t.mean((1, 3), keepdim=True)
        m1, m2 = mean(gg), mean(gg * xh)
        r = rs * (gg - m1 - xh * m2)
        big = gg.abs() + mean(gg.abs()) + xh.abs() * mean((gg * xh).abs())
        e1, e2 = mean(open_ * g.abs()), mean(open_ * g.abs() * xh.abs())
        tol = ulp_stored(r, dx.dtype) + REL * rs * big + t_rs * big \
            + rs * (t_xh * m2.abs() + xh.abs() * mean(gg.abs() * t_xh)) + rs * (e1 + xh.abs() * e2)
        return self._add(call, _compare(self._gn_rows(dx, groups, seq), r, tol, "dx", exclude=amb))

    def positional_encoding(self, call, pos, d, repeat, period, o):
        """o[n, r*d + j] = sin (j even) / cos (j odd) of pos[n] / period^(2 (j // 2) / d); the f32 argument errs by
        REL of itself, which moves the value by as much (|sin'|, |cos'| <= 1)"""
        p = pos.reshape(-1).to(F64)
        j = torch.arange(d, dtype=F64, device=p.device)
        arg = p[:, None] / torch.pow(torch.tensor(float(period), dtype=F64, device=p.device),
                                     2.0 * torch.div(j, 2, rounding_mode="floor") / d)
        r = torch.where((torch.arange(d, device=p.device) % 2 == 1)[None, :], torch.cos(arg), torch.sin(arg))
        r, arg = r.repeat(1, repeat), arg.repeat(1, repeat)
        if tuple(r.shape) != tuple(o.shape):
            raise ValueError(f"positional_encoding: output {tuple(o.shape)}, expected {tuple(r.shape)}")
        return self._add(call, _compare(o, r, REL * (1.0 + arg.abs()), "encoding"))

    def add_rowvec(self, call, before, vec, after):
        v = vec.to(F64)[:, None, None, :]
        r = before.to(F64) + v
        a = before.to(F64).abs() + v.abs()
        return self._add(call, _compare(after, r, ulp_stored(r, after.dtype) + REL * a, "x + vec"))

    def detect_pad_images(self, call, x, value, o):
        r = (x.reshape(x.shape[0], -1) == float(value)).all(1)
        return self._add(call, _exact_zero((o.bool() != r).to(torch.int8), "pad flags"))

    def mask_images(self, call, before, pad, value, after):
        fill = torch.tensor(float(value), dtype=before.dtype, device=before.device)
        keep = (pad == 0).reshape((-1,) + (1,) * (before.dim() - 1))
        r = torch.where(keep, before, fill).to(F64)
        return self._add(call, _compare(after, r, torch.zeros_like(r), "masked copy"))

    def mul(self, call, x, m, o):
        r = x.to(F64) * m.to(F64)
        return self._add(call, _compare(o, r, ulp_stored(r, o.dtype) + REL * r.abs(), "x * m"))

    @staticmethod
    def _ltae_views(k, v, Q, pad, drop, B, T):
        NH, DK = Q.shape
        k5 = k.to(F64).reshape(B, T, -1, NH, DK)
        v5 = v.to(F64).reshape(B, T, k5.shape[2], NH, -1)
        padm = (pad.reshape(B, T) != 0)[:, :, None, None]
        dr = None if drop is None else drop.to(F64).permute(1, 2, 3, 0)
        return k5, v5, Q.to(F64), padm, dr

    def ltae_attention(self, call, k, v, Q, pad, drop, B, T, out, attn, prob=None):
        """score[t] = <Q[h], k[t]> / sqrt(d_k), padded dates -1e3, prob = softmax over the dates, attn = prob * drop,
        out = sum_t attn[t] v[t].  A score errs by REL of its magnitude sum (t_s); the softmax passes that on as
        p_t (t_s[t] + sum_u p_u t_s[u]) and adds REL p for the exponential and the denominator."""
        k5, v5, q, padm, dr = self._ltae_views(k, v, Q, pad, drop, B, T)
        temp = float(q.shape[1]) ** 0.5
        s = ((k5 * q).sum(-1) / temp).masked_fill(padm, -1e3)
        t_s = (REL * (k5 * q).abs().sum(-1) / temp).masked_fill(padm, 0.0)
        p = torch.softmax(s, dim=1)
        t_p = REL * p + p * (t_s + (p * t_s).sum(1, keepdim=True))
        at, t_a = (p, t_p) if dr is None else (p * dr, t_p * dr)
        r = (at[..., None] * v5).sum(1)
        a = (at[..., None] * v5.abs()).sum(1)
        tol = ulp_stored(r, out.dtype) + REL * a + (t_a[..., None] * v5.abs()).sum(1)
        self._add(call, _compare(out.reshape(r.shape), r, tol, "out"))
        self._add(call, _compare(attn.permute(1, 2, 3, 0), at, t_a, "attn"))
        if prob is not None:
            self._add(call, _compare(prob.permute(1, 2, 3, 0), p, t_p, "prob"))

    def ltae_attention_bwd(self, call, k, v, Q, pad, drop, prob, dout, dattn_ext, B, T, dk, dv, dq):
        """from the saved clean prob: da = <dout, v> + dattn_ext, dp = da drop, ds = prob (dp - sum prob dp), 0 at a
        padded date, over sqrt(d_k); dk = ds Q, dv = prob drop dout, dQ = sum over samples, dates and pixels of ds k"""
        k5, v5, q, padm, dr = self._ltae_views(k, v, Q, pad, drop, B, T)
        temp = float(q.shape[1]) ** 0.5
        p = prob.to(F64).permute(1, 2, 3, 0)
        dr = torch.ones_like(p) if dr is None else dr
        go = dout.to(F64).reshape(B, 1, k5.shape[2], q.shape[0], -1)
        da, a_da = (go * v5).sum(-1), (go * v5).abs().sum(-1)
        if dattn_ext is not None:
            ext = dattn_ext.to(F64).permute(1, 2, 3, 0)
            da, a_da = da + ext, a_da + ext.abs()
        t_da = REL * a_da
        dp = da * dr
        ds = p * (dp - (p * dp).sum(1, keepdim=True))
        t_ds = p * (dr * t_da + (p * dr * t_da).sum(1, keepdim=True)) \
            + REL * p * (dp.abs() + (p * dp.abs()).sum(1, keepdim=True))
        ds, t_ds = ds.masked_fill(padm, 0.0) / temp, t_ds.masked_fill(padm, 0.0) / temp
        r = ds[..., None] * q
        self._add(call, _compare(dk.reshape(r.shape), r, ulp_stored(r, dk.dtype) + REL * r.abs() + t_ds[..., None] * q.abs(),
                                 "dk"))
        r = (p * dr)[..., None] * go
        self._add(call, _compare(dv.reshape(r.shape), r, ulp_stored(r, dv.dtype) + REL * r.abs(), "dv"))
        r = (ds[..., None] * k5).sum((0, 1, 2))
        tol = REL * (ds.abs()[..., None] * k5.abs()).sum((0, 1, 2)) + (t_ds[..., None] * k5.abs()).sum((0, 1, 2)) + ulp_f32(r)
        self._add(call, _compare(dq, r, tol, "dQ"))
        self.grad_sources.append(("dQ", dq.detach().clone()))

    @staticmethod
    def _aggregate_views(x, attn, pad, B, T, use_pad):
        NH = attn.shape[0]
        x5 = x.to(F64).reshape(B, T, -1, NH, x.shape[-1] // NH)
        a4 = attn.to(F64).permute(1, 2, 3, 0)
        dead = (pad.reshape(B, T) != 0)[:, :, None, None] & bool(use_pad)
        return x5, a4.masked_fill(dead, 0.0) if use_pad else a4, dead

    def temporal_aggregate(self, call, x, attn, pad, B, T, use_pad, o):
        """o[b, p, c] = sum_t attn[c // (C / n_head), b, t, p] x[b, t, p, c], padded dates left out when use_pad"""
        x5, a4, _ = self._aggregate_views(x, attn, pad, B, T, use_pad)
        r = (a4[..., None] * x5).sum(1)
        a = (a4.abs()[..., None] * x5.abs()).sum(1)
        return self._add(call, _compare(o.reshape(r.shape), r, ulp_stored(r, o.dtype) + REL * a, "out"))

    def temporal_aggregate_bwd(self, call, x, attn, pad, dout, B, T, use_pad, dx, dattn):
        x5, a4, dead = self._aggregate_views(x, attn, pad, B, T, use_pad)
        go = dout.to(F64).reshape(B, 1, x5.shape[2], x5.shape[3], -1)
        r = a4[..., None] * go
        self._add(call, _compare(dx.reshape(r.shape), r, ulp_stored(r, dx.dtype) + REL * r.abs(), "dx"))
        r = (x5 * go).sum(-1).masked_fill(dead, 0.0)
        a = (x5 * go).abs().sum(-1).masked_fill(dead, 0.0)
        self._add(call, _compare(dattn.permute(1, 2, 3, 0), r, REL * a, "dattn"))

    def column_sums(self, call, x, o):
        v = x.to(F64).reshape(-1, x.shape[-1])
        return self._add(call, _compare(o, v.sum(0), REL * v.abs().sum(0), "column sums"))

    def packed_bias(self, call, bias, holder_bias, n_out, scale=None, shift=None):
        """the bias vector HipUTAE._packed hands out with an operand: the layer's bias, in eval mode
        shift + scale * bias (one f32 multiply and add), zeros behind the real channels"""
        r = bias.new_zeros(bias.shape, dtype=F64)
        tol = torch.zeros_like(r)
        if holder_bias is not None:
            hb = holder_bias.to(F64)
            if scale is None:
                r[:n_out] = hb
            else:
                sc, sh = scale[:n_out].to(F64), shift[:n_out].to(F64)
                r[:n_out] = sh + sc * hb
                tol[:n_out] = 2 * ulp_f32(sh.abs() + (sc * hb).abs())
        return self._add(call, _compare(bias, r, tol, "bias vector"))


# --------------------------------------------------------------------------------------------------
# the recorder: patches flairhip.ops and dispatches every outermost call to the Checker

def _clone(v):
    return v.detach().clone() if torch.is_tensor(v) else v


class Recorder(Checker):
    """with Recorder(model, mode) as rec: <training step>  -- then rec.results / rec.calls / rec.unchecked"""

    def __init__(self, model=None, mode="full", chunk=2, seed=1234):
        super().__init__(mode, chunk, seed)
        self.names = {}
        self._fold_params = None  # (scale, shift) of the bn_eval_params call inside the running _eval_folded, if any
        self.adopt(model)
        self.depth = 0
        self.unchecked = defaultdict(int)
        self.counts = defaultdict(int)
        self._saved = []
        self._wcache = {}
        self._chains = {}        # fusion conv name -> real channels of the links of its forward chain, in order
        self._scaled = {}        # address of a rescaled dlogits buffer -> what its consumer's bias gradient must be
        self.head_bias = {}      # module name of a head -> the entry of _scaled its dgrad call consumed
        self.sum_inputs = {}     # id of a checked column_sums output -> (call index, (address, shape) of what it summed)
        self.wgrad_operands = []  # (call index, (address, shape)) of the x and dy of every checked conv_wgrad call
        self._dattn_parts = []   # dattn of the temporal_aggregate_bwd calls since the last ltae_attention_bwd
        self._convT_grad = None  # (call index, (address, shape)) of the output gradient a ConvTranspose2d's backward read

    def adopt(self, model):
        """take the module names of `model` (a program that builds its model inside the recording hands it over here)"""
        self.model = model
        if model is not None:
            self.names.update({id(m): n for n, m in model.named_modules()})

    # ---- patching ------------------------------------------------------------------------------

    def __enter__(self):
        from flairhip import nn as hnn
        from flairhip import ops
        self._ops = ops
        for name, fn in list(vars(ops).items()):
            if name.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
                continue
            if name in HELPERS:
                continue
            self._saved.append((ops, name, fn))
            setattr(ops, name, self._wrap(name, fn))
        orig_packed = hnn.HipConv2d.packed
        rec = self

        def packed(mod, dtype, transpose=False, *a, **kw):
            pw = orig_packed(mod, dtype, transpose, *a, **kw)
            key = (id(mod), mod.weight._version, mod.weight.data_ptr(), hnn.state_epoch())
            w = rec._wcache.get(key)
            if w is None:
                w = rec._wcache[key] = mod.weight.detach().clone()
            rec.weights[id(pw)] = {"name": rec.names.get(id(mod), "?"), "transpose": bool(transpose), "weight": w,
                                   "stride": mod.stride, "padding": mod.padding}
            return pw

        self._saved.append((hnn.HipConv2d, "packed", orig_packed))
        hnn.HipConv2d.packed = packed
        orig_slice = hnn._fusion_slice

        def fusion_slice(conv, w, off, c, dtype, pitch, transpose):
            """the column block of a fusion 1x1 weight: the reference keeps the whole master weight and the offset the
            product asked for; _conv_call takes the block where the chain of real channel counts puts it"""
            pw = orig_slice(conv, w, off, c, dtype, pitch, transpose)
            key = (id(conv), conv.weight._version, conv.weight.data_ptr(), hnn.state_epoch())
            full = rec._wcache.get(key)
            if full is None:
                full = rec._wcache[key] = conv.weight.detach().clone()
            rec.weights[id(pw)] = {"name": rec.names.get(id(conv), "?"), "transpose": bool(transpose), "master": full,
                                   "off": int(off), "c": int(c), "stride": 1, "padding": 0}
            return pw

        self._saved.append((hnn, "_fusion_slice", orig_slice))
        hnn._fusion_slice = fusion_slice
        orig_fold = hnn._eval_folded

        def eval_folded(conv, bn, dtype, *a, **kw):
            """the eval-mode operand: master weight, the product's own f32 scale vector (checked as bn_eval_params'
            output) and the shift the conv call must carry as its bias.  An operand the cache built before the
            recording gets its scale from a bn_eval_params call of the same state, recorded and checked like any other."""
            rec._fold_params = None
            pw, shift = orig_fold(conv, bn, dtype, *a, **kw)
            params, rec._fold_params = rec._fold_params, None
            known = rec.weights.get(id(pw))
            if params is None and (known is None or known.get("operand") is not pw):
                params = rec._ops.bn_eval_params(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                                 bn.eps)
            if params is not None:
                key = (id(conv), conv.weight._version, conv.weight.data_ptr(), hnn.state_epoch())
                w = rec._wcache.get(key)
                if w is None:
                    w = rec._wcache[key] = conv.weight.detach().clone()
                rec.weights[id(pw)] = {"name": rec.names.get(id(conv), "?"), "transpose": False, "weight": w,
                                       "scale": params[0].detach().clone(), "shift": shift, "operand": pw,
                                       "stride": conv.stride, "padding": conv.padding}
            return pw, shift

        self._saved.append((hnn, "_eval_folded", orig_fold))
        hnn._eval_folded = eval_folded
        from flairhip import utae as hutae
        orig_utae = hutae.HipUTAE._packed

        def utae_packed(net, tag, holder, ci_pitch, bn=None, transpose=False, cols=None, with_bias=True):
            """an operand of the U-TAE: the master weight as 4-D OIHW (Conv1d / Linear weights are 1x1 convolutions), the
            column slice and the transpose flag the product asked for, in eval mode the product's own bn_eval_params
            scale (checked like any other call).  The bias vector that comes with the operand is checked here; a conv
            call on the operand must pass that very vector.  Padding comes from the call."""
            rec._fold_params = None
            pw, bias = orig_utae(net, tag, holder, ci_pitch, bn=bn, transpose=transpose, cols=cols, with_bias=with_bias)
            params, rec._fold_params = rec._fold_params, None
            known = rec.weights.get(id(pw))
            fresh = known is None or known.get("operand") is not pw
            if bn is not None and params is None and fresh:
                params = rec._ops.bn_eval_params(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var,
                                                 bn.eps)
            if not fresh and params is None:
                return pw, bias
            key = (id(holder), holder.weight._version, holder.weight.data_ptr(), hnn.state_epoch())
            w = rec._wcache.get(key)
            if w is None:
                w = holder.weight.detach().float()
                w = w.reshape(tuple(w.shape) + (1,) * (4 - w.dim())).clone()
                rec._wcache[key] = w
            c0, c1, _ = (cols if cols is not None else slice(None)).indices(w.shape[1])
            name = rec.names.get(id(holder), "?")
            info = {"name": name, "tag": tag, "utae": True, "transpose": bool(transpose), "weight": w, "cols": (c0, c1),
                    "operand": pw, "stride": 1, "padding": None, "bias": bias, "with_bias": bool(with_bias)}
            if params is not None:
                info["scale"], info["shift"] = params[0].detach().clone(), params[1].detach().clone()
            rec.weights[id(pw)] = info
            n_out = w.shape[1] if transpose else w.shape[0]
            with torch.no_grad():
                rec.packed_bias({"op": "utae_packed", "family": "utae_packed_bias", "call": f"packed:{tag}", "module": name},
                                bias, holder.bias.detach() if with_bias else None, n_out, info.get("scale"),
                                info.get("shift"))
            return pw, bias

        self._saved.append((hutae.HipUTAE, "_packed", orig_utae))
        hutae.HipUTAE._packed = utae_packed
        return self

    def __exit__(self, *exc):
        for obj, name, fn in reversed(self._saved):
            setattr(obj, name, fn)
        self._saved = []
        return False

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)
        rec = self

        def wrapper(*args, **kw):
            if rec.depth > 0:
                return fn(*args, **kw)
            check = getattr(rec, "_op_" + name, None)
            if check is None:
                rec.unchecked[name] += 1
                return fn(*args, **kw)
            ba = sig.bind(*args, **kw)
            ba.apply_defaults()
            pre = {k: _clone(v) for k, v in ba.arguments.items()}
            rec.depth += 1
            try:
                out = fn(*args, **kw)
            finally:
                rec.depth -= 1
            rec.counts[name] += 1
            call = {"op": name, "call": len(rec.calls)}
            try:
                with torch.no_grad():
                    check(call, pre, ba.arguments, out)
            except Exception as e:  # a reference that cannot run is a failed check, not a crash of the step
                rec._add(call, {"what": "reference", "shape": None, "n": 0, "fail": 1, "worst": float("inf"),
                                "error": f"{type(e).__name__}: {e}"})
            rec.calls.append(call)
            return out

        return wrapper

    # ---- per-op adapters: (call summary, cloned inputs, live arguments, outputs) ----------------

    def _fusion_block(self, call, info, residual):
        """master columns of one link of a fusion 1x1 conv.  The offset is not taken from the product: the links of a
        forward chain (it starts at the call without a residual) occupy the columns in call order, each as many as its
        source has real channels, and together all of them; a dgrad link must be one of the blocks of that chain."""
        W, off, c, name = info["master"], info["off"], info["c"], info["name"]
        call.update(fusion=True, off=off, c=c, module=name)
        if not info["transpose"]:
            chain = self._chains[name] = [] if residual is None else self._chains.get(name)
            if chain is None:
                raise ValueError("fusion link with a residual before the first link of its chain")
            want = sum(chain)
            chain.append(c)
            if sum(chain) > W.shape[1]:
                raise ValueError(f"fusion chain of {sum(chain)} channels over a weight of {W.shape[1]} columns")
        else:
            chain = self._chains.get(name) or []
            starts = {sum(chain[:m]): cm for m, cm in enumerate(chain)}
            if sum(chain) != W.shape[1] or starts.get(off) != c:
                raise ValueError(f"dgrad block [{off}, {off + c}) is no link of the forward chain {chain} "
                                 f"over {W.shape[1]} columns")
            want = off
        blk = W[:, want:want + c]
        if off != want:
            raise ValueError(f"fusion block taken at column {off}, the chain of real channels puts it at {want}")
        return blk

    @staticmethod
    def _operand_values(call, info, pw, W, bias):
        """float64 values of the packed operand: the master weight rounded to the storage type, for an eval-mode operand
        with the product's scale folded in as the packer does it (folded_weight).  Such an operand must be called with
        the shift of its own fold as the bias, bit for bit."""
        bf16 = pw.data.dtype == torch.bfloat16
        call["folded"] = "scale" in info
        if not call["folded"]:
            return bf16_round(W) if bf16 else W.to(F64)
        if info["transpose"]:
            raise ValueError("eval-mode fold on a dgrad operand")
        if bias is None or not torch.equal(bias, info["shift"]):
            raise ValueError("eval-mode operand called without the shift of its fold as the bias")
        return folded_weight(W, info["scale"], bf16)

    def _conv_call(self, call, a, out, w, dil, residual, bias=None, relu=False, stats=False):
        info = self._weight(a["w"])
        pw = a["w"]
        W = self._fusion_block(call, info, residual) if "master" in info else info["weight"]
        w64 = self._operand_values(call, info, pw, W, bias)
        call.update(module=info["name"], layout=layout_of(pw), transpose=info["transpose"], kernel=f"{pw.kh}x{pw.kw}",
                    stride=pw.stride, dil=dil, residual=residual is not None, stats=stats, bias=bias is not None,
                    relu=bool(relu))
        x = a["x"]
        # conv3x3_persist_kernel (a block walks several tiles) or one tile per block: the library's own answer
        call.update(dtype=str(x.dtype).replace("torch.", ""),
                    persistent=self._ops.conv_is_persistent(x.dtype, out.shape[0], out.shape[1], out.shape[2], pw, dil))
        if not info["transpose"]:
            call["family"] = "fwd"
            return self.conv_forward(call, x, w64, pw.stride, a["pad"], out, bias=bias, residual=residual, relu=relu)
        call["family"] = "dgrad" + ("_dil2" if dil == 2 else "") + ("_residual" if residual is not None else "")
        if bias is not None or relu:
            raise ValueError("dgrad call with bias / relu")
        return self.conv_dgrad(call, x, w64, dil, pw.kh - 1 - a["pad"], out, residual=residual)

    def _op_conv2d(self, call, a, live, out):
        if a["stats"] is not None:
            raise ValueError("conv2d with a statistics buffer outside conv2d_bn_stats")
        # a dgrad call that reads a rescaled dlogits buffer is the backward of the head that produced those logits: its
        # node is the one that takes the loss sums for its bias gradient
        hit = self._scaled.pop(live["x"].data_ptr(), None)
        if hit is not None and hit["shape"] == tuple(live["x"].shape):
            info = self.weights.get(id(a["w"]))
            if info is not None and info["transpose"]:
                self.head_bias[info["name"]] = hit
        info = self.weights.get(id(a["w"]))
        if info is not None and info.get("utae"):
            return self._utae_conv(call, a, live, out, info)
        self._conv_call(call, a, out, a["w"], a["dil"], a["residual"], bias=a["bias"], relu=a["relu"])

    def _utae_conv(self, call, a, live, out, info):
        """conv2d on an operand of HipUTAE._packed.  Forward operands: the convolution of the call's padding with the
        column slice of the master weight (the second link of a sliced pair comes through the residual input).
        Transposed operands, whatever the product uses them for -- ConvTranspose2d(3, 1, 1) as a pad-1 conv, the input
        gradient of a pad-0 conv as a pad-(k-1) conv with out_hw -- are held to F.conv_transpose2d of the master weight
        [in, out, k, k] with padding k - 1 - pad: the transposed convolution and the adjoint are one map."""
        pw = a["w"]
        c0, c1 = info["cols"]
        W = info["weight"][:, c0:c1]
        transpose, tag = info["transpose"], info["tag"]
        n_out = W.shape[1] if transpose else W.shape[0]
        folded = "scale" in info
        if folded:  # the packer's fold (csrc/conv_pack.hip): w * scale[row] in f32, then the storage rounding
            sc = info["scale"].float()[:n_out]
            W = W.float() * (sc[None, :, None, None] if transpose else sc[:, None, None, None])
        w64 = bf16_round(W) if pw.data.dtype == torch.bfloat16 else W.to(F64)
        bias, residual = a["bias"], a["residual"]
        if bias is not None and not torch.equal(bias, info["bias"]):
            raise ValueError("conv call with another bias vector than the one packed with its operand")
        if bias is not None and not info["with_bias"] and bool((bias != 0).any()):
            raise ValueError("conv call with the bias vector of an operand packed without one")
        if folded and bias is None and residual is None:
            raise ValueError("eval-mode operand called without the shift of its fold")
        if a["dil"] != 1 or a["stats"] is not None:
            raise ValueError("U-TAE conv call with a dilation or a statistics buffer")
        call.update(module=info["name"], tag=tag, layout=layout_of(pw), transpose=transpose, kernel=f"{pw.kh}x{pw.kw}",
                    stride=1, dil=1, residual=residual is not None, bias=bias is not None, relu=bool(a["relu"]),
                    folded=folded, cols=(c0, c1), sliced=(c1 - c0) != info["weight"].shape[1],
                    out_hw=a["out_hw"] is not None, dtype=str(a["x"].dtype).replace("torch.", ""), utae=True)
        if not transpose:
            call["family"] = "utae_fwd"
            if tag.endswith(":D"):  # the input gradient of a ConvTranspose2d: a forward conv of the output gradient
                self._convT_grad = (call["call"], (live["x"].data_ptr(), tuple(live["x"].shape)))
            return self.conv_forward(call, a["x"], w64, 1, a["pad"], out, bias=bias, residual=residual, relu=a["relu"])
        if residual is not None:
            raise ValueError("transposed U-TAE operand called with a residual")
        call["family"] = "utae_dgrad" if tag.endswith(":T") else "utae_conv_transpose"
        return self.conv_transposed(call, a["x"], w64, pw.kh - 1 - a["pad"], out, bias=bias, relu=a["relu"],
                                    what="dx" if tag.endswith(":T") else "out")

    def _op_conv2d_bn_stats(self, call, a, live, out):
        y0, scale, shift, mean, rstd = out
        self._conv_call(call, a, y0, a["w"], 1, None, stats=True)
        self.bn_stats(dict(call, family="bn_stats", layout=None), y0, a["gamma"], a["beta"], a["running_mean"], a["running_var"], live["running_mean"],
                      live["running_var"], a["momentum"], a["eps"], scale, shift, mean, rstd)

    def _upcat_weight(self, call, pw, bias=None):
        info = self._weight(pw)
        call.update(module=info["name"], layout=layout_of(pw), transpose=info["transpose"], kernel="3x3",
                    dtype=str(pw.data.dtype).replace("torch.", ""))
        return self._operand_values(call, info, pw, info["weight"], bias)

    def _op_conv2d_upcat(self, call, a, live, out, stats=False):
        if out is None:
            return
        w64 = self._upcat_weight(call, a["w"], a.get("bias"))
        call.update(family="upcat_fwd", stats=stats, bias=a.get("bias") is not None, relu=bool(a.get("relu", False)),
                    residual=False)
        lo, skip = a["lo"], a["skip"]
        c1, c2 = lo.shape[-1], (0 if skip is None else skip.shape[-1])
        call.update(c1=c1, c2=c2)
        if w64.shape[1] != c1 + c2:
            raise ValueError("two-source conv: pitch != real input channels")

        class _Cat:  # lazily concatenated input, sliced per batch chunk
            shape = (lo.shape[0], 2 * lo.shape[1], 2 * lo.shape[2], c1 + c2)

            def __getitem__(self, idx):
                bs = idx[0]
                return upcat(lo[bs].to(F64), None if skip is None else skip[bs].to(F64))[..., :c1 + c2]

        return self.conv_forward(call, _Cat(), w64, 1, 1, out, bias=a.get("bias"), relu=a.get("relu", False))

    def _op_conv2d_upcat_bn_stats(self, call, a, live, out):
        y0, scale, shift, mean, rstd = out
        self._op_conv2d_upcat(call, dict(a, bias=None, relu=False), live, y0, stats=True)
        self.bn_stats(dict(call, family="bn_stats", layout=None), y0, a["gamma"], a["beta"], a["running_mean"], a["running_var"], live["running_mean"],
                      live["running_var"], a["momentum"], a["eps"], scale, shift, mean, rstd)

    def _op_conv2d_dgrad_upcat(self, call, a, live, out):
        if out is None:
            return
        dlo, dskip = out
        w64 = self._upcat_weight(call, a["wt"])
        c1, c2 = a["c1"], a["c2"]
        call.update(family="upcat_dgrad", c1=c1, c2=c2)
        dy = a["dy"]
        B, H, W, _ = dy.shape
        O = w64.shape[0]
        wa = w64.abs()
        for part, sel, o in (("dlo", slice(0, c1), dlo), ("dskip", slice(c1, c1 + c2), dskip)):
            if o is None:
                continue
            wp, wpa = w64[:, sel], wa[:, sel]
            pool = part == "dlo"

            def ref(b0, b1, u, wp=wp, wpa=wpa, pool=pool):
                d = dy[b0:b1, ..., :O].to(F64)
                if u is not None:
                    wp_, wpa_ = torch.einsum("oikl,ij->ojkl", wp, u), torch.einsum("oikl,ij->ojkl", wpa, u.abs())
                else:
                    wp_, wpa_ = wp, wpa
                r, aa = conv_scatter(d, wp_, 1, 1, H, W), conv_scatter(d.abs(), wpa_, 1, 1, H, W)
                return (pool2_sum(r), pool2_sum(aa)) if pool else (r, aa)

            self._check_linear(call, o, wp.shape[1], ref, part, B)

    def _op_conv_wgrad(self, call, a, live, out):
        call.update(family="wgrad", kernel=f"{a['kh']}x{a['kw']}", stride=a["stride"],
                    layout="thin" if (a["x"].dtype == torch.bfloat16 and a["x"].shape[-1] <= 32 and a["dy"].shape[-1] <= 32
                                      and a["kh"] == 3 and a["stride"] == 1) else "general",
                    dtype=str(a["x"].dtype).replace("torch.", ""))
        call.update(co=out.shape[0], ci=out.shape[1], hw=tuple(a["x"].shape[1:3]))
        before = a["out"] if a["accumulate"] else None
        self.wgrad_operands += [(call["call"], (live[k].data_ptr(), tuple(live[k].shape))) for k in ("x", "dy")]
        node, self._convT_grad = self._convT_grad, None
        if node is not None and call["call"] == node[0] + 1:
            # y = C^T x for the convolution C with OIHW weight w [in, out, k, k]: dW is the weight gradient of C with the
            # output gradient as C's input and x as C's output gradient -- the roles exchanged
            call["conv_transpose"] = True
            ok = node[1] == (live["x"].data_ptr(), tuple(live["x"].shape))
            self._add(call, {"what": "ConvTranspose2d weight gradient: x is the output gradient", "shape": tuple(out.shape),
                             "n": 1, "fail": 0 if ok else 1, "worst": 0.0 if ok else float("inf")})
        self.conv_wgrad(call, a["x"], a["dy"], a["kh"], a["kw"], a["stride"], a["pad"], out, before=before)
        self.grad_sources.append(("dW", out.detach().clone()))

    def _op_conv_wgrad_upcat(self, call, a, live, out):
        if out is None:
            return
        lo, skip = a["lo"], a["skip"]
        if lo.dtype == torch.float32:  # conv3x3_thin_wgrad_kernel is bf16-only
            call["layout"] = "general"
        call.update(family="upcat_wgrad", kernel="3x3", c1=lo.shape[-1], c2=0 if skip is None else skip.shape[-1],
                    dtype=str(lo.dtype).replace("torch.", ""))
        x = upcat(lo, skip)
        self.conv_wgrad(call, x, a["dy"], 3, 3, 1, 1, out)
        self.grad_sources.append(("dW", out.detach().clone()))

    def _op_upsample2x_concat_fwd(self, call, a, live, out):
        """the materialised decoder input where no two-source kernel takes the channel split: a copy, so exact"""
        call.update(family="upsample2x_concat_fwd", c1=a["lo"].shape[-1], c2=0 if a["skip"] is None else a["skip"].shape[-1])
        r = upcat(a["lo"], a["skip"])
        self._add(call, _exact_zero((out != r).to(torch.int8), "cat(nearest_x2(lo), skip)"))

    def _op_upsample2x_concat_bwd(self, call, a, live, out):
        """dlo = the 2 x 2 sums of the first c1 channels (four terms: REL * a + the stored rounding), dskip = the rest"""
        call["family"] = "upsample2x_concat_bwd"
        dlo, dskip = out
        c1, dcat = a["c1"], a["dcat"]
        parts = []
        for b0, b1 in self._chunks(dcat.shape[0]):
            d = dcat[b0:b1, ..., :c1].to(F64)
            r, mag = pool2_sum(d), pool2_sum(d.abs())
            parts.append(_shift(_compare(dlo[b0:b1], r, ulp_stored(r, dlo.dtype) + REL * mag, "dlo"), b0, dlo.shape))
        self._add(call, _merge(parts, "dlo"))
        if dskip is not None:
            self._add(call, _exact_zero((dskip != dcat[..., c1:]).to(torch.int8), "dskip"))

    def _op_bn_apply(self, call, a, live, out):
        call["family"] = "bn_apply"
        self.bn_apply(call, a["x"], a["scale"], a["shift"], a["residual"], a["relu"], out)

    def _op_bn_bwd(self, call, a, live, out):
        dx, dres, dg, db = out
        mode = 0 if not a["relu"] else (1 if a["y"] is not None else 2)
        call.update(family=f"bn_bwd_mode{mode}", dres=dres is not None)
        # a rescaled dlogits buffer that a BatchNorm consumes (the U-TAE's class-score layer) feeds no head's bias gradient
        self._scaled.pop(live["dy"].data_ptr(), None)
        self.bn_bwd(call, a["x"], a["dy"], a["y"], a["gamma"], a["beta"], a["mean"], a["rstd"], a["relu"], dx, dres, dg, db)

    def _op_bn_stats(self, call, a, live, out):
        scale, shift, mean, rstd = out
        call["family"] = "bn_stats"
        self.bn_stats(call, a["x"], a["gamma"], a["beta"], a["running_mean"], a["running_var"], live["running_mean"],
                      live["running_var"], a["momentum"], a["eps"], scale, shift, mean, rstd)

    def _op_channel_sums(self, call, a, live, out):
        call["family"] = "channel_sums"
        self.channel_sums(call, a["x"], *out)
        self.sum_sources.append(out[0].detach().clone())

    def _op_maxpool3x3s2_fwd(self, call, a, live, out):
        call["family"] = "maxpool_fwd"
        self.maxpool_fwd(call, a["x"], *out)

    def _op_maxpool3x3s2_bwd(self, call, a, live, out):
        call.update(family="maxpool_bwd" + ("_add" if a["add"] is not None else ""))
        self.maxpool_bwd(call, a["dy"], a["idx"], a["in_hw"], a["add"], out)

    def _op_softmax_ce(self, call, a, live, out):
        call["family"] = "softmax_ce"
        self.softmax_ce(call, a["logits"], a["targets"], a["class_weights"], a["num_classes"], a["grad_scale"], out)

    def _op_scale_inplace(self, call, a, live, out):
        call["family"] = "scale_inplace"
        self.scale_inplace(call, a["x"], a["scale"], out)
        gs = float(a["scale"].reshape(-1)[0])
        call["scale"] = gs
        if out.dim() == 4:  # a gradient buffer on its way to the layer that produced the logits
            Cp = out.shape[-1]
            ref, mag = out.new_zeros(Cp, dtype=F64), out.new_zeros(Cp, dtype=F64)
            for b0, b1 in self._chunks(out.shape[0]):
                ref += out[b0:b1].to(F64).reshape(-1, Cp).sum(0)
                mag += a["x"][b0:b1].to(F64).abs().reshape(-1, Cp).sum(0) * abs(gs)
            self._scaled[out.data_ptr()] = {"shape": tuple(out.shape), "sums": ref, "abs_sums": mag, "scale": gs,
                                            "call": call["call"]}

    def _op_nchw_to_nhwc(self, call, a, live, out):
        call["family"] = "nchw_to_nhwc"
        self.nchw_to_nhwc(call, a["x"], out)

    def _op_nhwc_to_nchw(self, call, a, live, out):
        call["family"] = "nhwc_to_nchw"
        self.nhwc_to_nchw(call, a["x"], a["channels"], out)

    def _op_bilinear_fwd(self, call, a, live, out):
        call.update(family="bilinear_fwd", ratio=a["x"].shape[1] / out.shape[1])
        self.bilinear(call, a["x"], out, False)

    def _op_bilinear_bwd(self, call, a, live, out):
        call.update(family="bilinear_bwd", ratio=out.shape[1] / a["dy"].shape[1])
        self.bilinear(call, a["dy"], out, True)

    def _op_mean_stack(self, call, a, live, out):
        call["family"] = "mean_stack"
        self.mean_stack(call, list(a["xs"]), a["divisor"], out)

    def _op_u8_nchw_to_nhwc(self, call, a, live, out):
        call["family"] = "layout_norm"
        self.layout_norm(call, a["x"], a["mean"], a["std"], out)

    _op_raw_nchw_to_nhwc = _op_u8_nchw_to_nhwc

    def _op_d4_layout(self, call, a, live, out):
        call.update(family="d4_layout", codes=sorted(set(int(c) & 15 for c in a["codes"].tolist())))
        self.layout_norm(call, a["x"], a["mean"], a["std"], out, codes=a["codes"].tolist(), group=a["group"])

    def _op_d4_labels(self, call, a, live, out):
        call["family"] = "d4_labels"
        self.d4_labels(call, a["t"], a["codes"].tolist(), out)

    def _op_confusion_matrix_update(self, call, a, live, out):
        call["family"] = "confusion_matrix"
        self.confusion(call, a["counts"], live["counts"], a["pred"], a["target"])

    def _op_onehot_to_index(self, call, a, live, out):
        call["family"] = "onehot_to_index"
        self.onehot_to_index(call, a["onehot"], out)

    def _op_bn_eval_params(self, call, a, live, out):
        call["family"] = "bn_eval_params"
        self._fold_params = out
        self.bn_eval_params(call, a["gamma"], a["beta"], a["running_mean"], a["running_var"], a["eps"], *out)

    def _op_predict_u8(self, call, a, live, out):
        call.update(family="predict_u8", mode=a["mode"], crop=a["crop"])
        self.predict_u8(call, a["logits"], a["num_classes"], a["mode"], a["crop"], out)

    def _op_tta_accumulate_(self, call, a, live, out):
        call.update(family="tta_accumulate_", code=int(a["code"]), first=bool(a["first"]), crop=a["crop"])
        self.tta_accumulate(call, a["acc"], a["logits_nhwc"], a["num_classes"], a["code"], a["crop"], a["first"], out)

    @staticmethod
    def _tta_classes(a, live):
        k = a["num_classes"] if a["num_classes"] is not None else getattr(live["acc"], "_ffa_classes", None)
        if k is None:
            raise ValueError("accumulator without a class count")
        return int(k)

    def _op_tta_predict_u8(self, call, a, live, out):
        call.update(family="tta_predict_u8", mode=a["mode"], views=a["views"])
        self.tta_predict_u8(call, a["acc"], a["mode"], a["views"], self._tta_classes(a, live), out)

    def _op_tta_probabilities(self, call, a, live, out):
        call.update(family="tta_probabilities", views=a["views"])
        self.tta_probabilities(call, a["acc"], a["views"], self._tta_classes(a, live), out)

    # ---- the U-TAE branch ------------------------------------------------------------------------

    def _op_reflect_pad1(self, call, a, live, out):
        self.reflect_pad1(call, a["x"], out)

    def _op_reflect_pad1_bwd(self, call, a, live, out):
        self.reflect_pad1_bwd(call, a["dpad"], out)

    def _op_group_norm(self, call, a, live, out):
        call.update(relu=bool(a["relu"]), residual=a["residual"] is not None)
        self.group_norm(call, a["x"], a["gamma"], a["beta"], a["groups"], a["eps"], a["relu"], a["residual"], out)

    def _op_group_norm_seq(self, call, a, live, out):
        call.update(T=a["T"])
        self.group_norm(call, a["x"], a["gamma"], a["beta"], a["groups"], a["eps"], False, None, out, seq=(a["B"], a["T"]))

    def _op_group_norm_bwd(self, call, a, live, out):
        call.update(relu=bool(a["relu"]))
        self.group_norm_bwd(call, a["x"], a["dy"], a["gamma"], a["beta"], a["groups"], a["eps"], a["relu"], *out)

    def _op_group_norm_seq_bwd(self, call, a, live, out):
        call.update(T=a["T"])
        self.group_norm_bwd(call, a["x"], a["dy"], a["gamma"], a["beta"], a["groups"], a["eps"], False, *out,
                            seq=(a["B"], a["T"]))

    def _op_positional_encoding(self, call, a, live, out):
        self.positional_encoding(call, a["pos"], a["d"], a["repeat"], a["period"], out)

    def _op_add_rowvec_(self, call, a, live, out):
        self.add_rowvec(call, a["x"], a["vec"], out)

    def _op_detect_pad_images(self, call, a, live, out):
        self.detect_pad_images(call, a["x"], a["value"], out)

    def _op_mask_images_(self, call, a, live, out):
        call.update(value=float(a["value"]))
        self.mask_images(call, a["x"], a["pad"], a["value"], out)

    def _op_mul(self, call, a, live, out):
        self.mul(call, a["x"], a["m"], out)

    def _op_ltae_attention(self, call, a, live, out):
        call.update(T=a["T"])
        self.ltae_attention(call, a["k"], a["v"], a["Q"], a["pad"], None, a["B"], a["T"], *out)

    def _op_ltae_attention_train(self, call, a, live, out):
        call.update(T=a["T"], drop=a["drop"] is not None)
        self.ltae_attention(call, a["k"], a["v"], a["Q"], a["pad"], a["drop"], a["B"], a["T"], *out)

    def _op_ltae_attention_bwd(self, call, a, live, out):
        call.update(T=a["T"], drop=a["drop"] is not None, dattn_ext=a["dattn_ext"] is not None)
        self.ltae_attention_bwd(call, a["k"], a["v"], a["Q"], a["pad"], a["drop"], a["prob"], a["dout"], a["dattn_ext"],
                                a["B"], a["T"], *out)
        # what the aggregators sent back to the returned masks: dattn_ext must be the sum of the dattn of every
        # temporal_aggregate_bwd call of this backward pass (autograd adds them in f32, in some order)
        parts, self._dattn_parts = self._dattn_parts, []
        call["aggregators"] = len(parts)
        if parts or a["dattn_ext"] is not None:
            ext = a["dattn_ext"] if a["dattn_ext"] is not None else torch.zeros_like(a["prob"])
            r = sum(p.to(F64) for p in parts) if parts else torch.zeros_like(ext, dtype=F64)
            mag = sum(p.to(F64).abs() for p in parts) if parts else r
            self._add(call, _compare(ext, r, len(parts) * ulp_f32(mag), "dattn_ext = sum of the aggregators' dattn"))

    def _op_temporal_aggregate(self, call, a, live, out):
        self.temporal_aggregate(call, a["x"], a["attn"], a["pad"], a["B"], a["T"], a["use_pad"], out)

    def _op_temporal_aggregate_bwd(self, call, a, live, out):
        self.temporal_aggregate_bwd(call, a["x"], a["attn"], a["pad"], a["dout"], a["B"], a["T"], a["use_pad"], *out)
        self._dattn_parts.append(out[1].detach().clone())

    def _op_column_sums(self, call, a, live, out):
        self.column_sums(call, a["x"], out)
        src = out.detach().clone()
        self.sum_sources.append(src)
        self.sum_inputs[id(src)] = (call["call"], (live["x"].data_ptr(), tuple(live["x"].shape)))

    # ---- report --------------------------------------------------------------------------------

    def failures(self) -> List[Result]:
        return [r for r in self.results if not r.ok]

    def grad_orphans(self, named_parameters) -> List[str]:
        """names of the parameters whose gradient is not what a checked call produced.  A gradient is accounted for if

        * it IS the output of a checked call, bit for bit (dW, dgamma, dbeta, the loss sums of an upstream gradient 1);
        * (a) it is the dim=1 concatenation of checked conv_wgrad outputs that follow one another in call order (the
          weight of a fusion 1x1 conv: one wgrad per source);
        * (b) it is the bias gradient of a head whose dgrad call read a rescaled dlogits buffer: then it must pass
          head_bias_grad against the final contents of THAT buffer, whatever else it may equal;
        * it is a bias gradient cut from the front of a checked channel_sums / column_sums output, bit for bit; column
          sums count only if the tensor they summed was also an operand of a checked conv_wgrad call of the same
          backward node (WGRAD_WINDOW calls around it, while the tensor is alive and its address its own) -- the gradient
          of the layer's output, which its weight gradient is taken from --, not just any tensor of the right width;
        * it is the front of a checked dgamma / dbeta vector (a class-score layer stored at the logits pitch);
        * it is a Conv1d [O, I, 1] or Linear [O, I] weight's view of a checked 1x1 conv_wgrad output [O, I, 1, 1];
        * it is dQ [n_head, d_k] as ltae_attention_bwd returned it (a view of its column sums, checked there)."""
        by_shape = defaultdict(list)
        for _, t in self.grad_sources:
            by_shape[tuple(t.shape)].append(t)
        dws = [t for tag, t in self.grad_sources if tag == "dW"]
        orphans = []
        for name, p in named_parameters:
            if p.grad is None:
                continue
            g = p.grad.detach()
            mod, _, leaf = name.rpartition(".")
            if leaf == "bias" and mod in self.head_bias:
                h = self.head_bias[mod]
                res = self.head_bias_grad({"op": "head_bias_grad", "family": "head_bias_grad", "call": h["call"],
                                           "module": mod, "scale": h["scale"]}, h["sums"], h["abs_sums"], g)
                if not res.ok:
                    orphans.append(name)
                continue
            if any(torch.equal(g, t) for t in by_shape.get(tuple(g.shape), [])):
                continue
            if g.dim() == 4 and self._is_concat_of_wgrads(g, dws):
                continue
            if g.dim() == 1 and any(t.numel() >= g.numel() and torch.equal(g, t[:g.numel()]) and self._summed_a_wgrad_operand(t)
                                    for t in self.sum_sources):
                continue
            if g.dim() == 1 and any(t.dim() == 1 and t.numel() > g.numel() and torch.equal(g, t[:g.numel()])
                                    for tag, t in self.grad_sources if tag in ("dgamma", "dbeta")):
                continue
            if g.dim() in (2, 3) and g.numel() == g.shape[0] * g.shape[1] and any(
                    tuple(t.shape) == (g.shape[0], g.shape[1], 1, 1) and torch.equal(g.reshape(t.shape), t) for t in dws):
                continue
            orphans.append(name)
        return orphans

    WGRAD_WINDOW = (-4, 8)  # a node's wgrad calls come at most 4 calls before and 8 after the column sums of its bias

    def _summed_a_wgrad_operand(self, t) -> bool:
        src = self.sum_inputs.get(id(t))
        if src is None:  # channel_sums: the statistics pass of the layer's own output
            return True
        c, key = src
        lo, hi = self.WGRAD_WINDOW
        return any(k == key and lo <= w - c <= hi for w, k in self.wgrad_operands)

    @staticmethod
    def _is_concat_of_wgrads(g, dws) -> bool:
        O, I, kh, kw = g.shape
        for i in range(len(dws)):
            run, width = [], 0
            for t in dws[i:]:
                if t.shape[0] != O or tuple(t.shape[2:]) != (kh, kw) or width + t.shape[1] > I:
                    break
                run.append(t)
                width += t.shape[1]
                if width == I:
                    break
            if len(run) > 1 and width == I and torch.equal(g, torch.cat(run, dim=1)):
                return True
        return False

    def table(self) -> str:
        fam = defaultdict(lambda: {"calls": set(), "layouts": set(), "worst": 0.0, "checks": 0, "what": ""})
        for r in self.results:
            f = fam[r.get("family", r["op"])]
            f["calls"].add(r["call"])
            if r.get("layout"):
                f["layouts"].add(r["layout"])
            f["checks"] += 1
            if r["worst"] > f["worst"]:
                f["worst"], f["what"] = r["worst"], f"{r['what']} [{r.get('module') or ''}]"
        lines = [f"{'family':<24}{'calls':>6}{'checks':>8}  {'worst err/bound':>16}  {'layouts':<14}  worst check"]
        for k in sorted(fam):
            f = fam[k]
            lines.append(f"{k:<24}{len(f['calls']):>6}{f['checks']:>8}  {f['worst']:>16.4g}  "
                         f"{','.join(sorted(f['layouts'])):<14}  {f['what']}")
        lines.append(f"ambiguous ReLU masks (bn_bwd mode 2): {self.ambiguous[0]} of {self.ambiguous[1]} elements")
        for kind in sorted(self.open):
            n_open, n = self.open[kind]
            lines.append(f"{kind} values within {HALF_OPEN} of a half-integer (may differ by 1): {n_open} of {n} "
                         f"({n_open / max(n, 1):.4%}, cap {OPEN_MAX_SHARE:.0%} per call)")
        for op in sorted(self.ties):
            lines.append(f"{op}: {self.ties[op]} labels checked at an exact tie of the top two")
        return "\n".join(lines)
