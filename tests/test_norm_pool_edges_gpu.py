"""BatchNorm statistics / apply / backward, channel sums and the 3x3 s2 max-pool (csrc/norm_pool.hip) against float64 at
the channel and pixel counts where their index arithmetic changes.

Each GPU test calls one flairhip.ops wrapper and hands the call's inputs and outputs to the matching Checker method of
tests/insitu.py in mode "full" (the references and bounds of the in-situ step checks: REL, ulp_stored, AMBIG_REL,
AMBIG_MAX_FRACTION -- none loosened, nothing fitted to what the kernels return).  Inputs are quantised to the storage type
(f32 or bf16) first.

What the shapes reach (CG = C / 8 channel groups, PL = 256 / CG pixel lanes per block, U = 4 (bf16) or 2 (f32) vectors in
flight per thread, reduce_blocks = ceil(npix / (8 PL)) capped at 1024):
  C      CG   PL   idle lanes of channel_reduce_kernel   walk of bn_apply_kernel / bn_bwd_apply_kernel
  8       1  256     0                                   chunked (256 % CG == 0)
  24      3   85     1                                   grid stride, grid a multiple of 3
  40      5   51     1                                   grid stride, grid a multiple of 5
  96     12   21     4                                   grid stride, grid a multiple of 3
  1032  129    1   127                                   grid stride, grid a multiple of 129
  2040  255    1     1                                   grid stride, grid a multiple of 255
  2048  256    1     0                                   chunked
  pixel counts per C: 1 (var = 0, rstd = 1 / sqrt(eps), the running variance takes the biased value), 2, 7, 16 PL + 1 (three
  blocks, the last one with one pixel), 3 PL U - 1 and 3 PL U + 1 (the ok[u] tail guard on either side of a full iteration);
  at C = 2048 also 8184 (1023 blocks: the forward statistics walk a grid stride apart) and 8191 (1024 blocks: the saturated
  grid walks contiguous rows, with a ragged tail) -- 33 MB in bf16, the largest case of the file.
  ffa_bn_finalize / ffa_bn_bwd_partials are fed hand-made partial rows (float64 per-slab sums of the test's own tensor,
  rounded once to f32): 1, 1024 (the last count that is not folded), 1025 and 4099 rows (through partials_fold_kernel), and
  one ragged conv2d_bnbwd -> bn_bwd_partials case goes through the real epilogue.
Conditioning, per channel c (c % 8): 0 gamma = 0; 1 gamma < 0; 2 a spread of 1e-3 around 0; 3 mean 4, spread 0.5 (mean /
spread = 8, the most the recomputed ReLU mask of mode 2 takes below the cap on ambiguous masks); 5, in f32 and outside mode
2 only, mean 100 with a spread of 0.05 (the E[x^2] - mean^2 cancellation must stay inside t_v = REL * s2 / n); the others
mean 0.3, spread 1.7.  |beta| >= 0.05 so that a mask is not ambiguous by construction where xhat is 0 or +-1 (1 and 2
pixels).  For the raw_x finalize (sum g x - mean sum g) rstd the dgamma bound is stated in what the kernel sums:
Checker.bn_bwd(raw_x=True).
Max-pool: (H, W) in (1,1) (1,7) (2,2) (5,1) (9,70) at C = 8 and 64 (at 9 x 70 both Wo CG and W CG pass one block's 256
threads with a ragged rest), a channel of -inf (every window entirely -inf), a constant channel and values on a coarse grid
(ties: the first tap in row-major order must win -- checked on the index itself, next to Checker.maxpool_fwd), backward
with `add`.  No NaN: the checker's equality does not define it.
ffa_bn_bwd_fused (the grid-barrier kernel, off by default) is not exercised here; its test in tests/test_kernels_gpu.py
stays as it is.

The CPU tests of this module (unmarked) put an f32 torch emulation that sums in the kernels' grouping (thread walk, lane sum,
double finalize, f32 fold) through the same checker at the edge shapes (test_emulation_*: inside the bounds, ambiguity cap
met), and planted faults that must each be flagged (test_mutant_*).

One MI355X run of this module (138 GPU cases, 6.5 s): largest error as a fraction of its bound over all cases, per wrapper
output and storage type.  No case exceeded its bound and no kernel bug was found.
  wrapper (kernels)                                        output           f32     bf16
  bn_stats (channel_reduce_kernel<StatOp>,                 mean             0.023   0.004
            bn_finalize_kernel)                            rstd             0.563   0.595
                                                           scale            0.526   0.526
                                                           shift            0.521   0.092
                                                           running_mean     0.319   0.314
                                                           running_var      0.323   0.324
  channel_sums (channel_reduce_kernel<StatOp>,             sum              0.022   0.002
                bn_bwd_finalize_kernel)                    sum of squares   0.046   0.028
  bn_apply (bn_apply_kernel)                               y                0.008   0.499
  bn_bwd, relu mode 0 / 1 / 2                              dbeta            0.009   0.002
      (channel_reduce_kernel<BnBwdOp>,                     dgamma           0.012   0.011
       bn_bwd_finalize_kernel, bn_bwd_apply_kernel)        dx               0.009   0.499
                                                           dres (mode 1)    exact   exact
  _bn_finalize, 1 .. 4099 rows (partials_fold_kernel,      mean             0.006   0.004
                bn_finalize_kernel)                        rstd             0.075   0.081
                                                           scale            0.103   0.101
                                                           shift            0.008   0.005
                                                           running_mean     0.258   0.255
                                                           running_var      0.189   0.189
  bn_bwd_partials, 1 .. 4099 rows (partials_fold_kernel,   dbeta            0.000   0.000
      bn_bwd_finalize_kernel raw_x, bn_bwd_apply_kernel)   dgamma           0.001   0.000
                                                           dx               0.009   0.499
  conv2d_bnbwd -> bn_bwd_partials, ragged                  dy               0.018   0.495
      (conv_igemm epilogue)                                dbeta / dgamma   0.001   0.001
                                                           dx               0.007   0.498
  maxpool3x3s2_fwd (maxpool_fwd_kernel)                    y, idx           exact   exact
  maxpool3x3s2_bwd (maxpool_bwd_kernel)                    dx               0.008   0.499
bf16-stored outputs sit at 0.499: half a bf16 ulp of the output rounding, which the ulp_stored term grants in full.  rstd,
scale and the running buffers reach 0.3 to 0.6 where their bound is all but the f32 ulp of the value: one pixel (var = 0, so
t_v adds nothing) and the channels of spread 1e-3.  In f32 one pixel leaves var = f32(x^2) - x^2 in double, up to 2^-24 x^2
and not 0: inside t_v = REL * s2 / n, so rstd = 1 / sqrt(eps) and a running variance of exactly (1 - momentum) rv hold bit for
bit in bf16 only (the square of a bf16 number is an f32 number), which is what the tests assert.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from insitu import AMBIG_MAX_FRACTION, Checker

gpu = pytest.mark.gpu
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
EPS, MOM = 1e-5, 0.1
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # the eps the kernels receive
RSTD_AT_ZERO_VAR = float(torch.tensor(1.0 / math.sqrt(EPS32), dtype=torch.float32))
THREADS, MAX_PARTIALS, FOLD_ROWS = 256, 1024, 64  # FFA_EW_THREADS, FFA_MAX_PARTIALS, R of partials_fold_kernel
CHANNELS = (8, 24, 40, 96, 1032, 2040, 2048)
ROWS = (1, 1024, 1025, 4099)

_measured = {}  # (op, what, storage) -> largest error / bound


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (op, what, storage), frac in sorted(_measured.items()):
        print(f"\nMEASURED {op:16s} {what:16s} {storage:5s} {frac:6.3f} of the bound", end="")


def _name(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _geometry(C, dtype):
    """-> (CG, PL, U) of csrc/norm_pool.hip"""
    CG = C // 8
    return CG, THREADS // CG, 4 if dtype == BF16 else 2


def _reduce_blocks(npix, C):
    PL = THREADS // (C // 8)
    return max(1, min(MAX_PARTIALS, (npix + PL * 8 - 1) // (PL * 8)))


def _pixel_counts(C, dtype):
    _, PL, U = _geometry(C, dtype)
    counts = {1, 2, 7, PL * 8 * 2 + 1, PL * U * 3 - 1, PL * U * 3 + 1}
    if C == 2048:
        counts |= {8184, 8191}
    return sorted(counts)


def test_the_shapes_reach_the_branches_they_are_chosen_for():
    idle = {C: THREADS - (C // 8) * (THREADS // (C // 8)) for C in CHANNELS}
    assert idle == {8: 0, 24: 1, 40: 1, 96: 4, 1032: 127, 2040: 1, 2048: 0}
    assert [THREADS % (C // 8) == 0 for C in CHANNELS] == [True, False, False, False, False, False, True]
    assert _reduce_blocks(8184, 2048) == 1023 and _reduce_blocks(8191, 2048) == MAX_PARTIALS
    for dtype in (F32, BF16):
        for C in CHANNELS:
            _, PL, U = _geometry(C, dtype)
            n = _pixel_counts(C, dtype)
            assert any(v % (PL * U) == PL * U - 1 for v in n) and any(v % (PL * U) == 1 and v > 1 for v in n)
            assert any(_reduce_blocks(v, C) == 3 and v % (PL * 8) == 1 for v in n)


# --------------------------------------------------------------------------------------------------
# inputs

def _inputs(C, npix, dtype, seed, large_mean=False, device="cpu"):
    """x, dy [1, 1, npix, C] of the storage type, gamma, beta, running buffers (f32), conditioned as the docstring says"""
    g = torch.Generator(device=device).manual_seed(seed)

    def rn(*shape):
        return torch.randn(*shape, generator=g, device=device)

    def ru(*shape):
        return torch.rand(*shape, generator=g, device=device)

    k = torch.arange(C, device=device) % 8
    mu = torch.full((C,), 0.3, device=device)
    sd = torch.full((C,), 1.7, device=device)
    mu[k == 2], sd[k == 2] = 0.0, 1e-3
    mu[k == 3], sd[k == 3] = 4.0, 0.5
    if large_mean:
        assert dtype == F32, "bf16 quantises a spread of 0.05 around 100 away"
        mu[k == 5], sd[k == 5] = 100.0, 0.05
    x = (rn(1, 1, npix, C) * sd + mu).to(dtype)
    dy = rn(1, 1, npix, C).to(dtype)
    gamma = ru(C) + 0.5
    gamma[k == 0] = 0.0
    gamma[k == 1] = -(ru(int((k == 1).sum())) + 0.5)
    beta = (0.05 + 0.3 * ru(C)) * torch.where(ru(C) < 0.5, -1.0, 1.0)
    return {"x": x, "dy": dy, "gamma": gamma, "beta": beta, "rm0": rn(C) * 0.1, "rv0": ru(C) + 0.5,
            "res": rn(1, 1, npix, C).to(dtype), "C": C, "npix": npix, "dtype": dtype}


def _stats64(x, gamma, beta):
    """mean, rstd, scale, shift as f32 vectors: float64 statistics rounded once, the affine formed in f32 as the kernels
    form it (gamma * rstd, beta - mean * scale)"""
    C = x.shape[-1]
    v = x.to(F64).reshape(-1, C)
    mean = v.mean(0)
    var = ((v * v).mean(0) - mean * mean).clamp_min(0)
    mean, rstd = mean.float(), (1.0 / torch.sqrt(var + EPS)).float()
    scale = (gamma if gamma is not None else torch.ones_like(rstd)) * rstd
    shift = (beta if beta is not None else torch.zeros_like(rstd)) - mean * scale
    return mean, rstd, scale, shift


def _forward64(x, scale, shift, res, dtype):
    """y = relu(x * scale + shift + res) from float64, stored as dtype"""
    y = x.to(F64) * scale.to(F64) + shift.to(F64)
    if res is not None:
        y = y + res.to(F64)
    return y.clamp_min(0).to(dtype)


def _slab_rows(a, b, rows):
    """[npix, C] float64 addends -> partial rows [rows, 2, C] f32: pixel i belongs to slab i % rows; float64 sums per slab,
    rounded once"""
    npix, C = a.shape
    slab = torch.arange(npix, device=a.device) % rows
    out = torch.zeros(rows, 2, C, dtype=F64, device=a.device)
    out[:, 0].index_add_(0, slab, a)
    out[:, 1].index_add_(0, slab, b)
    return out.float().contiguous()


def _masked64(x, dy, scale, shift):
    """the mode-2 gradient in float64 from the kernel's f32 affine -> (g, g * x) as [npix, C]"""
    C = x.shape[-1]
    xc, dc = x.to(F64).reshape(-1, C), dy.to(F64).reshape(-1, C)
    gm = torch.where(xc * scale.to(F64) + shift.to(F64) > 0, dc, torch.zeros_like(dc))
    return gm, gm * xc


def _first_tap(x):
    """[B, Ho, Wo, C] window-local index of the first maximal tap (row-major) among the taps inside the image"""
    B, H, W, C = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    hp, wp = max(H + 2, 2 * Ho + 1), max(W + 2, 2 * Wo + 1)
    xp = F.pad(x.to(F64), (0, 0, 1, wp - W - 1, 1, hp - H - 1), value=float("-inf"))
    inside = F.pad(torch.ones((B, H, W, C), dtype=torch.bool, device=x.device), (0, 0, 1, wp - W - 1, 1, hp - H - 1))
    sl = [(r, s) for r in range(3) for s in range(3)]
    taps = torch.stack([xp[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r, s in sl])
    ok = torch.stack([inside[:, r:r + 2 * Ho - 1:2, s:s + 2 * Wo - 1:2] for r, s in sl])
    hit = ok & (taps == taps.max(0).values)
    return torch.argmax(hit.to(torch.int8), dim=0).to(torch.uint8)


def _pool_input(B, H, W, C, dtype, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    x = (torch.randn(B, H, W, C, generator=g, device=device) * 2).round() / 2  # a grid of 0.5: ties in most windows
    x[..., 1] = 0.5                     # equal values everywhere: the first tap inside the image
    x[..., 3] = float("-inf")           # every window of this channel is entirely -inf
    x[:, : (H + 1) // 2, : (W + 1) // 2, 5] = float("-inf")  # and a corner of this one
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randn(B, Ho, Wo, C, generator=g, device=device).to(dtype)
    add = torch.randn(B, H, W, C, generator=g, device=device).to(dtype)
    return x.to(dtype), dy, add


def _settle(ck, op, dtype, expect):
    """record the fractions, print the lines, assert every check passed and that `expect` checks were made"""
    for r in ck.results:
        key = (op, r["what"], _name(dtype))
        if math.isfinite(r["worst"]):
            _measured[key] = max(_measured.get(key, 0.0), r["worst"])
    bad = [f"{r.get('case')}: {r.line()}" for r in ck.results if not r.ok]
    worst = max(ck.results, key=lambda r: r["worst"])
    print(f"\n{op} {_name(dtype)}: {len(ck.results)} checks, worst {worst.get('case')}: {worst.line()}")
    assert len(ck.results) == expect, (len(ck.results), expect)
    assert not bad, bad[:20]
    assert ck.ambiguous[0] <= AMBIG_MAX_FRACTION * max(ck.ambiguous[1], 1), ck.ambiguous


def _call(op, C, npix, **kw):
    return dict({"op": op, "call": 0, "case": f"C={C} npix={npix} " + " ".join(f"{k}={v}" for k, v in kw.items())})


# --------------------------------------------------------------------------------------------------
# f32 emulation of the kernels' summation order (CPU)

def _thread_walk(npix, grid, PL, U, chunk):
    """[steps, grid * PL] pixel index each (block, lane) of channel_reduce_kernel adds at each step, -1 for none"""
    S = grid * PL
    b, pl = torch.arange(grid)[:, None], torch.arange(PL)[None, :]
    p = (b * PL * (U if chunk else 1) + pl).reshape(-1)
    us = PL if chunk else S
    steps = []
    while bool((p < npix).any()):
        for u in range(U):
            q = p + us * u
            steps.append(torch.where((p < npix) & (q < npix), q, torch.full_like(q, -1)))
        p = p + S * U
    return torch.stack(steps)


def _emu_reduce(a, b, C, dtype, op_chunks, mutant=None):
    """a, b [npix, C] f32 addends per pixel -> ws [blocks, 2, C] f32: every thread's chain of f32 additions in the
    kernel's pixel order, then the lanes of a block added in lane order"""
    npix = a.shape[0]
    _, PL, U = _geometry(C, dtype)
    grid = _reduce_blocks(npix, C)
    chunk = op_chunks or grid == MAX_PARTIALS
    seen = npix - npix % (PL * U) if mutant == "tail_dropped" else npix
    walk = _thread_walk(seen, grid, PL, U, chunk)
    if mutant is None:  # every pixel exactly once
        assert torch.equal(torch.sort(walk[walk >= 0]).values, torch.arange(npix))
    acc = torch.zeros(2, grid * PL, C)
    for row in walk:
        live = (row >= 0)[:, None]
        idx = row.clamp_min(0)
        acc[0] += torch.where(live, a[idx], torch.zeros(()))
        acc[1] += torch.where(live, b[idx], torch.zeros(()))
    acc = acc.reshape(2, grid, PL, C)
    ws = torch.zeros(2, grid, C)
    for q in range(PL):
        ws += acc[:, :, q]
    ws = ws.permute(1, 0, 2).contiguous()
    if mutant == "group_lost":  # channel group 2 of the second block never reaches its partial row
        assert grid >= 2
        ws[1, :, 16:24] = 0
    return ws


def _emu_fold(rows, mutant=None):
    """partials_fold_kernel above 1024 rows: 64 rows, row r the f32 sum of p = r, r + 64, ... taken by 32 lanes (lane l
    adds p = r + 64 (l + 32 m) in order of m), the lanes then added in lane order"""
    n = rows.shape[0]
    if n <= MAX_PARTIALS:
        return rows
    if mutant == "row_lost":
        rows = rows.clone()
        rows[n - 1] = 0
    per = FOLD_ROWS * 32
    padded = torch.zeros(((n + per - 1) // per * per,) + tuple(rows.shape[1:]))
    padded[:n] = rows
    v = padded.reshape(-1, 32, FOLD_ROWS, *rows.shape[1:])
    lanes = torch.zeros_like(v[0])
    for m in range(v.shape[0]):
        lanes += v[m]
    out = torch.zeros_like(lanes[0])
    for lane in range(32):
        out += lanes[lane]
    return out


def _emu_finalize(ws, n, gamma, beta, rm0, rv0, mutant=None):
    """bn_finalize_kernel: the partial rows added in double, f32 outputs -> dict"""
    s, q = ws[:, 0].double().sum(0), ws[:, 1].double().sum(0)
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + EPS32)).float()
    scale = (gamma if gamma is not None else torch.ones_like(rstd)) * rstd
    shift = (beta if beta is not None else torch.zeros_like(rstd)) - mean.float() * scale
    unbiased = var * n / (n - 1) if n > 1 and mutant != "biased_running_var" else var
    return {"mean": mean.float(), "rstd": rstd, "scale": scale, "shift": shift,
            "rm1": (1 - MOM) * rm0 + MOM * mean.float(), "rv1": (1 - MOM) * rv0 + MOM * unbiased.float()}


def _emu_apply(x, scale, shift, res, relu, mutant=None):
    C = x.shape[-1]
    if mutant == "group0_coefficients":
        scale, shift = scale[:8].repeat(C // 8), shift[:8].repeat(C // 8)
    y = x.float() * scale + shift
    if res is not None:
        y = y + res.float()
    return (y.clamp_min(0) if relu else y).to(x.dtype)


def _emu_masked(x, dy, y, scale, shift, mode):
    g = dy.float()
    if mode == 1:
        g = torch.where(y > 0, g, torch.zeros(()))
    elif mode == 2:
        g = torch.where(x.float() * scale + shift > 0, g, torch.zeros(()))
    return g


def _emu_bwd_finalize(ws, n, gamma, mean, rstd, raw_x=False, mutant=None):
    """bn_bwd_finalize_kernel -> dbeta, dgamma and the three apply coefficients"""
    s, q = ws[:, 0].double().sum(0), ws[:, 1].double().sum(0)
    if raw_x:
        q = (q - (0.0 if mutant == "raw_x_without_mean" else mean.double() * s)) * rstd.double()
    dbeta, dgamma = s.float(), q.float()
    inv = torch.tensor(1.0 / n, dtype=F32)
    kg = (gamma if gamma is not None else torch.ones_like(rstd)) * rstd
    kx = -kg * rstd * dgamma * inv
    k0 = -kg * dbeta * inv - kx * mean
    return dbeta, dgamma, (kg, kx, k0)


def _emu_bn_bwd(c, mode, st, want_dres):
    """ffa_bn_bwd in f32: BnBwdOp sums in the chunked walk, finalize, apply -> dx, dres, dgamma, dbeta"""
    x, C = c["x"], c["C"]
    y = c.get("y")
    g = _emu_masked(x, c["dy"], y, st["scale"], st["shift"], mode)
    xf = x.float()
    a = g.reshape(-1, C)
    b = (g * (xf - st["mean"]) * st["rstd"]).reshape(-1, C)
    ws = _emu_reduce(a, b, C, c["dtype"], True)
    dbeta, dgamma, (kg, kx, k0) = _emu_bwd_finalize(ws, c["npix"], c["gamma"], st["mean"], st["rstd"])
    dx = (kg * g + kx * xf + k0).to(x.dtype)
    return dx, (g.to(x.dtype) if want_dres else None), dgamma, dbeta


def _emu_stats(c, gamma="own", beta="own", mutant=None):
    C = c["C"]
    v = c["x"].float().reshape(-1, C)
    ws = _emu_reduce(v, v * v, C, c["dtype"], False, mutant)
    return _emu_finalize(ws, c["npix"], c["gamma"] if gamma == "own" else gamma, c["beta"] if beta == "own" else beta,
                         c["rm0"], c["rv0"], mutant)


def _check_stats(ck, call, c, st, gamma="own", beta="own"):
    ck.bn_stats(call, c["x"], c["gamma"] if gamma == "own" else gamma, c["beta"] if beta == "own" else beta, c["rm0"],
                c["rv0"], st["rm1"], st["rv1"], MOM, EPS, st["scale"], st["shift"], st["mean"], st["rstd"])


# (C, pixels): 1 x 1 x 1, 1 x 1 x 2, 1 x 3 x 5, 2 x 17 x 23, 3 x 13 x 29 and 2 x 9 x 7 maps, and the counts around a full iteration
EMU_SHAPES = [(8, 1), (8, 2), (24, 15), (40, 782), (2048, 1131), (96, 126), (24, 3 * 85 * 4 + 1), (24, 3 * 85 * 2 - 1),
              (96, 16 * 21 + 1), (2040, 17), (8, 4097)]


@DTYPES
@pytest.mark.parametrize("C,npix", EMU_SHAPES)
def test_emulation_stays_inside_the_bounds(C, npix, dtype):
    """statistics (with the large-mean channels in f32), channel sums, apply, and the backward in its three relu modes
    (mode 2 and bf16 with mean / spread <= 8), as the kernels group their sums"""
    c = _inputs(C, npix, dtype, seed=C + npix, large_mean=dtype == F32)
    ck = Checker("full", chunk=1)
    st = _emu_stats(c)
    _check_stats(ck, _call("bn_stats", C, npix), c, st)
    v = c["x"].float().reshape(-1, C)
    ws = _emu_reduce(v, v * v, C, dtype, False)
    ck.channel_sums(_call("channel_sums", C, npix), c["x"], ws[:, 0].double().sum(0).float(),
                    ws[:, 1].double().sum(0).float())
    for res, relu in ((None, False), (c["res"], True)):
        y = _emu_apply(c["x"], st["scale"], st["shift"], res, relu)
        ck.bn_apply(_call("bn_apply", C, npix, relu=relu), c["x"], st["scale"], st["shift"], res, relu, y)
    c["y"] = y
    for mode in (0, 1, 2):
        cm = c if mode != 2 else _inputs(C, npix, dtype, seed=C + npix)
        sm = st if mode != 2 else _emu_stats(cm)
        dx, dres, dgamma, dbeta = _emu_bn_bwd(cm, mode, sm, mode == 1)
        ck.bn_bwd(_call("bn_bwd", C, npix, mode=mode), cm["x"], cm["dy"], cm["y"] if mode == 1 else None, cm["gamma"],
                  cm["beta"], sm["mean"], sm["rstd"], mode > 0, dx, dres, dgamma, dbeta)
    bad = [f"{r.get('case')}: {r.line()}" for r in ck.results if not r.ok]
    assert not bad, bad
    assert ck.ambiguous[1] == c["x"].numel() and ck.ambiguous[0] <= AMBIG_MAX_FRACTION * ck.ambiguous[1], ck.ambiguous
    if npix == 1 and dtype == BF16:  # var = 0 exactly (the square of a bf16 value is an f32 number): rstd = 1 / sqrt(eps)
        assert torch.equal(st["rstd"], torch.full((C,), RSTD_AT_ZERO_VAR))  # and the running variance takes the biased 0
        assert torch.equal(st["rv1"], (1 - MOM) * c["rv0"] + MOM * torch.zeros(C))


def test_emulation_of_the_saturated_grid_stays_inside_the_bounds():
    """1024 blocks: the forward statistics leave the grid-stride order for contiguous rows (C = 1032: 127 idle lanes,
    one pixel lane), with the large-mean channels"""
    C, npix = 1032, 8191
    assert _reduce_blocks(npix, C) == MAX_PARTIALS and _reduce_blocks(npix - 7, C) == MAX_PARTIALS - 1
    for n in (npix, npix - 7):
        c = _inputs(C, n, F32, seed=3, large_mean=True)
        ck = Checker("full", chunk=1)
        _check_stats(ck, _call("bn_stats", C, n), c, _emu_stats(c))
        assert len(ck.results) == 6 and all(r.ok for r in ck.results), [r.line() for r in ck.results if not r.ok]


def _emu_partial_rows_case(rows, dtype, C=24, npix=4131, seed=9):
    c = _inputs(C, npix, dtype, seed=seed + rows)
    v = c["x"].to(F64).reshape(-1, C)
    mean, rstd, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
    gm, gx = _masked64(c["x"], c["dy"], scale, shift)
    c.update(part_fwd=_slab_rows(v, v * v, rows), part_bwd=_slab_rows(gm, gx, rows), mean=mean, rstd=rstd, scale=scale,
             shift=shift)
    return c


def _emu_partials(ck, c, rows, mutant=None):
    """_bn_finalize and bn_bwd_partials from the case's partial rows, emulated and checked"""
    C, npix = c["C"], c["npix"]
    st = _emu_finalize(_emu_fold(c["part_fwd"], mutant), npix, c["gamma"], c["beta"], c["rm0"], c["rv0"])
    _check_stats(ck, _call("bn_finalize", C, npix, rows=rows), c, st)
    dbeta, dgamma, (kg, kx, k0) = _emu_bwd_finalize(_emu_fold(c["part_bwd"], mutant), npix, c["gamma"], c["mean"],
                                                    c["rstd"], raw_x=True, mutant=mutant)
    g = _emu_masked(c["x"], c["dy"], None, c["scale"], c["shift"], 2)
    dx = (kg * g + kx * c["x"].float() + k0).to(c["dtype"])
    ck.bn_bwd(_call("bn_bwd_partials", C, npix, rows=rows), c["x"], c["dy"], None, c["gamma"], c["beta"], c["mean"],
              c["rstd"], True, dx, None, dgamma, dbeta, raw_x=True)


@DTYPES
@pytest.mark.parametrize("rows", ROWS)
def test_emulation_from_partial_rows_stays_inside_the_bounds(rows, dtype):
    c = _emu_partial_rows_case(rows, dtype)
    ck = Checker("full", chunk=1)
    _emu_partials(ck, c, rows)
    assert len(ck.results) == 9 and all(r.ok for r in ck.results), [r.line() for r in ck.results if not r.ok]
    assert ck.ambiguous[0] <= AMBIG_MAX_FRACTION * ck.ambiguous[1]


def _flagged(ck, *whats):
    bad = {r["what"] for r in ck.results if not r.ok}
    assert bad, "the planted fault passed: " + "; ".join(r.line() for r in ck.results)
    assert set(whats) <= bad, (bad, [r.line() for r in ck.results])


@DTYPES
def test_mutant_channel_group_left_out_of_the_reduction(dtype):
    C, npix = 24, 3 * 85 * 8 + 1
    c = _inputs(C, npix, dtype, seed=1)
    ck = Checker("full", chunk=1)
    _check_stats(ck, _call("bn_stats", C, npix), c, _emu_stats(c, mutant="group_lost"))
    _flagged(ck, "mean", "running_mean")
    assert all(r["where"][0] >= 16 for r in ck.results if not r.ok), "only channel group 2 lost anything"


@DTYPES
def test_mutant_ragged_tail_dropped(dtype):
    C = 24
    _, PL, U = _geometry(C, dtype)
    npix = 3 * PL * U + 1  # one pixel past three full iterations
    c = _inputs(C, npix, dtype, seed=2)
    ck = Checker("full", chunk=1)
    _check_stats(ck, _call("bn_stats", C, npix), c, _emu_stats(c, mutant="tail_dropped"))
    _flagged(ck, "mean")


@DTYPES
def test_mutant_folded_partial_row_lost(dtype):
    c = _emu_partial_rows_case(1025, dtype)
    ck = Checker("full", chunk=1)
    _emu_partials(ck, c, 1025, mutant="row_lost")
    _flagged(ck, "mean", "dbeta", "dgamma")


@DTYPES
def test_mutant_raw_x_finalize_without_the_mean_term(dtype):
    c = _emu_partial_rows_case(1024, dtype)
    ck = Checker("full", chunk=1)
    _emu_partials(ck, c, 1024, mutant="raw_x_without_mean")
    _flagged(ck, "dgamma", "dx")
    assert all(r.ok for r in ck.results if r["what"] in ("dbeta", "mean", "rstd")), "nothing else was touched"


@DTYPES
def test_mutant_apply_with_the_coefficients_of_channel_group_0(dtype):
    C, npix = 24, 15
    c = _inputs(C, npix, dtype, seed=4)
    st = _emu_stats(c)
    ck = Checker("full", chunk=1)
    ck.bn_apply(_call("bn_apply", C, npix), c["x"], st["scale"], st["shift"], None, False,
                _emu_apply(c["x"], st["scale"], st["shift"], None, False, mutant="group0_coefficients"))
    _flagged(ck, "y")
    assert ck.results[0]["where"][-1] >= 8, "channel group 0 itself is right"


@DTYPES
def test_mutant_biased_variance_in_the_running_buffer(dtype):
    C, npix = 40, 7
    c = _inputs(C, npix, dtype, seed=5)
    ck = Checker("full", chunk=1)
    _check_stats(ck, _call("bn_stats", C, npix), c, _emu_stats(c, mutant="biased_running_var"))
    assert {r["what"] for r in ck.results if not r.ok} == {"running_var"}, [r.line() for r in ck.results]


# --------------------------------------------------------------------------------------------------
# the kernels (GPU)

CD = pytest.mark.parametrize("C", CHANNELS)


@gpu
@DTYPES
@CD
def test_bn_stats(cuda, C, dtype):
    """ffa_bn_stats with its running buffers at every pixel count; once without gamma / beta, once without buffers"""
    from flairhip import ops
    ck = Checker("full", chunk=1)
    counts = _pixel_counts(C, dtype)
    for npix in counts:
        c = _inputs(C, npix, dtype, seed=C + npix, large_mean=dtype == F32, device=cuda)
        for variant in ("affine",) + (("plain", "no buffers") if npix in (1, counts[-1]) else ()):
            gamma, beta = (None, None) if variant == "plain" else (c["gamma"], c["beta"])
            rm, rv = (None, None) if variant == "no buffers" else (c["rm0"].clone(), c["rv0"].clone())
            scale, shift, mean, rstd = ops.bn_stats(c["x"], gamma, beta, rm, rv, MOM, EPS)
            torch.cuda.synchronize()
            ck.bn_stats(_call("bn_stats", C, npix, variant=variant), c["x"], gamma, beta, c["rm0"], c["rv0"], rm, rv,
                        MOM, EPS, scale, shift, mean, rstd)
            if npix == 1 and variant == "affine":
                assert torch.equal(mean, c["x"].float().reshape(C))
                if dtype == BF16:  # (in f32 the rounding of x * x leaves a variance of up to 2^-24 x^2: inside t_v)
                    assert torch.equal(rstd, torch.full_like(rstd, RSTD_AT_ZERO_VAR))
                    assert torch.equal(rv, (1 - MOM) * c["rv0"] + MOM * torch.zeros_like(rv))
    _settle(ck, "bn_stats", dtype, 6 * len(counts) + 2 * (6 + 4))


@gpu
@DTYPES
@CD
def test_channel_sums(cuda, C, dtype):
    from flairhip import ops
    ck = Checker("full", chunk=1)
    counts = _pixel_counts(C, dtype)
    for npix in counts:
        c = _inputs(C, npix, dtype, seed=C + npix + 1, large_mean=dtype == F32, device=cuda)
        s, q = ops.channel_sums(c["x"])
        torch.cuda.synchronize()
        ck.channel_sums(_call("channel_sums", C, npix), c["x"], s, q)
    _settle(ck, "channel_sums", dtype, 2 * len(counts))


@gpu
@DTYPES
@CD
def test_bn_apply(cuda, C, dtype):
    """with and without residual and ReLU; scale / shift from float64 statistics"""
    from flairhip import ops
    ck = Checker("full", chunk=1)
    counts = _pixel_counts(C, dtype)
    for npix in counts:
        c = _inputs(C, npix, dtype, seed=C + npix + 2, large_mean=dtype == F32, device=cuda)
        _, _, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
        for res, relu in ((None, False), (None, True), (c["res"], False), (c["res"], True)):
            y = ops.bn_apply(c["x"], scale, shift, res, relu)
            torch.cuda.synchronize()
            assert y.dtype == dtype and y.shape == c["x"].shape
            ck.bn_apply(_call("bn_apply", C, npix, res=res is not None, relu=relu), c["x"], scale, shift, res, relu, y)
    _settle(ck, "bn_apply", dtype, 4 * len(counts))


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@DTYPES
@CD
def test_bn_bwd(cuda, C, dtype, mode):
    """relu mode 0, 1 (mask from the stored y of a residual block, with dres) and 2 (mask recomputed from x); saved mean /
    rstd from float64; at the last pixel count dgamma / dbeta go to slots inside a larger buffer (a gradient bucket)"""
    from flairhip import ops
    ck = Checker("full", chunk=1)
    counts = _pixel_counts(C, dtype)
    for npix in counts:
        c = _inputs(C, npix, dtype, seed=C + npix + 3 + mode, large_mean=dtype == F32 and mode != 2, device=cuda)
        mean, rstd, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
        y = _forward64(c["x"], scale, shift, c["res"], dtype) if mode == 1 else None
        slots = npix == counts[-1]
        bucket = torch.full((2 * C + 7,), 7.0, device=cuda)
        out = (bucket[3:3 + C], bucket[C + 4:2 * C + 4]) if slots else (None, None)
        dx, dres, dgamma, dbeta = ops.bn_bwd(c["x"], c["dy"], y, c["gamma"], c["beta"], mean, rstd, mode > 0, mode == 1,
                                             out_dgamma=out[0], out_dbeta=out[1])
        torch.cuda.synchronize()
        if slots:
            assert dgamma.data_ptr() == out[0].data_ptr() and dbeta.data_ptr() == out[1].data_ptr()
            keep = torch.ones_like(bucket, dtype=torch.bool)
            keep[3:3 + C] = keep[C + 4:2 * C + 4] = False
            assert bool((bucket[keep] == 7.0).all()), "the kernel wrote outside the two slots"
        assert (dres is not None) == (mode == 1)
        ck.bn_bwd(_call("bn_bwd", C, npix, mode=mode), c["x"], c["dy"], y, c["gamma"], c["beta"], mean, rstd, mode > 0,
                  dx, dres, dgamma, dbeta)
    _settle(ck, f"bn_bwd mode {mode}", dtype, (4 if mode == 1 else 3) * len(counts))


def _partial_rows_case(cuda, rows, C, dtype):
    npix = 4131  # 3 x 17 x 81: ragged against every PL * U, and at least one pixel in each of 4099 slabs
    c = _inputs(C, npix, dtype, seed=rows + C, device=cuda)
    v = c["x"].to(F64).reshape(-1, C)
    mean, rstd, scale, shift = _stats64(c["x"], c["gamma"], c["beta"])
    gm, gx = _masked64(c["x"], c["dy"], scale, shift)
    c.update(part_fwd=_slab_rows(v, v * v, rows), part_bwd=_slab_rows(gm, gx, rows), mean=mean, rstd=rstd)
    return c


@gpu
@DTYPES
@pytest.mark.parametrize("C", [24, 96])
@pytest.mark.parametrize("rows", ROWS)
def test_bn_finalize_from_partial_rows(cuda, rows, C, dtype):
    """ffa_bn_finalize on both sides of the fold at 1024 rows, without a large convolution in front"""
    from flairhip import ops
    c = _partial_rows_case(cuda, rows, C, dtype)
    rm, rv = c["rm0"].clone(), c["rv0"].clone()
    scale, shift, mean, rstd = ops._bn_finalize(c["part_fwd"], rows, c["npix"], C, c["gamma"], c["beta"], rm, rv, MOM, EPS)
    torch.cuda.synchronize()
    ck = Checker("full", chunk=1)
    ck.bn_stats(_call("bn_finalize", C, c["npix"], rows=rows), c["x"], c["gamma"], c["beta"], c["rm0"], c["rv0"], rm, rv,
                MOM, EPS, scale, shift, mean, rstd)
    _settle(ck, "bn_finalize", dtype, 6)


@gpu
@DTYPES
@pytest.mark.parametrize("C", [24, 96])
@pytest.mark.parametrize("rows", ROWS)
def test_bn_bwd_partials_from_partial_rows(cuda, rows, C, dtype):
    """ffa_bn_bwd_partials: (sum g, sum g x) rows with the mode-2 mask -> the raw_x finalize and the apply pass"""
    from flairhip import ops
    c = _partial_rows_case(cuda, rows, C, dtype)
    dx, dgamma, dbeta = ops.bn_bwd_partials(c["x"], c["dy"], c["part_bwd"], rows, c["gamma"], c["beta"], c["mean"],
                                            c["rstd"])
    torch.cuda.synchronize()
    ck = Checker("full", chunk=1)
    ck.bn_bwd(_call("bn_bwd_partials", C, c["npix"], rows=rows), c["x"], c["dy"], None, c["gamma"], c["beta"], c["mean"],
              c["rstd"], True, dx, None, dgamma, dbeta, raw_x=True)
    _settle(ck, "bn_bwd_partials", dtype, 3)


@gpu
@DTYPES
def test_bn_bwd_partials_from_the_conv_epilogue_at_a_ragged_shape(cuda, dtype):
    """conv2d_bnbwd (24 -> 40 channels, pitches 32 and 48, 3 x 13 x 29: no full tile row or column) leaves the partial
    rows; dy, dx, dgamma and dbeta all go to float64"""
    from flairhip import ops
    g = torch.Generator().manual_seed(17)
    B, H, W, cin, cout = 3, 13, 29, 24, 40
    cip, cop = ops.pad_channels(cin), ops.pad_channels(cout)

    def nhwc(t, pitch):
        return F.pad(t, (0, pitch - t.shape[-1])).to(dtype).to(cuda).contiguous()

    d2 = nhwc(torch.randn(B, H, W, cin, generator=g), cip)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to(dtype).float()
    pw = ops.pack_conv_weight(w.to(cuda), dtype, 1, cip, allow_ring=False, allow_thin=False)
    x1 = nhwc(torch.randn(B, H, W, cout, generator=g) * 0.5 + 4.0 * (torch.arange(cout) % 8 == 3), cop)
    gamma = (torch.rand(cop, generator=g) + 0.5).to(cuda)
    gamma[0], gamma[1] = 0.0, -0.7
    beta = ((0.05 + 0.3 * torch.rand(cop, generator=g)) * torch.where(torch.rand(cop, generator=g) < 0.5, -1.0, 1.0)).to(cuda)
    mean, rstd, scale, shift = _stats64(x1, gamma, beta)
    dy, part, rows = ops.conv2d_bnbwd(d2, pw, 1, cop, x1, scale, shift)
    dx, dgamma, dbeta = ops.bn_bwd_partials(x1, dy, part, rows, gamma, beta, mean, rstd)
    torch.cuda.synchronize()
    assert rows > 1 and dy.shape == x1.shape
    ck = Checker("full", chunk=1)
    ck.conv_forward(_call("conv2d_bnbwd", cop, B * H * W), d2, w.to(cuda).to(F64), 1, 1, dy)
    ck.bn_bwd(_call("bn_bwd_partials", cop, B * H * W, rows=rows), x1, dy, None, gamma, beta, mean, rstd, True, dx, None,
              dgamma, dbeta, raw_x=True)
    _settle(ck, "conv2d_bnbwd", dtype, 2 + 3)


@gpu
@DTYPES
@pytest.mark.parametrize("C", [8, 64])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (2, 2), (5, 1), (9, 70)])
def test_maxpool(cuda, H, W, C, dtype):
    """forward (values, and the first maximal tap inside the image as the index) and backward with `add`"""
    from flairhip import ops
    B = 2
    x, dy, add = _pool_input(B, H, W, C, dtype, seed=H * 100 + W + C, device=cuda)
    y, idx = ops.maxpool3x3s2_fwd(x)
    dx = ops.maxpool3x3s2_bwd(dy, idx, (H, W), add)
    dx0 = ops.maxpool3x3s2_bwd(dy, idx, (H, W))
    torch.cuda.synchronize()
    assert bool(torch.isinf(y[..., 3]).all()) and bool((y[..., 1] == 0.5).all())
    want = _first_tap(x)
    assert torch.equal(idx, want), f"{int((idx != want).sum())} windows kept another tap than the first maximal one"
    ck = Checker("full", chunk=1)
    ck.maxpool_fwd(_call("maxpool_fwd", C, H * W), x, y, idx)
    ck.maxpool_bwd(_call("maxpool_bwd", C, H * W, add=True), dy, idx, (H, W), add, dx)
    ck.maxpool_bwd(_call("maxpool_bwd", C, H * W, add=False), dy, idx, (H, W), None, dx0)
    _settle(ck, "maxpool", dtype, 4)
