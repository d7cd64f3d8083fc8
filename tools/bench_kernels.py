#!/usr/bin/env python
"""Micro-benchmark of single libflairhip kernels on the layer shapes of the batch-32 U-Net step.

  python tools/bench_kernels.py                 # table: shape, us, TFLOP/s or GB/s
  python tools/bench_kernels.py --only conv128  # one shape, many launches (use under rocprofv3 --pmc)

Inputs are random (never zeros: DVFS), each kernel is timed with HIP events on the stream it runs on,
median of several batches of back-to-back launches.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flair-for-aigle_amd"))

import torch

from flairhip import ops

B = 32
# name, Cin, Cout, k, stride, pad, H (input), what
CONV_SHAPES = [
    ("conv64", 64, 64, 3, 1, 1, 128),
    ("conv128", 128, 128, 3, 1, 1, 64),
    ("conv256", 256, 256, 3, 1, 1, 32),
    ("conv512", 512, 512, 3, 1, 1, 16),
    ("dec0c1", 768, 256, 3, 1, 1, 32),
    ("dec1c1", 384, 128, 3, 1, 1, 64),
    ("dec2c1", 192, 64, 3, 1, 1, 128),
    ("dec3c1", 128, 32, 3, 1, 1, 256),
    ("dec3c2", 32, 32, 3, 1, 1, 256),
    ("dec4c1", 32, 16, 3, 1, 1, 512),
    ("dec4c2", 16, 16, 3, 1, 1, 512),
    ("head", 16, 19, 3, 1, 1, 512),
    ("l2down", 64, 128, 3, 2, 1, 128),
    ("stem", 5, 64, 7, 2, 3, 512),
]


def timeit(fn, iters=20, reps=7, warm_s=0.4):
    """median over `reps` batches of `iters` back-to-back launches, after `warm_s` seconds of the same launches (a
    fresh process starts at a low power state: the first batches read 15-20 % slow)"""
    import time
    fn()
    torch.cuda.synchronize()
    t0 = time.time()
    while time.time() - t0 < warm_s:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    best = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        best.append(s.elapsed_time(e) / iters * 1e3)
    best.sort()
    return best[len(best) // 2]


# name, C, H of the BatchNorm layers of the step (count per step in the comment)
BN_SHAPES = [
    ("bn_stem", 64, 256),    # 1
    ("bn_l1", 64, 128),      # 6 (+2 decoder)
    ("bn_l2", 128, 64),      # 9 (+2)
    ("bn_l3", 256, 32),      # 13 (+2)
    ("bn_l4", 512, 16),      # 7
    ("bn_d3", 32, 256),      # 2
    ("bn_d4", 16, 512),      # 2
]


def bench_bn(args):
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    print(f"{'shape':10s} {'kernel':10s} {'us':>9s} {'GB/s':>9s}")
    for name, C, H in BN_SHAPES:
        if args.only and args.only != name:
            continue
        x = torch.randn(B, H, H, C, device=dev).to(dt)
        dy = torch.randn(B, H, H, C, device=dev).to(dt)
        y = torch.empty_like(x)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        sc, sh, mean, rstd = ops.bn_stats(x, gamma, beta, rm, rv, 0.1, 1e-5)
        nb = x.numel() * 2
        runs = [
            ("stats", lambda: ops.bn_stats(x, gamma, beta, rm, rv, 0.1, 1e-5), nb),
            ("apply", lambda: ops.bn_apply(x, sc, sh, None, True, out=y), 2 * nb),
            ("apply+res", lambda: ops.bn_apply(x, sc, sh, dy, True, out=y), 3 * nb),
            ("bwd(m2)", lambda: ops.bn_bwd(x, dy, None, gamma, beta, mean, rstd, True, False), 5 * nb),
            ("bwd(m1,dr)", lambda: ops.bn_bwd(x, dy, y, gamma, beta, mean, rstd, True, True), 8 * nb),
        ]
        for kname, fn, nbytes in runs:
            us = timeit(fn, iters=args.iters)
            print(f"{name:10s} {kname:10s} {us:9.1f} {nbytes / us / 1e3:9.0f}")
    if args.only:
        return
    # the other streaming kernels of the step (algorithmic bytes)
    x = torch.randn(B, 256, 256, 64, device=dev).to(dt)
    yp, idx = ops.maxpool3x3s2_fwd(x)
    dyp = torch.randn_like(yp)
    add = torch.randn_like(x)
    xin = torch.randn(B, 5, 512, 512, device=dev)
    xu8 = torch.randint(0, 255, (B, 5, 512, 512), device=dev, dtype=torch.uint8)
    mu, sd = torch.full((5,), 110.0, device=dev), torch.full((5,), 50.0, device=dev)
    flip, rot = torch.full((B,), 3, dtype=torch.uint8, device=dev), torch.full((B,), 4, dtype=torch.uint8, device=dev)
    u8_bytes = xu8.numel() + B * 512 * 512 * 16 * 2
    logits = torch.randn(B, 512, 512, 32, device=dev).to(dt)
    tgt = torch.randint(0, 19, (B, 512, 512), device=dev, dtype=torch.uint8)
    cw = torch.tensor([1.0] * 15 + [0.0] * 4, device=dev)
    nb = x.numel() * 2
    runs = [
        ("maxpool", "fwd", lambda: ops.maxpool3x3s2_fwd(x), nb + nb // 4 + nb // 8),
        ("maxpool", "bwd+add", lambda: ops.maxpool3x3s2_bwd(dyp, idx, (256, 256), add), 2 * nb + nb // 4 + nb // 8),
        ("layout", "nchw->nhwc", lambda: ops.nchw_to_nhwc(xin, dt), xin.numel() * 4 + B * 512 * 512 * 16 * 2),
        ("layout", "u8->nhwc", lambda: ops.u8_nchw_to_nhwc(xu8, dt, mu, sd, 16), u8_bytes),
        # the training augmentation in the same pass (csrc/augment.hip): both flips (even k), a rotation by 90 degrees
        ("layout", "d4 flips", lambda: ops.d4_layout(xu8, dt, flip, mu, sd, 16), u8_bytes),
        ("layout", "d4 rot90", lambda: ops.d4_layout(xu8, dt, rot, mu, sd, 16), u8_bytes),
        ("loss", "softmax_ce", lambda: ops.softmax_ce(logits, tgt, cw, 19, want_grad=True, want_pred=True),
         2 * logits.numel() * 2 + 2 * tgt.numel()),
    ]
    for name, kname, fn, nbytes in runs:
        us = timeit(fn, iters=args.iters)
        print(f"{name:10s} {kname:10s} {us:9.1f} {nbytes / us / 1e3:9.0f}")


def bench_layout(args):
    """ops.d4_layout (the layout pass with the training augmentation's gather) per code against the existing
    u8_nchw_to_nhwc on the flagship input, 32 x 5 x 512 x 512 uint8 -> bf16 pitch 16, same process: us, the ratio to the
    existing kernel and TB/s of algorithmic bytes (source read once, destination written once); then the label passes"""
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    x = torch.randint(0, 255, (B, 5, 512, 512), device=dev, dtype=torch.uint8)
    mu, sd = torch.full((5,), 110.0, device=dev), torch.full((5,), 50.0, device=dev)
    nbytes = x.numel() + B * 512 * 512 * 16 * 2
    base = timeit(lambda: ops.u8_nchw_to_nhwc(x, dt, mu, sd, 16), iters=args.iters)
    print(f"{'kernel':24s} {'us':>9s} {'ratio':>7s} {'TB/s':>7s}")
    print(f"{'u8_nchw_to_nhwc':24s} {base:9.1f} {1.0:7.2f} {nbytes / base / 1e6:7.2f}")
    for code in range(16):
        codes = torch.full((B,), code, dtype=torch.uint8, device=dev)
        us = timeit(lambda: ops.d4_layout(x, dt, codes, mu, sd, 16), iters=args.iters)
        name = f"d4_layout code {code:2d} (k={code >> 2}{' v' if code & 2 else ''}{' h' if code & 1 else ''})"
        print(f"{name:24s} {us:9.1f} {us / base:7.2f} {nbytes / us / 1e6:7.2f}")
    mixed = torch.arange(B, device=dev).to(torch.uint8) % 16
    us = timeit(lambda: ops.d4_layout(x, dt, mixed, mu, sd, 16), iters=args.iters)
    print(f"{'d4_layout mixed codes':24s} {us:9.1f} {us / base:7.2f} {nbytes / us / 1e6:7.2f}")
    tgt = torch.randint(0, 19, (B, 512, 512), device=dev, dtype=torch.uint8)
    onehot = torch.nn.functional.one_hot(tgt.long(), 19).permute(0, 3, 1, 2).float().contiguous()
    base = timeit(lambda: ops.onehot_to_index(onehot), iters=args.iters)
    print(f"{'onehot_to_index':24s} {base:9.1f} {1.0:7.2f} {(onehot.numel() * 4 + tgt.numel()) / base / 1e6:7.2f}")
    for label, codes in (("even k", torch.full((B,), 3, dtype=torch.uint8, device=dev)),
                         ("odd k", torch.full((B,), 4, dtype=torch.uint8, device=dev))):
        us = timeit(lambda: ops.d4_onehot_to_index(onehot, codes), iters=args.iters)
        print(f"{'d4_onehot_to_index ' + label:24s} {us:9.1f} {us / base:7.2f} "
              f"{(onehot.numel() * 4 + tgt.numel()) / us / 1e6:7.2f}")
        us = timeit(lambda: ops.d4_labels(tgt, codes), iters=args.iters)
        print(f"{'d4_labels ' + label:24s} {us:9.1f} {'':>7s} {2 * tgt.numel() / us / 1e6:7.2f}")


def bench_gather(args):
    """ops.gather_layout / ops.gather_labels (a batch gathered from a device-resident sample store, csrc/sample_gather.hip)
    against ops.d4_layout / ops.d4_labels at the same shape in the same process: a store of 4 * B patches of 5 x 512 x 512
    uint8, a batch of B random indices -> bf16 pitch 16; then a 2-band float32 DEM with the elevation difference"""
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    N = 4 * B
    store = torch.randint(0, 255, (N, 5, 512, 512), device=dev, dtype=torch.uint8)
    index = torch.randperm(N, device=dev)[:B].to(torch.int32)
    x = store[index.long()].contiguous()
    mu, sd = torch.full((5,), 110.0, device=dev), torch.full((5,), 50.0, device=dev)
    nbytes = x.numel() + B * 512 * 512 * 16 * 2
    print(f"{'kernel':32s} {'us':>9s} {'ratio':>7s} {'TB/s':>7s}")
    for label, codes in (("code 0", torch.zeros(B, dtype=torch.uint8, device=dev)),
                         ("mixed codes", torch.arange(B, device=dev).to(torch.uint8) % 16)):
        base = timeit(lambda: ops.d4_layout(x, dt, codes, mu, sd, 16), iters=args.iters)
        us = timeit(lambda: ops.gather_layout(store, index, dt, codes, mu, sd, 16), iters=args.iters)
        print(f"{'d4_layout ' + label:32s} {base:9.1f} {1.0:7.2f} {nbytes / base / 1e6:7.2f}")
        print(f"{'gather_layout ' + label:32s} {us:9.1f} {us / base:7.2f} {nbytes / us / 1e6:7.2f}")
    lstore = torch.randint(0, 24, (N, 512, 512), device=dev, dtype=torch.uint8)
    t = lstore[index.long()].contiguous()
    codes = torch.arange(B, device=dev).to(torch.uint8) % 16
    base = timeit(lambda: ops.d4_labels(t, codes), iters=args.iters)
    us = timeit(lambda: ops.gather_labels(lstore, index, 19, codes), iters=args.iters)
    print(f"{'d4_labels mixed codes':32s} {base:9.1f} {1.0:7.2f} {2 * t.numel() / base / 1e6:7.2f}")
    print(f"{'gather_labels mixed codes':32s} {us:9.1f} {us / base:7.2f} {2 * t.numel() / us / 1e6:7.2f}")
    dem = torch.randn(N, 2, 512, 512, device=dev)
    m1, s1 = torch.full((1,), 9.5, device=dev), torch.full((1,), 7.25, device=dev)
    db = B * 2 * 512 * 512 * 4 + B * 512 * 512 * 16 * 2
    us = timeit(lambda: ops.gather_layout(dem, index, dt, codes, m1, s1, 16, elevation=ops.ELEV_DIFF), iters=args.iters)
    print(f"{'gather_layout DEM z0 - z1':32s} {us:9.1f} {'':>7s} {db / us / 1e6:7.2f}")


def bench_series(args):
    """ops.gather_series (the padded U-TAE batch and its pad flags from a ragged series store, csrc/series_gather.hip)
    against the pair it replaces on the streamed path, ops.d4_layout(group=T) + ops.detect_pad_images on the same
    padded f32 batch, in the same process: B samples of 10 bands x 10 x 10 uint16 -> bf16 pitch 16, every series T
    dates long (T = 12: monthly averages) and of ragged lengths up to T = 40.  Three medians each: the spread."""
    import numpy as np
    from flairhip.sample_store import SeriesStore
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    r = np.random.RandomState(0)
    print(f"{'kernel':44s} {'us (3 medians)':>24s} {'ratio':>7s}")
    for T, lengths in ((12, [12] * (4 * B)), (40, list(r.randint(20, 41, 4 * B - 1)) + [40])):
        N, D = len(lengths), int(sum(lengths))
        st = SeriesStore(N, D, (10, 10, 10), np.uint16, device=dev)
        st.fill(0, r.randint(1, 10000, (D, 10, 10, 10)).astype(np.uint16), np.zeros(D), lengths)
        index = torch.from_numpy(np.concatenate([[N - 1], r.permutation(N - 1)[:B - 1]]).astype(np.int32)).to(dev)
        codes = torch.arange(B, device=dev).to(torch.uint8) % 16
        nhwc, _ = ops.gather_series(st, index, T, torch.float32, None, 16)
        x = nhwc[..., :10].permute(0, 3, 1, 2).contiguous()  # the padded f32 batch [B*T, 10, 10, 10]
        want = ops.d4_layout(x, dt, codes, cp=16, group=T)
        got, pad = ops.gather_series(st, index, T, dt, codes, 16)
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(pad, ops.detect_pad_images(x, 0.0))

        def pair():
            ops.d4_layout(x, dt, codes, cp=16, group=T)
            ops.detect_pad_images(x, 0.0)

        rows = {"d4_layout(group=T)": lambda: ops.d4_layout(x, dt, codes, cp=16, group=T),
                "detect_pad_images": lambda: ops.detect_pad_images(x, 0.0), "the pair": pair,
                "gather_series": lambda: ops.gather_series(st, index, T, dt, codes, 16)}
        us = {k: sorted(timeit(fn, iters=args.iters) for _ in range(3)) for k, fn in rows.items()}
        for k, v in us.items():
            text = " ".join(f"{t:7.1f}" for t in v)
            print(f"{k + f' B={B} T={T} ({B * T} images)':44s} {text:>24s} {v[1] / us['the pair'][1]:7.2f}")


def bench_blas(args):
    """The equal-FLOP GEMM of every MFMA-bound conv shape (M = B*Ho*Wo pixels, N = Cout, K = Cin*k*k) through torch's
    matmul = hipBLASLt on this image, same box, random bf16 operands: what a tuned vendor GEMM reaches on these M/N/K,
    i.e. the ceiling the implicit-GEMM kernels are measured against (an im2col-free conv moves 1/9 of the A bytes, so
    it can be faster, but not by the MFMA schedule)."""
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    print(f"{'shape':10s} {'M':>8s} {'N':>5s} {'K':>6s} {'us':>9s} {'TFLOP/s':>9s}   layout")
    for name, cin, cout, k, stride, pad, H in CONV_SHAPES:
        if args.only and args.only != name:
            continue
        if cout < 64 or k != 3 or stride != 1:
            continue
        Ho = (H + 2 * pad - k) // stride + 1
        M, N, K = B * Ho * Ho, cout, cin * k * k
        a = torch.randn(M, K, device=dev).to(dt)
        w = torch.randn(N, K, device=dev).to(dt)
        wt = w.t().contiguous()
        for lay, fn in (("a[M,K] @ w[N,K]^T", lambda: torch.matmul(a, w.t())), ("a[M,K] @ w[K,N]", lambda: torch.matmul(a, wt))):
            us = timeit(fn, iters=args.iters)
            print(f"{name:10s} {M:8d} {N:5d} {K:6d} {us:9.1f} {2.0 * M * N * K / us / 1e6:9.1f}   {lay}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--blas", action="store_true", help="hipBLASLt (torch.matmul) on the equal-FLOP GEMM of each MFMA-bound conv shape")
    ap.add_argument("--kinds", default="fwd,dgrad,wgrad")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bn", action="store_true", help="BatchNorm kernels instead of the convolutions")
    ap.add_argument("--layout", nargs="?", const="d4", choices=("d4", "gather", "series"), default=None,
                    help="the input layout pass with and without the augmentation gather; 'gather': the sample-store "
                         "gather kernels against d4_layout / d4_labels at the same shape; 'series': gather_series "
                         "against d4_layout(group=T) + detect_pad_images on the same padded batch")
    ap.add_argument("--data", default="randn", choices=["randn", "relu", "zeros"],
                    help="activation values: randn (worst case for power), relu (post-ReLU: half zeros, no "
                         "negative values -- what the network's 3x3 convs actually read), zeros")
    args = ap.parse_args()
    if args.bn:
        return bench_bn(args)
    if args.layout:
        return {"gather": bench_gather, "series": bench_series}.get(args.layout, bench_layout)(args)
    if args.blas:
        return bench_blas(args)
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    kinds = args.kinds.split(",")
    print(f"{'shape':10s} {'kind':6s} {'us':>9s} {'TFLOP/s':>9s} {'GB/s(min traffic)':>18s}")
    for name, cin, cout, k, stride, pad, H in CONV_SHAPES:
        if args.only and args.only != name:
            continue
        cip = ops.pad_channels(cin)
        cop = 32 if cout == 19 else ops.pad_channels(cout)
        Ho = (H + 2 * pad - k) // stride + 1
        x = torch.randn(B, H, H, cip, device=dev)
        if args.data == "relu":
            x = x.relu()
        elif args.data == "zeros":
            x = x * 0
        x = x.to(dt)
        if cip > cin:
            x[..., cin:] = 0
        w = torch.randn(cout, cin, k, k, device=dev) / (cin * k * k) ** 0.5
        dy = torch.randn(B, Ho, Ho, cop, device=dev).to(dt)
        flops = 2.0 * B * Ho * Ho * cout * cin * k * k
        bytes_min = (x.numel() + dy.numel()) * 2
        pw = ops.pack_conv_weight(w, dt, stride, cip)
        pwt = ops.pack_conv_weight(w, dt, stride, cop, transpose=True) if name != "stem" else None
        out = torch.empty(B, Ho, Ho, cop, device=dev, dtype=dt)
        dx = torch.empty(B, H, H, cip, device=dev, dtype=dt)
        dw = torch.empty(cout, cin, k, k, device=dev)
        stats = torch.empty(ops.conv_stat_rows(B, Ho, Ho, pw) * 2 * cop, device=dev)
        runs = {
            "fwd": lambda: ops.conv2d(x, pw, pad, cop, out=out),
            "fwdst": lambda: ops.conv2d(x, pw, pad, cop, out=out, stats=stats),  # + BatchNorm statistics epilogue
            "dgrad": lambda: ops.conv2d(dy, pwt, k - 1 - pad, cip, dil=stride, out_hw=(H, H), out=dx),
            "wgrad": lambda: ops.conv_wgrad(x, dy, cout, cin, k, k, stride, pad, out=dw),
        }
        for kind in kinds:
            if kind == "dgrad" and name == "stem":
                continue
            us = timeit(runs[kind], iters=args.iters)
            print(f"{name:10s} {kind:6s} {us:9.1f} {flops / us / 1e6:9.1f} {bytes_min / us / 1e3:18.0f}")


if __name__ == "__main__":
    main()
