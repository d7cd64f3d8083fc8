"""Zonal-statistics timings on synthetic class maps (GPU required).

    python tools/bench_zone_stats.py [--sizes 5000 16384] [--grids 100 316] [--reps 3] [--baseline-zones 100]

Map: a blocky 19-class map (64-pixel blocks, 2 % label noise) with a random uint8 confidence plane, made on the device.
Zone sets per size: "one" (a single box over the whole raster) and a g x g jittered parcel grid for every g of --grids
(quads over shared jittered vertices: the parcels tile the raster and reach past its borders).  One JSON line per
(size, zone set):
  * "total_ms": ffa_zone_stats_u8 with confidence, hip events around the call, best of --reps after a warm-up, tables
    resident on the device;
  * "rasterise_ms": the same call with a work list of one chunk -- spans, toggles and row scan run in full, the
    tabulation touches one chunk -- and "tabulate_ms" = total_ms - rasterise_ms, a difference, not an event pair;
  * "ops_ms": the whole ops.zone_class_stats call (windows, offsets and chunks in numpy, uploads, kernels, a final
    synchronise), wall clock, best of --reps; "plan_ms": its numpy part alone;
  * "workspace_bytes", "plane_words", "chunks", "vertices";
  * the byte floor: H W class bytes + H W confidence bytes + 4 bytes per plane word (read once by the tabulation;
    the rasteriser's clear, toggles and scan are not in it), and "floor_ms" = that at the 8 TB/s HBM specification;
  * the yardstick, the only route before this kernel: ops.rasterize_zone + a masked torch.bincount per zone, wall clock
    with a synchronise, over the first --baseline-zones zones ("per_zone_baseline_ms"), and "baseline_scaled_ms" = that
    times Z / zones timed.  The scaled figure is an extrapolation, not a measurement.
The counts are checked against the map on the way: the single zone and the parcel grids must count every pixel once.

    python tools/bench_zone_stats.py --change [--sizes 5000 16384] [--grids 100 316] [--reps 3]

times land-cover change instead.  The *before* map is the map with a tenth of its 64-pixel
blocks redrawn.  One JSON line per (size, zone set), both calls on the same resident tables, rasters and workspace in
the same process, hip events, best of --reps after a warm-up:
  * "change_ms": ffa_zone_change_u8 with confidence; "stats_ms": ffa_zone_stats_u8 with confidence on the *after*
    raster; "ratio" = change_ms / stats_ms.  The two build identical planes; the new call reads 3 bytes per member pixel
    against 2 and keeps (K + 1)^2 entries per wave against K + 1;
and one line per size for ffa_change_code_u8: "code_ms", "bytes_per_s" over the byte floor 3 H W (two bytes read, one
written per pixel) and its share of the 8 TB/s HBM specification.  Run one process per size.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flair-for-aigle_amd")]

HBM_BYTES_PER_S = 8.0e12
K = 19


def blocky_map(n: int, dev, seed: int = 0):
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    k = n // 64 + 1
    seeds = torch.randint(0, K, (k, k), dtype=torch.uint8, device=dev, generator=g)
    cls = seeds.repeat_interleave(64, 0).repeat_interleave(64, 1)[:n, :n].contiguous()
    noise = torch.rand((n, n), device=dev, generator=g) < 0.02
    cls[noise] = torch.randint(0, K, (int(noise.sum()),), dtype=torch.uint8, device=dev, generator=g)
    conf = torch.randint(0, 256, (n, n), dtype=torch.uint8, device=dev, generator=g)
    return cls, conf


def parcel_grid(n: int, g: int, seed: int = 0):
    """g x g quads over shared jittered vertices; the jitter stays below a third of a cell, so the quads stay simple"""
    rng = np.random.default_rng(seed)
    cell = (n + 12.0) / g
    X, Y = np.meshgrid(np.linspace(-6, n + 6, g + 1), np.linspace(-6, n + 6, g + 1))
    jx, jy = rng.uniform(-0.3 * cell, 0.3 * cell, X.shape), rng.uniform(-0.3 * cell, 0.3 * cell, Y.shape)
    jx[:, [0, -1]] = 0.0  # the outline stays outside the raster: the parcels cover every pixel
    jy[[0, -1], :] = 0.0
    X, Y = X + jx, Y + jy
    P = np.stack([X, Y], axis=2)
    quads = np.stack([P[:-1, :-1], P[:-1, 1:], P[1:, 1:], P[1:, :-1]], axis=2).reshape(g * g, 4, 2)
    return [[q] for q in quads]


def device_call(cls, conf, zones, reps: int) -> dict:
    """hip-event times of ffa_zone_stats_u8 on resident tables: the whole call, and the call with one chunk"""
    import torch
    from flairhip import lib as L
    from flairhip import ops
    lib = L.load()
    H, W = cls.shape
    dev = cls.device
    t0 = time.perf_counter()
    xy, ro, zro = ops.zone_stats_flatten(zones)
    win = ops.zone_stats_windows(xy, ro, zro, H, W)
    offsets, plane_words, scan_starts, chunks = ops.zone_stats_plan(win)
    plan_ms = (time.perf_counter() - t0) * 1e3
    Z = len(zones)
    nbytes = int(lib.ffa_zone_stats_workspace_bytes(len(xy), plane_words, len(chunks)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, ro, zro, win, offsets, scan_starts, chunks)]
    counts = torch.empty((Z, K + 1), dtype=torch.int64, device=dev)
    sums = torch.empty((Z, K + 1), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(n_chunks):
        L.check(lib.ffa_zone_stats_u8(cls.data_ptr(), conf.data_ptr(), H, W, K, d[0].data_ptr(), len(xy),
                                      d[1].data_ptr(), len(ro) - 1, d[2].data_ptr(), Z, d[3].data_ptr(),
                                      d[4].data_ptr(), plane_words, d[5].data_ptr(), int(scan_starts[-1]),
                                      d[6].data_ptr(), n_chunks, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                      nbytes, st))

    def timed(n_chunks):
        best = []
        for rep in range(reps + 1):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            call(n_chunks)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                best.append(e0.elapsed_time(e1))
        return best

    raster = timed(1)
    total = timed(len(chunks))  # last: counts and sums hold the full result
    floor = 2 * H * W + 4 * plane_words
    res = {"zones": Z, "vertices": len(xy), "plane_words": plane_words, "chunks": len(chunks), "workspace_bytes": nbytes,
           "plan_ms": round(plan_ms, 2), "total_ms": round(min(total), 4), "total_ms_all": [round(v, 4) for v in total],
           "rasterise_ms": round(min(raster), 4), "tabulate_ms": round(min(total) - min(raster), 4),
           "floor_bytes": floor, "floor_ms": round(floor / HBM_BYTES_PER_S * 1e3, 4)}
    res["tabulate_fraction_of_floor"] = round(res["floor_ms"] / max(res["tabulate_ms"], 1e-9), 4)
    return res, counts, sums


def best_ms(fn, reps: int) -> float:
    """hip-event time of fn(), the best of ``reps`` after one warm-up call"""
    import torch
    times = []
    for rep in range(reps + 1):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if rep:
            times.append(e0.elapsed_time(e1))
    return min(times)


def redrawn_blocks(cls, share: float = 0.1, seed: int = 1):
    """the *before* map of --change: ``cls`` with this share of its 64-pixel blocks taken from another blocky map"""
    import torch
    n, dev = cls.shape[0], cls.device
    other, _ = blocky_map(n, dev, seed=seed + 100)
    g = torch.Generator(device=dev).manual_seed(seed)
    k = n // 64 + 1
    pick = torch.rand((k, k), device=dev, generator=g) < share
    pick = pick.repeat_interleave(64, 0).repeat_interleave(64, 1)[:n, :n]
    return torch.where(pick, other, cls).contiguous()


def change_call(before, cls, conf, zones, reps: int):
    """ffa_zone_change_u8 beside ffa_zone_stats_u8 (both with confidence) on the same tables, rasters and workspace"""
    import torch
    from flairhip import lib as L
    from flairhip import ops
    lib = L.load()
    H, W = cls.shape
    dev = cls.device
    xy, ro, zro = ops.zone_stats_flatten(zones)
    win = ops.zone_stats_windows(xy, ro, zro, H, W)
    offsets, plane_words, scan_starts, chunks = ops.zone_stats_plan(win)
    Z = len(zones)
    nbytes = int(lib.ffa_zone_stats_workspace_bytes(len(xy), plane_words, len(chunks)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    d = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, ro, zro, win, offsets, scan_starts, chunks)]
    c1, s1 = (torch.empty((Z, K + 1), dtype=torch.int64, device=dev) for _ in range(2))
    c2, s2 = (torch.empty((Z, K + 1, K + 1), dtype=torch.int64, device=dev) for _ in range(2))
    st = torch.cuda.current_stream().cuda_stream
    tables = (d[0].data_ptr(), len(xy), d[1].data_ptr(), len(ro) - 1, d[2].data_ptr(), Z, d[3].data_ptr(),
              d[4].data_ptr(), plane_words, d[5].data_ptr(), int(scan_starts[-1]), d[6].data_ptr(), len(chunks))

    def stats():
        L.check(lib.ffa_zone_stats_u8(cls.data_ptr(), conf.data_ptr(), H, W, K, *tables, c1.data_ptr(), s1.data_ptr(),
                                      ws.data_ptr(), nbytes, st))

    def change():
        L.check(lib.ffa_zone_change_u8(before.data_ptr(), cls.data_ptr(), conf.data_ptr(), H, W, K, *tables,
                                       c2.data_ptr(), s2.data_ptr(), ws.data_ptr(), nbytes, st))

    stats_ms = best_ms(stats, reps)
    change_ms = best_ms(change, reps)
    # the marginal over the before classes is the existing kernel's table of the after raster
    assert torch.equal(c2.sum(1), c1) and torch.equal(s2.sum(1), s1)
    return {"zones": Z, "plane_words": plane_words, "chunks": len(chunks), "change_ms": round(change_ms, 4),
            "stats_ms": round(stats_ms, 4), "ratio": round(change_ms / stats_ms, 3),
            "changed_pixels": int(c2.sum() - c2.diagonal(dim1=1, dim2=2).sum()) if Z == 1 else None}


def code_call(before, cls, reps: int):
    """ffa_change_code_u8 over the whole raster with the default table (code k = became k)"""
    import torch
    from flairhip import lib as L
    lib = L.load()
    lut = torch.full((K + 1, K + 1), 255, dtype=torch.uint8)
    for k in range(K):
        lut[:K, k] = k
        lut[k, k] = 255
    lut = lut.to(cls.device)
    out = torch.empty_like(cls)
    n = cls.numel()
    st = torch.cuda.current_stream().cuda_stream
    ms = best_ms(lambda: L.check(lib.ffa_change_code_u8(before.data_ptr(), cls.data_ptr(), n, K, lut.data_ptr(),
                                                        out.data_ptr(), st)), reps)
    want = torch.where((before != cls) & (before < K) & (cls < K), cls, torch.full_like(cls, 255))
    assert torch.equal(out, want)
    rate = 3.0 * n / (ms * 1e-3)
    return {"code_ms": round(ms, 4), "floor_bytes": 3 * n, "bytes_per_s": round(rate, 1),
            "fraction_of_hbm_spec": round(rate / HBM_BYTES_PER_S, 4)}


def main_change(args) -> None:
    import torch
    dev = torch.device("cuda")
    for n in args.sizes:
        cls, conf = blocky_map(n, dev)
        before = redrawn_blocks(cls)
        box = np.array([[-1.0, -1.0], [n + 1.0, -1.0], [n + 1.0, n + 1.0], [-1.0, n + 1.0]])
        sets = [("one", [[box]])] + [(f"grid{g}", parcel_grid(n, g)) for g in args.grids]
        for name, zones in sets:
            res = change_call(before, cls, conf, zones, args.reps)
            res.update({"H": n, "W": n, "zone_set": name})
            print(json.dumps(res), flush=True)
        res = code_call(before, cls, args.reps)
        res.update({"H": n, "W": n})
        print(json.dumps(res), flush=True)
        del cls, conf, before


def baseline(cls, zones, n_zones: int) -> float:
    """ms per zone of the route without the kernel: one ops.rasterize_zone call and a masked torch.bincount per zone"""
    import torch
    from flairhip import ops
    H, W = cls.shape
    some = zones[:n_zones]
    best = []
    for rep in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for rings in some:
            xy = np.concatenate(rings)
            ro = np.concatenate([[0], np.cumsum([len(r) for r in rings])]).astype(np.int32)
            mask = ops.rasterize_zone(xy, ro, H, W)
            torch.bincount(cls[mask.bool()].to(torch.int64), minlength=K)
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) * 1e3 / len(some))
    return min(best)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16384])
    ap.add_argument("--grids", type=int, nargs="+", default=[100, 316])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-zones", type=int, default=100)
    ap.add_argument("--change", action="store_true",
                    help="time ffa_zone_change_u8 beside ffa_zone_stats_u8, and ffa_change_code_u8, instead")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_zone_stats needs an MI355X")
    if args.change:
        return main_change(args)
    from flairhip import ops
    dev = torch.device("cuda")
    for n in args.sizes:
        cls, conf = blocky_map(n, dev)
        whole_c = torch.bincount(cls.view(-1).to(torch.int64), minlength=K + 1)
        whole_s = torch.bincount(cls.view(-1).to(torch.int64), weights=conf.view(-1).to(torch.float64),
                                 minlength=K + 1).to(torch.int64)  # < 2^53: exact
        box = np.array([[-1.0, -1.0], [n + 1.0, -1.0], [n + 1.0, n + 1.0], [-1.0, n + 1.0]])
        sets = [("one", [[box]])] + [(f"grid{g}", parcel_grid(n, g)) for g in args.grids]
        for name, zones in sets:
            res, counts, sums = device_call(cls, conf, zones, args.reps)
            # every pixel once: the box holds the raster, the parcels tile it
            assert torch.equal(counts.sum(0), whole_c) and torch.equal(sums.sum(0), whole_s), name
            ops_ms = []
            for rep in range(args.reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                c2, s2 = ops.zone_class_stats(cls, zones, K, conf=conf)
                torch.cuda.synchronize()
                if rep:
                    ops_ms.append((time.perf_counter() - t0) * 1e3)
            assert torch.equal(c2, counts) and torch.equal(s2, sums)
            nb = min(args.baseline_zones, len(zones))
            per_zone = baseline(cls, zones, nb)
            res.update({"H": n, "W": n, "zone_set": name, "ops_ms": round(min(ops_ms), 2),
                        "baseline_zones_timed": nb, "per_zone_baseline_ms": round(per_zone, 4),
                        "baseline_scaled_ms": round(per_zone * len(zones), 1),
                        "baseline_scaled_is_extrapolated": nb < len(zones)})
            print(json.dumps(res), flush=True)
        del cls, conf


if __name__ == "__main__":
    main()
