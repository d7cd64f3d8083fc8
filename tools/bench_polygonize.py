"""Polygonisation timings on synthetic class maps (GPU required).

    python tools/bench_polygonize.py [--sizes 5000 16384] [--reps 3] [--confidence] [--zone] [--sieve-area 0.2]
        [--target-crs EPSG:4326] [--compare]

Maps: 'voronoi' (blocky nearest-seed map of 19 classes with 2 % label noise), 'checker' (checkerboard: every pixel a
component, four boundary edges per pixel -- the worst case for edges), 'uniform' (one class: a single component over
the whole raster, the worst case for contention on one accumulator; on request).  Per map it prints one JSON line with
  * device time of the label phase and of the emit phase (hip events around each, after a warm-up call),
  * D2H time of the five output arrays,
  * host times: float64 map coordinates, simplifier (0.1 m at 0.2 m pixels, 16 threads), object build
    (PolygonFrame), GeoPackage write,
  * the counts and a lower bound of the bytes the label phase must move (class map read, labels written and read
    back, edge arrays), with the time that bound would take at the HBM rate (8 TB/s).
With --confidence the zonal-sum stage (ffa_polygonize_zonal_sum_u8 over a random uint8 plane, after emit) is timed
as well: "zonal_sum_ms", and the 5 bytes per pixel it must read (label + value) at the HBM rate.
With --zone one more JSON line per voronoi size: a jagged star contour of 50 000 vertices covering about 40 % of the
map is rasterised (ffa_zone_mask_u8) and applied (ffa_zone_clip_u8), hip-event times, best of --reps after a warm-up,
next to the time the unavoidable traffic would take at the HBM rate (H W bytes of mask written, H W / 8 bytes of toggles
written and read; 3 H W bytes for the clip), and the polygon count and host time (objects + GeoPackage) of the
clipped map and of the whole one.
With --target-crs one JSON line per --vertices count (default 4 M and 43 M, the range the maps above emit): Lambert-93
vertices on a 0.2 m grid are reprojected to that CRS (ffa_crs_transform_f64, device resident, out of place):
"reproject_ms" (hip events, best of --reps after a warm-up) next to the time the 32 bytes per vertex take at the HBM
rate, the same for the inverse direction and for Lambert-93 -> UTM 31N (both projections in the one pass), and
"reproject_host_ms", what ops.reproject_points costs for a numpy array (H2D, kernel, D2H; wall clock).
With --sieve-area M2 one JSON line per voronoi size: the sieve (ffa_sieve_round_u8, regions below M2 at 0.2 m pixels
merged into their largest neighbour) round by round, hip events around each call, per round the best of --reps after
a warm-up: "round_ms", their number, "label_only_ms" (the same call with min_pixels = 1 on the input map: labels,
counts and the root pass, no vote and no apply; "label_only_after_ms": on the sieved map), the round's algorithmic
traffic (class map 1 B, labels 4 B written and three reads per pixel, best + new_class 9 B per component) and the
rate the first round reaches on it, then polygons, rings, vertices and the host stages (objects, GeoPackage) of the
map before and after.
With --workspace counted (or both) the count-sized path is timed: one JSON line with "count_ms", "trace_ms", their
per-repetition sum "label_ms" (the figure to hold against the bound-sized "label_ms"; "label_ms_all" lists every
repetition, for the spread), "emit_ms", both workspaces' sizes and the edges per pixel.  Device stages only;
`--sizes 25000 --maps voronoi --workspace counted` is a full 5 km BD ORTHO dalle, which the bound-sized path refuses.
With --compare one JSON line per voronoi size: object matching of the map (the prediction) against a copy of it
shifted by 3 rows and 5 columns (the reference).  "label_ms" is ffa_polygonize_label on the map, as in the plain run
and in the same session; "overlap_count_ms" (ffa_region_overlap_count: both rasters labelled, regions numbered, the
pair bound) and "overlap_pairs_ms" (region tables, hash insert, compaction) are hip-event times, best of --reps after
a warm-up; "count_over_two_labels" = overlap_count_ms / (2 * label_ms), the count phase against its yardstick of
two label phases; "match_host_ms" is flairhip.objects.match_objects + object_counts on the host (wall clock), and
"ops_ms" the whole ops.region_overlaps call with its two synchronisations and the sort.
Per-kernel times (count_kernel, the labelling kernels and zonal_sum_kernel of the same run side by side): run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_polygonize.py --confidence --device-only`.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flair-for-aigle_amd")]

HBM_BYTES_PER_S = 8.0e12


def voronoi(n: int, seed: int = 0) -> np.ndarray:
    g = np.random.default_rng(seed)
    cell = 64
    k = n // cell + 2
    jitter = g.integers(0, cell, (k, k, 2))
    lab = g.integers(0, 19, (k, k)).astype(np.uint8)
    out = np.zeros((n, n), np.uint8)
    xx = np.arange(n)[None, :]
    cx = xx // cell
    for y0 in range(0, n, 512):  # row blocks keep the temporaries small at 16384^2
        yy = np.arange(y0, min(n, y0 + 512))[:, None]
        cy = yy // cell
        best = np.full((len(yy), n), np.iinfo(np.int64).max)
        for dy in (0, 1):
            for dx in (0, 1):
                sy, sx = np.minimum(cy + dy, k - 1), np.minimum(cx + dx, k - 1)
                d = (sy * cell + jitter[sy, sx, 0] - yy) ** 2 + (sx * cell + jitter[sy, sx, 1] - xx) ** 2
                m = d < best
                best[m] = d[m]
                out[y0:y0 + len(yy)][m] = lab[sy, sx][m]
    noise = g.random((n, n), dtype=np.float32) < 0.02
    out[noise] = g.integers(0, 19, int(noise.sum()), dtype=np.uint8)
    return out


def checker(n: int) -> np.ndarray:
    return (np.add.outer(np.arange(n), np.arange(n)) % 2).astype(np.uint8)


def timed_reps(x, reps: int, confidence: bool, phases, emit, zonal):
    """The timed loop of both paths: hip events around each device phase, ``reps`` repetitions after a warm-up one.
    ``phases``: [(name, prepare)], the label side in order; ``prepare(counts)`` does the host work that precedes its
    phase (reading what the phase before left in the device tensor ``counts``, allocating) and returns the call to
    time.  ``emit((P, R, V, E), bufs)`` and ``zonal((P, R, V, E), values, sums)`` are the calls themselves; the zonal
    sum is timed from the end of emit.  Returns (times in ms by phase name and "emit", "d2h", "zonal"; the counts
    (P, R, V, E); the five output arrays on the host)."""
    import torch
    H, W = x.shape
    dev = x.device
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    values = torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev) if confidence else None
    times = {name: [] for name in [n for n, _ in phases] + ["emit", "d2h", "zonal"]}

    def timed(call):
        events = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        events[0].record()
        call()
        events[1].record()
        return events

    bufs = None
    for rep in range(reps + 1):
        spans = {name: timed(prepare(counts)) for name, prepare in phases}
        n = P, R, V, E = tuple(int(v) for v in counts.cpu().tolist())
        del bufs  # the caching allocator serves the next ones from the same blocks
        bufs = [torch.empty(P, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int64, device=dev),
                torch.empty(P + 1, dtype=torch.int32, device=dev), torch.empty(R + 1, dtype=torch.int32, device=dev),
                torch.empty((V, 2), dtype=torch.int32, device=dev)]
        spans["emit"] = timed(lambda: emit(n, bufs))
        if confidence:
            sums = torch.empty(P, dtype=torch.int64, device=dev)
            zonal(n, values, sums)
            spans["zonal"] = [spans["emit"][1], torch.cuda.Event(enable_timing=True)]  # from the end of emit
            spans["zonal"][1].record()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [b.cpu().numpy() for b in bufs]
        t1 = time.perf_counter()
        if rep:
            for name, (e0, e1) in spans.items():
                times[name].append(e0.elapsed_time(e1))
            times["d2h"].append((t1 - t0) * 1e3)
    if confidence:
        assert int(sums.sum()) == int(values[x != 18].sum(dtype=torch.int64))  # every non-background pixel, once
    return times, n, out


def run(name: str, cls: np.ndarray, reps: int, confidence: bool = False, device_only: bool = False,
        outputs: list = None) -> dict:
    import torch
    from flairhip import lib as L
    from flairhip import ops
    from flair_zonal_detection.polygons import FlatPolygons, PolygonFrame
    lib = L.load()
    H, W = cls.shape
    x = torch.from_numpy(cls).to(torch.device("cuda"))
    nbytes = int(lib.ffa_polygonize_workspace_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    st = torch.cuda.current_stream().cuda_stream

    def label(counts):
        return lambda: L.check(lib.ffa_polygonize_label(x.data_ptr(), H, W, 18, 1, ws.data_ptr(), nbytes,
                                                        counts.data_ptr(), st))

    def emit(n, bufs):
        L.check(lib.ffa_polygonize_emit(ws.data_ptr(), nbytes, H, W, *n[:3], *(b.data_ptr() for b in bufs), st))

    def zonal(n, values, sums):
        L.check(lib.ffa_polygonize_zonal_sum_u8(ws.data_ptr(), nbytes, H, W, values.data_ptr(), n[0],
                                                sums.data_ptr() if n[0] else None, st))

    t, (P, R, V, E), out = timed_reps(x, reps, confidence, [("label", label)], emit, zonal)
    pc, pp, pro, rvo, verts = out
    if outputs is not None:
        outputs[:] = out
    res = {"map": name, "H": H, "W": W, "workspace_GB": round(nbytes / 1e9, 3), "polygons": P, "rings": R,
           "vertices": V, "edges": E, "label_ms": round(min(t["label"]), 3),
           "label_ms_all": [round(v, 3) for v in t["label"]], "emit_ms": round(min(t["emit"]), 3),
           "d2h_ms": round(min(t["d2h"]), 3)}
    # bytes the label phase cannot avoid: class map (1 B) + labels written, read by counts / edges (3 x 4 B) per pixel,
    # then the compacted edge arrays (eid, succ written; ~log2(E) pointer-jumping rounds read 2 x 4 B and write 2 x 4 B)
    rounds = max(1, int(np.ceil(np.log2(max(4 * H * W, 2)))))
    lb = H * W * 13 + E * 8 + 2 * rounds * E * 16
    res["label_bytes_lower_bound_GB"] = round(lb / 1e9, 3)
    res["label_ms_at_hbm_rate"] = round(lb / HBM_BYTES_PER_S * 1e3, 3)
    if confidence:
        res["zonal_sum_ms"] = round(min(t["zonal"]), 3)
        res["zonal_sum_ms_at_hbm_rate"] = round(H * W * 5 / HBM_BYTES_PER_S * 1e3, 3)
    if device_only:
        return res
    t0 = time.perf_counter()
    xy = np.empty(verts.shape, np.float64)
    xy[:, 0] = 651992.36 + verts[:, 0] * 0.2
    xy[:, 1] = 6860417.84 - verts[:, 1] * 0.2
    t1 = time.perf_counter()
    keep = ops.polygon_simplify(xy, rvo, pro, 0.1, 16)
    t2 = time.perf_counter()
    before = np.concatenate([[0], np.cumsum(keep)])
    flat = FlatPolygons(pc, pro, before[rvo].astype(np.int32), xy[keep])
    frame = PolygonFrame.from_flat(flat, "EPSG:2154")
    t3 = time.perf_counter()
    with tempfile.TemporaryDirectory() as d:
        frame.to_file(os.path.join(d, "p.gpkg"), driver="GPKG")
        t4 = time.perf_counter()
        res["gpkg_MB"] = round(os.path.getsize(os.path.join(d, "p.gpkg")) / 1e6, 1)
    res.update({"coords_ms": round((t1 - t0) * 1e3, 1), "simplify_ms": round((t2 - t1) * 1e3, 1),
                "objects_ms": round((t3 - t2) * 1e3, 1), "gpkg_ms": round((t4 - t3) * 1e3, 1),
                "vertices_after_simplify": int(keep.sum())})
    return res


def run_counted(name: str, cls: np.ndarray, reps: int, confidence: bool = False, compare=None) -> dict:
    """The count-sized path (ffa_polygonize_count / _trace / _counted_emit), device stages only: "label_ms" = count +
    trace is what ``run`` calls label_ms.  The trace workspace is allocated in every repetition as
    ops.polygonize_counted does (the caching allocator serves it from the second one on).  ``compare``: the five
    arrays of ``run`` on the same map, checked for equal bytes."""
    import torch
    from flairhip import lib as L
    lib = L.load()
    H, W = cls.shape
    x = torch.from_numpy(cls).to(torch.device("cuda"))
    px_bytes = int(lib.ffa_polygonize_count_bytes(H, W))
    ws_px = torch.empty(px_bytes, dtype=torch.uint8, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    tr = {}  # of the current repetition: the trace workspace, its size and the edge count it was sized for

    def count(counts):
        return lambda: L.check(lib.ffa_polygonize_count(x.data_ptr(), H, W, 18, 1, ws_px.data_ptr(), px_bytes,
                                                        counts.data_ptr(), st))

    def trace(counts):
        E, P = (int(v) for v in counts[:2].cpu().tolist())
        tr.clear()
        nbytes = int(lib.ffa_polygonize_trace_bytes(E, P))
        if nbytes < 0:
            raise SystemExit(lib.ffa_last_error().decode())
        tr.update(ws=torch.empty(nbytes, dtype=torch.uint8, device=x.device), bytes=nbytes, E=E)
        return lambda: L.check(lib.ffa_polygonize_trace(x.data_ptr(), H, W, 1, ws_px.data_ptr(), px_bytes, E, P,
                                                        tr["ws"].data_ptr(), nbytes, counts.data_ptr(), st))

    def emit(n, bufs):
        L.check(lib.ffa_polygonize_counted_emit(ws_px.data_ptr(), px_bytes, H, W, tr["ws"].data_ptr(), tr["bytes"],
                                                tr["E"], *n[:3], *(b.data_ptr() for b in bufs), st))

    def zonal(n, values, sums):
        L.check(lib.ffa_polygonize_counted_zonal_sum_u8(ws_px.data_ptr(), px_bytes, H, W, tr["ws"].data_ptr(),
                                                        tr["bytes"], tr["E"], values.data_ptr(), n[0],
                                                        sums.data_ptr(), st))

    t, (P, R, V, E), out = timed_reps(x, reps, confidence, [("count", count), ("trace", trace)], emit, zonal)
    tr_bytes = tr["bytes"]
    label = [a + b for a, b in zip(t["count"], t["trace"])]
    res = {"map": name, "workspace": "counted", "H": H, "W": W, "pixel_workspace_GB": round(px_bytes / 1e9, 3),
           "trace_workspace_GB": round(tr_bytes / 1e9, 3), "workspace_GB": round((px_bytes + tr_bytes) / 1e9, 3),
           "polygons": P, "rings": R, "vertices": V, "edges": E, "edges_per_pixel": round(E / (H * W), 4),
           "count_ms": round(min(t["count"]), 3), "trace_ms": round(min(t["trace"]), 3),
           "label_ms": round(min(label), 3), "label_ms_all": [round(v, 3) for v in label],
           "emit_ms": round(min(t["emit"]), 3), "jump_rounds": max(1, int(np.ceil(np.log2(max(E, 2)))))}
    if confidence:
        res["zonal_sum_ms"] = round(min(t["zonal"]), 3)
    if compare is not None:
        res["bytes_equal_to_bound_path"] = all(a.tobytes() == b.tobytes() for a, b in zip(compare, out))
    return res


def star_contour(n: int, points: int = 25000) -> np.ndarray:
    """pixel coordinates of a 2 * points-vertex star about the map centre whose area pi R r is 40 % of n^2"""
    k = np.arange(2 * points)
    ang = np.pi * k / points
    rad = np.where(k % 2 == 0, 0.37, 0.344) * n  # pi * 0.37 * 0.344 = 0.400
    return np.stack([n / 2 + 0.3 + rad * np.cos(ang), n / 2 - 0.2 + rad * np.sin(ang)], axis=1)


def host_stage(out) -> dict:
    """simplifier, objects and GeoPackage of polygonize's five arrays (host): the part a zone clip shortens"""
    from flairhip import ops
    from flair_zonal_detection.polygons import FlatPolygons, PolygonFrame
    pc, pp, pro, rvo, verts = out
    xy = np.empty(verts.shape, np.float64)
    xy[:, 0] = 651992.36 + verts[:, 0] * 0.2
    xy[:, 1] = 6860417.84 - verts[:, 1] * 0.2
    t1 = time.perf_counter()
    keep = ops.polygon_simplify(xy, rvo, pro, 0.1, 16)
    t2 = time.perf_counter()
    before = np.concatenate([[0], np.cumsum(keep)])
    frame = PolygonFrame.from_flat(FlatPolygons(pc, pro, before[rvo].astype(np.int32), xy[keep]), "EPSG:2154")
    t3 = time.perf_counter()
    with tempfile.TemporaryDirectory() as d:
        frame.to_file(os.path.join(d, "p.gpkg"), driver="GPKG")
        t4 = time.perf_counter()
    return {"polygons": len(pc), "simplify_ms": round((t2 - t1) * 1e3, 1), "objects_ms": round((t3 - t2) * 1e3, 1),
            "gpkg_ms": round((t4 - t3) * 1e3, 1)}


def run_zone(cls: np.ndarray, reps: int, device_only: bool = False) -> dict:
    import torch
    from flairhip import lib as L
    from flairhip import ops
    lib = L.load()
    H, W = cls.shape
    dev = torch.device("cuda")
    ring = star_contour(H)
    xy = torch.from_numpy(ring).to(dev)
    ro = torch.tensor([0, len(ring)], dtype=torch.int32, device=dev)
    nbytes = int(lib.ffa_zone_mask_workspace_bytes(H, W, len(ring)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    x0 = torch.from_numpy(cls).to(dev)
    t_mask, t_clip = [], []
    for rep in range(reps + 1):
        x = x0.clone()
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        L.check(lib.ffa_zone_mask_u8(xy.data_ptr(), ro.data_ptr(), 1, H, W, mask.data_ptr(), 0, ws.data_ptr(), nbytes, st))
        e1.record()
        L.check(lib.ffa_zone_clip_u8(x.data_ptr(), mask.data_ptr(), None, H * W, 18, st))
        e2.record()
        torch.cuda.synchronize()
        if rep:
            t_mask.append(e0.elapsed_time(e1))
            t_clip.append(e1.elapsed_time(e2))
    mask_lb, clip_lb = H * W + 2 * (H * W // 8), 3 * H * W
    res = {"map": "voronoi+zone", "H": H, "W": W, "zone_vertices": len(ring),
           "zone_fraction": round(float(mask.sum(dtype=torch.int64)) / (H * W), 4),
           "zone_mask_ms": round(min(t_mask), 4), "zone_mask_ms_at_hbm_rate": round(mask_lb / HBM_BYTES_PER_S * 1e3, 4),
           "zone_clip_ms": round(min(t_clip), 4), "zone_clip_ms_at_hbm_rate": round(clip_lb / HBM_BYTES_PER_S * 1e3, 4)}
    res["zone_mask_fraction_of_bound"] = round(res["zone_mask_ms_at_hbm_rate"] / res["zone_mask_ms"], 4)
    if device_only:
        return res
    for name, t in (("with_zone", x), ("without_zone", x0)):
        res[name] = host_stage([a.cpu().numpy() for a in ops.polygonize(t, 18, 1)])
    return res


def run_sieve(cls: np.ndarray, reps: int, sieve_area: float, device_only: bool = False) -> dict:
    import torch
    from flairhip import lib as L
    from flairhip import ops
    from flair_zonal_detection.inference import sieve_pixels_for_area
    lib = L.load()
    H, W = cls.shape
    dev = torch.device("cuda")
    T = sieve_pixels_for_area(sieve_area, 0.2 * 0.2)
    nbytes = int(lib.ffa_sieve_workspace_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    x0 = torch.from_numpy(cls).to(dev)

    def timed_round(x, min_pixels):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        L.check(lib.ffa_sieve_round_u8(x.data_ptr(), H, W, 18, min_pixels, ws.data_ptr(), nbytes, counts.data_ptr(), st))
        e1.record()
        c = counts.cpu().tolist()  # synchronises
        return e0.elapsed_time(e1), c

    per_rep, label_only, label_only_in, first = [], [], [], None
    for rep in range(reps + 1):
        x = x0.clone()
        ms_in, _ = timed_round(x, 1)  # min_pixels = 1 moves nothing
        times = []
        while len(times) < 64:
            ms, c = timed_round(x, T)
            times.append(ms)
            first = first or c
            if c[2] == 0:
                break
        ms, _ = timed_round(x, 1)
        if rep:
            per_rep.append(times)
            label_only.append(ms)
            label_only_in.append(ms_in)
    assert len({len(t) for t in per_rep}) == 1  # the same rounds every time
    round_ms = [round(min(t[k] for t in per_rep), 4) for k in range(len(per_rep[0]))]
    small, comps_moved, pixels_moved, comps = first
    traffic = H * W * 17 + comps * 9
    res = {"map": "voronoi+sieve", "H": H, "W": W, "sieve_area": sieve_area, "sieve_pixels": T,
           "workspace_GB": round(nbytes / 1e9, 3), "rounds": len(round_ms), "round_ms": round_ms,
           "label_only_ms": round(min(label_only_in), 4), "label_only_after_ms": round(min(label_only), 4),
           "components": comps, "small_components": small,
           "first_round_relabelled_components": comps_moved, "first_round_relabelled_pixels": pixels_moved,
           "round_traffic_GB": round(traffic / 1e9, 4),
           "first_round_TB_per_s": round(traffic / (round_ms[0] * 1e-3) / 1e12, 3),
           "round_ms_at_hbm_rate": round(traffic / HBM_BYTES_PER_S * 1e3, 4)}
    for name, t in (("before", x0), ("after", x)):
        out = [a.cpu().numpy() for a in ops.polygonize(t, 18, 1)]
        side = {"polygons": len(out[0]), "rings": len(out[3]) - 1, "vertices": len(out[4])}
        if not device_only:
            side.update({k: v for k, v in host_stage(out).items() if k != "polygons"})
        res[name] = side
    return res


def run_compare(cls: np.ndarray, reps: int) -> dict:
    import torch
    from flairhip import lib as L
    from flairhip import objects, ops
    lib = L.load()
    H, W = cls.shape
    dev = torch.device("cuda")
    a = torch.from_numpy(cls).to(dev)
    b = torch.from_numpy(np.roll(cls, (3, 5), (0, 1))).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    counts = torch.empty(4, dtype=torch.int64, device=dev)

    def timed(call):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    res = {"map": "voronoi+compare", "H": H, "W": W}
    if 4 * H * W < 1 << 31:  # the label phase of the plain run, in this session
        nbytes = int(lib.ffa_polygonize_workspace_bytes(H, W))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        t = [timed(lambda: L.check(lib.ffa_polygonize_label(a.data_ptr(), H, W, 18, 1, ws.data_ptr(), nbytes,
                                                            counts.data_ptr(), st))) for _ in range(reps + 1)][1:]
        res["label_ms"] = round(min(t), 3)
        del ws
    nbytes = int(lib.ffa_region_overlap_bytes(H, W))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    t_count, t_pairs = [], []
    for rep in range(reps + 1):
        ms = timed(lambda: L.check(lib.ffa_region_overlap_count(a.data_ptr(), b.data_ptr(), H, W, 18, 18, 1, 1,
                                                                ws.data_ptr(), nbytes, counts.data_ptr(), st)))
        Pa, Pb, Q, _ = (int(v) for v in counts.cpu().tolist())
        tbytes = int(lib.ffa_region_overlap_table_bytes(Q))
        table = torch.empty(tbytes, dtype=torch.uint8, device=dev)
        out = [torch.empty(n, dtype=dt, device=dev) for n, dt in
               ((Pa, torch.int32), (Pa, torch.int32), (Pa, torch.int64), (Pb, torch.int32), (Pb, torch.int32),
                (Pb, torch.int64), (Q, torch.int32), (Q, torch.int32), (Q, torch.int64))]
        ms2 = timed(lambda: L.check(lib.ffa_region_overlap_pairs(ws.data_ptr(), nbytes, H, W, Pa, Pb, Q, table.data_ptr(),
                                                                 tbytes, *(o.data_ptr() for o in out),
                                                                 counts.data_ptr(), st)))
        if rep:
            t_count.append(ms)
            t_pairs.append(ms2)
    overflow, n_pairs = (int(v) for v in counts[2:].cpu().tolist())
    assert not overflow and n_pairs <= Q
    del ws, table, out
    t0 = time.perf_counter()
    ov = ops.region_overlaps(a, b, 18, 18)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    m = objects.match_objects(ov, 0.5, "same")
    c, _ = objects.object_counts(ov, m, 19)
    t2 = time.perf_counter()
    assert len(ov.pair_a) == n_pairs
    res.update({"workspace_GB": round(nbytes / 1e9, 3), "table_MB": round(tbytes / 1e6, 1), "regions_a": Pa,
                "regions_b": Pb, "pair_bound": Q, "pairs": n_pairs, "overlap_count_ms": round(min(t_count), 3),
                "overlap_pairs_ms": round(min(t_pairs), 3), "ops_ms": round((t1 - t0) * 1e3, 1),
                "match_host_ms": round((t2 - t1) * 1e3, 1), "matched": int(c[:, 0].sum())})
    if "label_ms" in res:
        res["count_over_two_labels"] = round(res["overlap_count_ms"] / (2 * res["label_ms"]), 3)
    return res


def run_reproject(n: int, target_crs: str, reps: int) -> dict:
    import torch
    from flairhip import ops
    dev = torch.device("cuda")
    g = np.random.default_rng(0)
    xy = np.empty((n, 2), np.float64)
    xy[:, 0] = 651992.4 + 0.2 * g.integers(0, 200000, n)
    xy[:, 1] = 6860417.8 - 0.2 * g.integers(0, 200000, n)
    src = torch.from_numpy(xy).to(dev)
    dst = torch.empty_like(src)
    back = torch.empty_like(src)

    def timed(a, b, s, d):
        best = []
        for rep in range(reps + 1):
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            e0.record()
            ops.reproject_points(a, s, d, out=b)
            e1.record()
            torch.cuda.synchronize()
            if rep:
                best.append(e0.elapsed_time(e1))
        return round(min(best), 4)

    res = {"map": "reproject", "vertices": n, "target_crs": target_crs,
           "reproject_ms": timed(src, dst, "EPSG:2154", target_crs),
           "reproject_back_ms": timed(dst, back, target_crs, "EPSG:2154"),
           "reproject_2154_to_32631_ms": timed(src, back, "EPSG:2154", "EPSG:32631"),
           "reproject_ms_at_hbm_rate": round(32.0 * n / HBM_BYTES_PER_S * 1e3, 4)}
    res["reproject_fraction_of_bound"] = round(res["reproject_ms_at_hbm_rate"] / res["reproject_ms"], 4)
    ops.reproject_points(dst, target_crs, "EPSG:2154", out=back)
    res["round_trip_max_m"] = float((back - src).abs().max())
    host = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        ops.reproject_points(xy, "EPSG:2154", target_crs)
        if rep:
            host.append((time.perf_counter() - t0) * 1e3)
    res["reproject_host_ms"] = round(min(host), 3)
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 16384])
    ap.add_argument("--maps", nargs="+", default=["voronoi", "checker"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--checker-size", type=int, default=5000)
    ap.add_argument("--confidence", action="store_true", help="also time the zonal-sum stage (per-polygon sums)")
    ap.add_argument("--device-only", action="store_true",
                    help="skip the host stages (simplifier, objects, GeoPackage: minutes on the checkerboard)")
    ap.add_argument("--zone", action="store_true",
                    help="voronoi maps only: time the zone mask + clip and the host stages with and without the zone")
    ap.add_argument("--sieve-area", type=float, default=None, metavar="M2",
                    help="voronoi maps only: time the sieve round by round and the stages after it with and without")
    ap.add_argument("--target-crs", type=str, default=None, metavar="EPSG:NNNN",
                    help="time the reprojection of --vertices Lambert-93 vertices to this CRS instead of the maps")
    ap.add_argument("--compare", action="store_true",
                    help="voronoi maps only: time the region overlaps (count, pairs) and the host matching of the map "
                         "against a shifted copy, next to the label phase")
    ap.add_argument("--vertices", type=int, nargs="+", default=[4_000_000, 43_000_000])
    ap.add_argument("--workspace", choices=["bound", "counted", "both"], default="bound",
                    help="bound: ffa_polygonize_label, sizes up to 23170; counted: ffa_polygonize_count / _trace, device "
                         "stages only, sizes up to 32767 (--sizes 25000 is one BD ORTHO dalle); both: one line each, "
                         "and the outputs compared byte for byte")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_polygonize needs an MI355X")
    if args.target_crs:
        for n in args.vertices:
            print(json.dumps(run_reproject(n, args.target_crs, args.reps)), flush=True)
        return
    if args.compare:
        for n in args.sizes:
            print(json.dumps(run_compare(voronoi(n), args.reps)), flush=True)
        return
    if args.sieve_area is not None:
        for n in args.sizes:
            print(json.dumps(run_sieve(voronoi(n), args.reps, args.sieve_area, args.device_only)), flush=True)
        return
    if args.zone:
        for n in args.sizes:
            print(json.dumps(run_zone(voronoi(n), args.reps, args.device_only)), flush=True)
        return
    def both(name, cls):
        old = []
        if args.workspace in ("bound", "both"):
            res = run(name, cls, args.reps, args.confidence, args.device_only, old)
            print(json.dumps(dict(res, workspace="bound")), flush=True)
        if args.workspace in ("counted", "both"):
            print(json.dumps(run_counted(name, cls, args.reps, args.confidence, old or None)), flush=True)

    if "voronoi" in args.maps:
        for n in args.sizes:
            both("voronoi", voronoi(n))
    if "uniform" in args.maps:
        for n in args.sizes:
            both("uniform", np.full((n, n), 3, np.uint8))
    if "checker" in args.maps:
        both("checker", checker(args.checker_size))


if __name__ == "__main__":
    main()
