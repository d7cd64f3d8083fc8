"""Polygonise one or several class rasters of one grid as ONE raster and write a GeoPackage (GPU required).

    python tools/polygonize_rasters.py out.gpkg in1.tif in2.tif ... [--classes 6 7] [--min-area 20]
        [--simplification 0.1] [--zone zone.geojson] [--zone-crs auto] [--target-crs EPSG:4326]
        [--confidence c1.tif c2.tif ...] [--workspace auto]

A thin wrapper over flair_zonal_detection.inference.rasters_to_polygons: adjacent dalles are assembled into one
mosaic on the device, so an object lying across a seam comes out as one polygon with its whole area, and a full
25 000 x 25 000 dalle goes through the count-sized workspace.  Prints one JSON line with the polygon count and times.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flair-for-aigle_amd")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("output", help="GeoPackage to write")
    ap.add_argument("rasters", nargs="+", help="one-band uint8 class rasters (GeoTIFF) on one grid, in any order")
    ap.add_argument("--confidence", nargs="+", default=None, metavar="TIF",
                    help="one confidence raster per class raster, in the same order: adds confidence and pixels columns")
    ap.add_argument("--classes", type=int, nargs="+", default=None, help="class ids to keep (default: all)")
    ap.add_argument("--background", type=int, default=18, help="the value that is no class (default 18)")
    ap.add_argument("--min-area", type=float, default=1.0, help="drop polygons below this area, map units squared")
    ap.add_argument("--simplification", type=float, default=0.1, help="simplifier tolerance in map units, 0 = off")
    ap.add_argument("--sieve-area", type=float, default=0.0)
    ap.add_argument("--zone", default=None, help="GeoJSON file: only pixels whose centre is inside are polygonised")
    ap.add_argument("--zone-crs", default=None, help="CRS of the zone ('auto' for GeoJSON); default: the rasters'")
    ap.add_argument("--target-crs", default=None, help="CRS of the written polygons; default: the rasters'")
    ap.add_argument("--workspace", choices=["auto", "bound", "counted"], default="auto")
    ap.add_argument("--jobs", type=int, default=None, help="host threads of the simplifier (at most 16)")
    args = ap.parse_args(argv)
    from flair_zonal_detection.inference import rasters_to_polygons
    t0 = time.perf_counter()
    frame = rasters_to_polygons(args.rasters, confidence=args.confidence, background_value=args.background,
                                min_area=args.min_area, simplification=args.simplification, n_jobs=args.jobs,
                                zone=args.zone, classes=args.classes, zone_crs=args.zone_crs,
                                target_crs=args.target_crs, sieve_area=args.sieve_area, workspace=args.workspace)
    t1 = time.perf_counter()
    frame.to_file(args.output, driver="GPKG")
    t2 = time.perf_counter()
    print(json.dumps({"output": args.output, "rasters": len(args.rasters), "polygons": len(frame),
                      "crs": str(frame.crs), "polygons_s": round(t1 - t0, 3), "gpkg_s": round(t2 - t1, 3)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
