"""Times of Raster.gradient, Raster.hillshade and Raster.rasterize_polygons on one GPU, and of the reference's gradient and
hillshade on the CPU.

    python tools/terrain_probe.py [--sizes 2048 8192] [--reps 5] [--out profiles/r12_terrain_probe.json]
    python tools/terrain_probe.py --reference [--out profiles/r12_terrain_reference_cpu.json]   (needs the reference)

The DEM is the seeded exact terrain of tests/viewshed_terrain.py (n x n cells of 10 x 10, float64 and float32).  GPU figures:
`call_ms` is the wall time of the Raster method (median of `--reps` repetitions after a warm-up call; allocation, upload
and download included), the split is the library's own HIP events inside such a call.  Per kernel, `share_of_8TBs` is its
ALGORITHMIC bytes -- each array it must read or write once, counted below -- over its time, over 8 TB/s: what the stencil
reads again through the caches is not in that count.  The polygon mask is an outline of 720 vertices over the middle
three quarters of the grid with a hole of 90; its kernels are timed together (bytes: the mask written once).  The
reference's time is one core of whatever machine runs it: another machine than the GPU's host, so the two are set side by
side, not divided.  (The reference's rasterize_polygons needs GDAL and is not timed.)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import terrain_restatement as tr  # noqa: E402
from tests import viewshed_terrain as vt  # noqa: E402

PEAK = 8.0e12  # bytes per second
# algorithmic bytes per cell of a float64 DEM (a float32 DEM: z and the gradients count 4)
GRADIENT_BYTES = 8 + 8 + 8  # z -> dzdx, dzdy
HILLSHADE_BYTES = 8 + 8     # z -> the float64 intensity (the whole call; per kernel below)
HILLSHADE_KERNEL_BYTES = {"stencil_ms": 8 + 8, "normalise_ms": 8 + 8}  # z -> raw; raw -> intensity in place


def case(n, dtype):
    from glimpse_amd import Raster

    return Raster(vt.terrain((n, n), 9300 + n).astype(dtype), x=(0.0, 10.0 * n), y=(10.0 * n, 0.0))


def outline(n):
    rng = np.random.default_rng(9301 + n)
    middle = (5.0 * n, 5.0 * n)
    return (tr.star(rng, middle, 2.5 * n, 3.75 * n, 720), tr.star(rng, middle, 0.5 * n, 1.0 * n, 90))


def timed(call, reps):
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(1e3 * (time.perf_counter() - t))
    return times


def gpu(args):
    import torch

    from glimpse_amd import _lib, helpers

    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH), "repetitions": args.reps,
           "rule": "median of repetitions after one warm-up call",
           "bytes_per_cell": {"gradient": GRADIENT_BYTES, "hillshade": HILLSHADE_BYTES, **HILLSHADE_KERNEL_BYTES},
           "sizes": {}}
    for n in args.sizes:
        out = res["sizes"][str(n)] = {"cells": n * n}
        for dtype in ("float64", "float32"):
            dem = case(n, dtype)
            d, cell = dem.d, 8 if dtype == "float64" else 4
            calls = timed(dem.gradient, args.reps)
            splits = [_lib.stage_gradient(dem.array, d[0], d[1], return_times=True)[1] for _ in range(args.reps)]
            med = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
            out[f"gradient_{dtype}"] = {"call_ms": statistics.median(calls), "call_ms_all": calls, **med,
                                        "share_of_8TBs": 3 * cell * n * n / (med["kernel_ms"] * 1e-3) / PEAK}
            print(n, "gradient", dtype, json.dumps(out[f"gradient_{dtype}"]), flush=True)
            calls = timed(dem.hillshade, args.reps)
            light = tr.light_direction(315, 45)
            splits = [_lib.stage_hillshade(dem.array, d[0], -d[1], 1.0, light, 1.0, return_times=True)[1]
                      for _ in range(args.reps)]
            med = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
            kernels = med["stencil_ms"] + med["reduce_ms"] + med["normalise_ms"]
            share = {k: (cell + 8 if k == "stencil_ms" else 16) * n * n / (med[k] * 1e-3) / PEAK for k in HILLSHADE_KERNEL_BYTES}
            share["kernels"] = (cell + 8) * n * n / (kernels * 1e-3) / PEAK
            out[f"hillshade_{dtype}"] = {"call_ms": statistics.median(calls), "call_ms_all": calls, **med,
                                         "kernels_ms": kernels, "share_of_8TBs": share}
            print(n, "hillshade", dtype, json.dumps(out[f"hillshade_{dtype}"]), flush=True)
        dem = case(n, "float32")
        ring, hole = outline(n)
        calls = timed(lambda: dem.rasterize_polygons([ring], holes=[hole]), args.reps)
        to_cells = lambda xy: ((xy - np.array((dem.xlim[0], dem.ylim[0]))) / dem.d - 0.5) + 0.5  # noqa: E731
        splits = [helpers.polygons_to_mask([to_cells(ring)], dem.size, [to_cells(hole)], return_times=True)[1]
                  for _ in range(args.reps)]
        med = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
        mask = dem.rasterize_polygons([ring], holes=[hole])
        out["polygon_mask"] = {"vertices": [len(ring), len(hole)], "inside": int(mask.sum()), "call_ms": statistics.median(calls),
                               "call_ms_all": calls, **med, "share_of_8TBs": n * n / (med["kernels_ms"] * 1e-3) / PEAK}
        print(n, "polygon_mask", json.dumps(out["polygon_mask"]), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import matplotlib
    import refstubs

    glimpse = refstubs.import_reference()
    res = {"what": "the reference's Raster.gradient and Raster.hillshade (NumPy %s, matplotlib %s, one core)"
                   % (np.__version__, matplotlib.__version__), "repetitions": args.reps, "sizes": {}}
    for n in args.sizes:
        out = res["sizes"][str(n)] = {"cells": n * n}
        for dtype in ("float64", "float32"):
            dem = glimpse.Raster(vt.terrain((n, n), 9300 + n).astype(dtype), x=(0.0, 10.0 * n), y=(10.0 * n, 0.0))
            for name, call in (("gradient", dem.gradient), ("hillshade", dem.hillshade)):
                times = []
                for _ in range(args.reps):
                    with warnings.catch_warnings(), np.errstate(all="ignore"):
                        warnings.simplefilter("ignore")
                        t = time.perf_counter()
                        call()
                        times.append(time.perf_counter() - t)
                out[f"{name}_{dtype}"] = {"seconds": statistics.median(times), "all_s": times}
                print(n, name, dtype, json.dumps(out[f"{name}_{dtype}"]), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 8192])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = reference(a) if a.reference else gpu(a)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")
