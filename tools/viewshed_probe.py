"""Times of Raster.viewshed on one GPU, and of the reference's Raster.viewshed on the CPU.

    python tools/viewshed_probe.py [--sizes 1024 4096 10000] [--reps 5] [--out profiles/r07_viewshed_probe.json]
    python tools/viewshed_probe.py --reference [--out profiles/r07_viewshed_reference_cpu.json]   (needs the reference)

The DEM is the seeded exact terrain of tests/viewshed_terrain.py (n x n cells of 30 m, 2 % NaN cells), the origin sits
between cell centres on the summit of the DEM's middle part, correction=True.  GPU figures: `call_ms` is the wall time of
`Raster.viewshed` (median of `--reps` repetitions, each the SECOND of two back-to-back calls; allocation, upload and
download included), the split is the library's own HIP events inside such a call (upload / per-cell kernel / sort /
sweep / download; what is left of the call is allocation, the ring histogram's trip to the host and Python), `rings` the
number of sweep launches.  The reference's time is one core of whatever machine runs it: another machine than the GPU's
host, so the two are set side by side, not divided.
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

from tests import viewshed_terrain as vt  # noqa: E402

CELL = 30.0


def case(n):
    z = vt.terrain((n, n), 7000 + n)
    r, c = vt.summit(z, None, None)
    z = vt.holes(z, 7001 + n, 0.02)
    xlim, ylim = (0.0, n * CELL), (n * CELL, 0.0)
    x, y = vt.centres(xlim, n), vt.centres(ylim, n)
    origin = (float(x[c] + 0.3 * CELL), float(y[r] + 0.2 * CELL), float(np.nanmax(z[r - 1:r + 2, c - 1:c + 2]) + 40.0))
    return z, xlim, ylim, origin


def gpu(args):
    import torch

    from glimpse_amd import Raster, _lib

    res = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps, "cell": CELL, "correction": True,
           "rule": "median of repetitions, each the second of two back-to-back calls", "sizes": {}}
    for n in args.sizes:
        z, xlim, ylim, origin = case(n)
        dem = Raster(z, x=xlim, y=ylim)
        xyz = np.array([origin])
        calls, splits, share = [], [], None
        for _ in range(args.reps):
            dem.viewshed(origin, correction=True)
            t = time.perf_counter()
            vis = dem.viewshed(origin, correction=True)
            calls.append(time.perf_counter() - t)
            splits.append(_lib.stage_viewshed(dem, xyz, True, return_times=True, float32=False)[1])
            share = float(vis.mean())
        med = {k: statistics.median(s[k] for s in splits) for k in _lib.VIEWSHED_TIMES}
        res["sizes"][str(n)] = {"cells": n * n, "call_ms": 1e3 * statistics.median(calls), "call_ms_all": [1e3 * c for c in calls],
                                "visible_share": share, **med,
                                "sweep_us_per_launch": 1e3 * med["sweep_ms"] / max(med["launches"], 1)}
        print(n, json.dumps(res["sizes"][str(n)]), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import refstubs

    glimpse = refstubs.import_reference()
    res = {"what": "the reference's Raster.viewshed (NumPy, one core)", "repetitions": args.reps, "cell": CELL,
           "correction": True, "sizes": {}}
    for n in args.sizes:
        z, xlim, ylim, origin = case(n)
        dem = glimpse.Raster(z, x=xlim, y=ylim)
        times = []
        for _ in range(args.reps):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                t = time.perf_counter()
                vis = dem.viewshed(origin, correction=True)
                times.append(time.perf_counter() - t)
        res["sizes"][str(n)] = {"cells": n * n, "viewshed_s": statistics.median(times), "visible_share": float(vis.mean())}
        print(n, json.dumps(res["sizes"][str(n)]), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 10000])
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
