"""Times of Raster.horizon on one GPU, and of the reference's Raster.horizon on the CPU.

    python tools/horizon_probe.py [--sizes 1024 4096 10000] [--headings 360 36000] [--reps 5] [--out profiles/r10_horizon_probe.json]
    python tools/horizon_probe.py --reference [--out profiles/r10_horizon_reference_cpu.json]   (needs the reference)

The DEM is the seeded exact terrain of tests/viewshed_terrain.py (n x n cells of 30 m, 2 % NaN cells), the origin sits
between cell centres on the summit of the DEM's middle part, 2 m above the highest of the nine cells around it,
correction=True; the headings are np.arange(0, 360, 360 / count).  GPU figures: `call_ms` is the wall time of
`Raster.horizon` (median of `--reps` repetitions, each the SECOND of two back-to-back calls; the host's rays, allocation,
upload and download included), the split is the library's own HIP events inside such a call (upload / kernel / download).
The reference is timed on the headings it can compute (it raises where a ray's exit lies a rounding error outside the
box: tests/horizon_restatement.py), on one core of whatever machine runs it: another machine than the GPU's host, so the
two are set side by side, not divided.  Nothing here asserts a speed.
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

from tests import horizon_restatement as hr  # noqa: E402
from tests import viewshed_terrain as vt  # noqa: E402

CELL = 30.0


def case(n):
    z = vt.terrain((n, n), 7000 + n)
    r, c = vt.summit(z, None, None)
    z = vt.holes(z, 7001 + n, 0.02)
    xlim, ylim = (0.0, n * CELL), (n * CELL, 0.0)
    x, y = vt.centres(xlim, n), vt.centres(ylim, n)
    origin = (float(x[c] + 0.3 * CELL), float(y[r] + 0.2 * CELL), float(np.nanmax(z[r - 1:r + 2, c - 1:c + 2]) + 2.0))
    return z, xlim, ylim, origin


def gpu(args):
    import torch

    from glimpse_amd import Raster, _lib

    res = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps, "cell": CELL, "correction": True,
           "rule": "median of repetitions, each the second of two back-to-back calls", "sizes": {}}
    for n in args.sizes:
        z, xlim, ylim, origin = case(n)
        dem = Raster(z, x=xlim, y=ylim)
        for count in args.headings:
            headings = np.arange(0, 360, 360 / count)
            start, ends = dem._horizon_rays(origin, headings)
            calls, splits, points = [], [], None
            for _ in range(args.reps):
                dem.horizon(origin, headings=headings, correction=True)
                t = time.perf_counter()
                runs = dem.horizon(origin, headings=headings, correction=True)
                calls.append(time.perf_counter() - t)
                splits.append(_lib.stage_horizon(dem, np.array([origin]), start[None], ends[None], True, return_times=True,
                                                 float32=False)[2])
                points = sum(len(r) for r in runs)
            med = {k: statistics.median(s[k] for s in splits) for k in _lib.HORIZON_TIMES}
            visits = int(np.abs(ends - start).max(axis=1).sum())
            res["sizes"][f"{n}x{count}"] = {"cells": n * n, "headings": count, "cell_visits": visits, "points": points,
                                           "call_ms": 1e3 * statistics.median(calls), "call_ms_all": [1e3 * c for c in calls],
                                           **med, "kernel_ns_per_visit": 1e6 * med["kernel_ms"] / max(visits, 1)}
            print(n, count, json.dumps(res["sizes"][f"{n}x{count}"]), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import refstubs

    glimpse = refstubs.import_reference()
    res = {"what": "the reference's Raster.horizon (NumPy, one core) on the headings it computes", "repetitions": args.reps,
           "cell": CELL, "correction": True, "sizes": {}}
    for n in args.sizes:
        z, xlim, ylim, origin = case(n)
        dem = glimpse.Raster(z, x=xlim, y=ylim)
        for count in args.headings:
            headings = np.arange(0, 360, 360 / count)
            _, _, raw = hr.rays(z.shape, xlim, ylim, origin, headings)
            computes = (raw[:, 0] >= 0) & (raw[:, 0] < n) & (raw[:, 1] >= 0) & (raw[:, 1] < n)
            times = []
            for _ in range(args.reps):
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    t = time.perf_counter()
                    runs = dem.horizon(origin, headings=headings[computes], correction=True)
                    times.append(time.perf_counter() - t)
            res["sizes"][f"{n}x{count}"] = {"cells": n * n, "headings": count, "headings_computed": int(computes.sum()),
                                           "horizon_s": statistics.median(times), "points": sum(len(r) for r in runs)}
            print(n, count, json.dumps(res["sizes"][f"{n}x{count}"]), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 10000])
    ap.add_argument("--headings", type=int, nargs="+", default=[360, 36000])
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
