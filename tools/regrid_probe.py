"""Times of Raster.sample(grid=True) and of one RasterInterpolant call on one GPU, and of the reference's on the CPU.

    python tools/regrid_probe.py [--sizes 1000 3000] [--orders 1 2 3 4 5] [--reps 5] [--out profiles/regrid_probe.json]
    python tools/regrid_probe.py --reference [--out profiles/regrid_reference_cpu.json]   (needs the reference and SciPy)

The DEM is the seeded exact terrain of tests/viewshed_terrain.py (n x n cells of 10 m at UTM-scale coordinates, around
1100 m); it is sampled on a grid of the same size and cell, shifted by 0.37 cells in x and 0.21 in y and pulled inside the
box.  The interpolant blends two such DEMs whose grids differ by that shift (so the second is regridded at order 1), with
their sigma rasters, at a third of the way between them.  GPU figures: `call_ms` is the wall time of the Python call
(median of `--reps` repetitions, each the SECOND of two back-to-back calls: the host's factoring, the tables, allocation,
upload and download included); the split is the library's own HIP events inside such a call (sample: upload / solve /
evaluate / download; interpolant: upload / regrid / blend / download).  The reference is timed on one core of whatever
machine runs it: another machine than the GPU's host, so the two are set side by side, not divided.  Nothing here asserts
a speed.
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

from tests import regrid_restatement as rr  # noqa: E402
from tests import viewshed_terrain as vt  # noqa: E402


def case(n, seed=0):
    z = rr.dem((n, n), 7100 + n + seed)
    xlim, ylim = rr.limits((n, n))
    return z, xlim, ylim


def targets(n, xlim, ylim):
    """(x, y) of the shifted grid's centres that lie inside the box, in the raster's directions."""
    x = vt.centres(xlim, n) + 0.37 * rr.CELL
    y = vt.centres(ylim, n) + 0.21 * rr.CELL
    return x[(x >= min(xlim)) & (x <= max(xlim))], y[(y >= min(ylim)) & (y <= max(ylim))]


def shifted(n, seed):
    """A DEM (and its sigma) one cell larger all round and shifted by (0.37, 0.21) cells against case(n)'s grid."""
    m = n + 2
    xlim, ylim = rr.limits((m, m), x0=rr.X0 - 0.63 * rr.CELL, y0=rr.Y0 - 0.79 * rr.CELL)
    return rr.dem((m, m), 7100 + n + seed), xlim, ylim


def sigma_of(shape, seed):
    return 0.5 + (vt.terrain(shape, seed) + 1024.0) / 1024.0


def gpu(args):
    import torch

    from glimpse_amd import Raster, RasterInterpolant, _lib

    res = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps, "cell": rr.CELL,
           "rule": "median of repetitions, each the second of two back-to-back calls", "sample": {}, "interpolant": {}}
    for n in args.sizes:
        z, xlim, ylim = case(n)
        dem = Raster(z, x=xlim, y=ylim)
        xy = targets(n, xlim, ylim)
        for order in args.orders:
            calls, splits = [], []
            for _ in range(args.reps):
                dem.sample(xy, grid=True, order=order)
                t = time.perf_counter()
                out = dem.sample(xy, grid=True, order=order)
                calls.append(time.perf_counter() - t)
                source, xo, yo, _, _ = dem._grid_source(xy, order, True, np.nan)
                splits.append(_lib.stage_raster_regrid(source, xo, yo, return_times=True)[1])
            med = {k: statistics.median(s[k] for s in splits) for k in _lib.REGRID_TIMES}
            res["sample"][f"{n}_k{order}"] = {"cells": n * n, "order": order, "samples": int(out.size),
                                              "call_ms": 1e3 * statistics.median(calls),
                                              "call_ms_all": [1e3 * c for c in calls], **med}
            print("sample", n, order, json.dumps(res["sample"][f"{n}_k{order}"]), flush=True)
        z1, xlim1, ylim1 = shifted(n, 1)
        means = [dem, Raster(z1, x=xlim1, y=ylim1)]
        sigmas = [Raster(sigma_of(z.shape, 7300 + n), x=xlim, y=ylim), Raster(sigma_of(z1.shape, 7301 + n), x=xlim1, y=ylim1)]
        interpolant = RasterInterpolant(means, sigmas, x=[0.0, 9.0])
        calls, splits = [], []
        for _ in range(args.reps):
            interpolant(3.0, return_sigma=True)
            t = time.perf_counter()
            mean, sigma = interpolant(3.0, return_sigma=True)
            calls.append(time.perf_counter() - t)
            # the library call of that __call__, once more with its events
            box = mean.box2d
            pair = [r.copy() for r in means + sigmas]
            for r in pair:
                r.crop(xlim=box[0::2], ylim=box[1::2])
            m1, xo, yo = interpolant._second(pair[:2], ())
            s1, _, _ = interpolant._second(pair[2:], ())
            splits.append(_lib.stage_raster_interpolate(pair[0].array, m1, 1 / 3, (1 / 3) ** 2, 1 / 3, s0=pair[2].array, s1=s1,
                                                        xo=xo, yo=yo, return_times=True)[2])
        med = {k: statistics.median(s[k] for s in splits) for k in _lib.INTERPOLATE_TIMES}
        res["interpolant"][str(n)] = {"cells": int(mean.array.size), "return_sigma": True, "regridded": True,
                                      "call_ms": 1e3 * statistics.median(calls), "call_ms_all": [1e3 * c for c in calls], **med}
        print("interpolant", n, json.dumps(res["interpolant"][str(n)]), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import refstubs

    glimpse = refstubs.import_reference()
    res = {"what": "the reference's Raster.sample(grid=True) and RasterInterpolant.__call__ (SciPy / NumPy, one core)",
           "repetitions": args.reps, "cell": rr.CELL, "sample": {}, "interpolant": {}}
    for n in args.sizes:
        z, xlim, ylim = case(n)
        dem = glimpse.Raster(z, x=xlim, y=ylim)
        xy = targets(n, xlim, ylim)
        for order in args.orders:
            times = []
            for _ in range(args.reps):
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    t = time.perf_counter()
                    out = dem.sample(xy, grid=True, order=order)
                    times.append(time.perf_counter() - t)
            res["sample"][f"{n}_k{order}"] = {"cells": n * n, "order": order, "samples": int(out.size),
                                              "sample_s": statistics.median(times)}
            print("sample", n, order, json.dumps(res["sample"][f"{n}_k{order}"]), flush=True)
        z1, xlim1, ylim1 = shifted(n, 1)
        means = [dem, glimpse.Raster(z1, x=xlim1, y=ylim1)]
        sigmas = [glimpse.Raster(sigma_of(z.shape, 7300 + n), x=xlim, y=ylim),
                  glimpse.Raster(sigma_of(z1.shape, 7301 + n), x=xlim1, y=ylim1)]
        interpolant = glimpse.RasterInterpolant(means, sigmas, x=[0.0, 9.0])
        times = []
        for _ in range(args.reps):
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                t = time.perf_counter()
                mean, _ = interpolant(3.0, return_sigma=True)
                times.append(time.perf_counter() - t)
        res["interpolant"][str(n)] = {"cells": int(mean.array.size), "return_sigma": True, "call_s": statistics.median(times)}
        print("interpolant", n, json.dumps(res["interpolant"][str(n)]), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 3000])
    ap.add_argument("--orders", type=int, nargs="+", default=[1, 2, 3, 4, 5])
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
