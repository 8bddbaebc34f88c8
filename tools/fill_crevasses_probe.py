"""Times of Raster.fill_crevasses on one GPU, and of the reference's Raster.fill_crevasses on the CPU.

    python tools/fill_crevasses_probe.py [--sizes 1024 4096 10000] [--reps 5] [--out profiles/r09_fill_crevasses_probe.json]
    python tools/fill_crevasses_probe.py --reference [--out profiles/r09_fill_crevasses_reference_cpu.json]   (needs the reference)

The DEM is the seeded exact terrain of tests/viewshed_terrain.py (n x n cells, float64) with 2 % of the cells lowered by
25 (the crevasses); the masked runs exclude a seeded 5 % of the cells with fill=True; the filters are the defaults (a 5 x 5
maximum, sigma 5: 41 taps an axis).  GPU figures: `call_ms` is the wall time of `Raster.fill_crevasses` (median of `--reps`
repetitions after a warm-up call; the NaN check, allocation, upload and download included), the split is the library's own
HIP events inside such a call (upload / maximum / Gaussian along rows / along columns / download).  Per kernel,
`share_of_8TBs` is its ALGORITHMIC bytes -- each array it must read or write once, counted below -- over its time, over
8 TB/s: what the kernel moves through the caches to serve its taps is not in that count.  The reference's time is one core
of whatever machine runs it: another machine than the GPU's host, so the two are set side by side, not divided.
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

PEAK = 8.0e12  # bytes per second
# algorithmic bytes per cell of a float64 DEM: (with a mask, without)
BYTES = {"max_ms": (8 + 1 + 8, 8 + 8),         # the array, the mask -> the maximum
         "gauss0_ms": (8 + 1 + 8 + 8, 8 + 8),  # the maximum, the mask -> xf, xf_sum
         "gauss1_ms": (8 + 8 + 1 + 8, 8 + 8)}  # xf, xf_sum, the mask -> the result


def case(n):
    z = vt.terrain((n, n), 9000 + n)
    rng = np.random.default_rng(9001 + n)
    z[rng.random(z.shape) < 0.02] -= 25.0
    mask = rng.random(z.shape) >= 0.05
    return z, mask


def gpu(args):
    import torch

    from glimpse_amd import Raster, filters

    res = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps, "dtype": "float64",
           "maximum": {"size": 5}, "gaussian": {"sigma": 5},
           "rule": "median of repetitions after one warm-up call", "bytes_per_cell": BYTES, "sizes": {}}
    for n in args.sizes:
        z, mask = case(n)
        res["sizes"][str(n)] = {"cells": n * n}
        for label, m, fill in (("masked_fill", mask, True), ("no_mask", None, False)):
            Raster(z.copy()).fill_crevasses(mask=m, fill=fill)
            calls, splits = [], []
            for _ in range(args.reps):
                dem = Raster(z.copy())
                t = time.perf_counter()
                dem.fill_crevasses(mask=m, fill=fill)
                calls.append(time.perf_counter() - t)
                splits.append(filters.fill_crevasses(z, {"size": 5}, {"sigma": 5}, mask=m, fill=fill, return_times=True)[1])
            med = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
            share = {k: BYTES[k][0 if m is not None else 1] * n * n / (med[k] * 1e-3) / PEAK for k in BYTES}
            res["sizes"][str(n)][label] = {"call_ms": 1e3 * statistics.median(calls), "call_ms_all": [1e3 * c for c in calls],
                                           **med, "share_of_8TBs": share}
            print(n, label, json.dumps(res["sizes"][str(n)][label]), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import refstubs

    glimpse = refstubs.import_reference()
    import scipy

    res = {"what": "the reference's Raster.fill_crevasses (scipy.ndimage %s, one core)" % scipy.__version__,
           "repetitions": args.reps, "dtype": "float64", "maximum": {"size": 5}, "gaussian": {"sigma": 5}, "sizes": {}}
    for n in args.sizes:
        z, mask = case(n)
        res["sizes"][str(n)] = {"cells": n * n}
        for label, m, fill in (("masked_fill", mask, True), ("no_mask", None, False)):
            times = []
            for _ in range(args.reps):
                dem = glimpse.Raster(z.copy())
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore")
                    t = time.perf_counter()
                    dem.fill_crevasses(mask=m, fill=fill)
                    times.append(time.perf_counter() - t)
            res["sizes"][str(n)][label] = {"fill_crevasses_s": statistics.median(times), "all_s": times}
            print(n, label, json.dumps(res["sizes"][str(n)][label]), flush=True)
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
