"""Times of optimize.CLAHE (glh_stage_clahe) on one GPU, and of its NumPy restatement on one CPU core.

    python tools/clahe_probe.py [--sizes 640x480 1920x1080 4000x3000] [--reps 5] [--out profiles/clahe_probe.json]
    python tools/clahe_probe.py --restatement --out profiles/clahe_restatement_cpu.json      (the CPU part alone: no GPU)

The frame is the seeded snow frame of tests/clahe_restated.py (a bright smooth band under a darker noisy third), gray and
RGB, at clipLimit 40 and the default 8 x 8 grid.  GPU figures: `call_ms` is the wall time of _lib.stage_clahe (median of
`--reps` repetitions after a warm-up call; allocation, upload and download included), the split is the library's own HIP
events inside such a call.  Per kernel, `share_of_8TBs` is its ALGORITHMIC bytes -- each array it must read or write once,
counted below -- over its time, over 8 TB/s: what the reflection reads twice and the table reads of the blend are not in
that count.  The first GPU result is checked against the restatement byte for byte at the smallest size.  The
restatement's time is one core of whatever machine runs it: set side by side with the GPU's, not divided.
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

from tests import clahe_restated as cr  # noqa: E402

PEAK = 8.0e12  # bytes per second
CLIP, GRID = 40.0, (8, 8)


def kernel_bytes(w, h, c):
    """Algorithmic bytes of each kernel: the histogram reads every channel and, with more than one, writes the gray plane;
    the tables read the counts and write the bytes; the blend reads the gray plane and writes the result."""
    tiles = GRID[0] * GRID[1]
    return {"histogram_ms": w * h * c + (w * h if c > 1 else 0) + tiles * 256 * 4, "lut_ms": tiles * 256 * 5,
            "apply_ms": 2 * w * h}


def frames(w, h):
    gray = cr.snow(h, w)
    return {"gray": gray, "rgb": np.ascontiguousarray(np.stack([gray, gray, gray], axis=2))}


def gpu(args):
    import torch

    from glimpse_amd import _lib

    res = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH), "repetitions": args.reps,
           "rule": "median of repetitions after one warm-up call", "clipLimit": CLIP, "tileGridSize": GRID, "sizes": {}}
    checked = False
    for w, h in args.sizes:
        out = res["sizes"][f"{w}x{h}"] = {"pixels": w * h}
        for name, array in frames(w, h).items():
            c = 1 if array.ndim == 2 else array.shape[2]
            found = _lib.stage_clahe(array, CLIP, GRID)  # the warm-up call
            if not checked:
                assert np.array_equal(found, cr.apply(cr.channel_mean(array) if c > 1 else array, CLIP, GRID)[0])
                checked = True
            calls, splits = [], []
            for _ in range(args.reps):
                t = time.perf_counter()
                _lib.stage_clahe(array, CLIP, GRID)
                calls.append(1e3 * (time.perf_counter() - t))
            for _ in range(args.reps):
                splits.append(_lib.stage_clahe(array, CLIP, GRID, return_times=True)[1])
            med = {k: statistics.median(s[k] for s in splits) for k in splits[0]}
            nbytes = kernel_bytes(w, h, c)
            share = {k: nbytes[k] / (med[k] * 1e-3) / PEAK if med[k] > 0 else None for k in nbytes}
            out[name] = {"channels": c, "call_ms": statistics.median(calls), "call_ms_all": calls, **med,
                         "kernels_ms": med["histogram_ms"] + med["lut_ms"] + med["apply_ms"], "algorithmic_bytes": nbytes,
                         "share_of_8TBs": share}
            print(f"{w}x{h}", name, json.dumps(out[name]), flush=True)
    return res


def restatement(args):
    res = {"what": "tests/clahe_restated.py (NumPy %s, one core), gray; the RGB figure adds mean(axis=2).astype(uint8)"
                   % np.__version__, "repetitions": args.reps, "sizes": {}}
    for w, h in args.sizes:
        both = frames(w, h)
        times, mean_times = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            cr.apply(both["gray"], CLIP, GRID)
            times.append(time.perf_counter() - t)
            t = time.perf_counter()
            both["rgb"].mean(axis=2).astype(np.uint8)
            mean_times.append(time.perf_counter() - t)
        res["sizes"][f"{w}x{h}"] = {"pixels": w * h, "seconds": statistics.median(times), "all_s": times,
                                    "host_mean_seconds": statistics.median(mean_times)}
        print(f"{w}x{h}", json.dumps(res["sizes"][f"{w}x{h}"]), flush=True)
    return res


def size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=size, nargs="+", default=[(640, 480), (1920, 1080), (4000, 3000)])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restatement", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clahe_probe.json"))
    a = ap.parse_args()
    result = restatement(a) if a.restatement else {**gpu(a), "restatement_cpu": restatement(a)}
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")
