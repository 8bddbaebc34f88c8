"""Times of Camera.xyz_map on one GPU, and of the rule's NumPy restatement on one CPU core.

    python tools/raycast_probe.py [--reps 5] [--out profiles/raycast_probe.json]

Two shapes: a 4000 x 3000 frame over a 2000 x 2000 DEM (`large`, 12 million rays) and a 1920 x 1080 frame over a
500 x 500 DEM (`small`); cells of 2 m, rolling terrain, a camera with the full distortion model and an elevation
correction above the DEM's southern edge looking north and down at 25 degrees, so that the lower rows hit the terrain
nearby and the upper ones cross the whole DEM and leave it.  Each shape is cast at `block = 0` (every patch marched) and
at `block = 16` (the Python default), the two alternating in the same process; every figure is the median of `--reps`
calls after one warm-up call of each.

* `call_ms`: one `Camera.xyz_map(dem, return_depth=True)` call, wall time (allocations, copies, kernels).
* `upload_ms`, `pyramid_ms`, `march_ms`, `download_ms`: the split of one library call by HIP events (the DEM in; the block
  maxima; the march; t, xyz, patch and status out, through pageable memory).
* `equal_to_block_0`: the four result arrays of `block = 16` equal those of `block = 0` in every byte.
* `cpu`: tests/raycast_rule.py, with NumPy held to one thread, on the pixel centres `cpu_step` apart of the small shape --
  a size it finishes -- at both block sizes, and whether the device returns its bytes for those rays.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"  # (the restatement on one core; set before NumPy loads)

import argparse  # noqa: E402
import json  # noqa: E402
import statistics  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import raycast_rule  # noqa: E402

CELL = 2.0
SHAPES = {"large": (2000, (4000, 3000)), "small": (500, (1920, 1080))}
BLOCKS = (0, 16)


def scene(n, size):
    from glimpse_amd import Camera, Raster

    x = (np.arange(n) + 0.5) * CELL
    y = x[::-1].copy()
    X, Y = np.meshgrid(x, y)
    L = n * CELL
    z = 0.05 * Y + 0.02 * L * np.sin(7.0 * X / L) * np.cos(5.0 * Y / L) + 0.01 * L * np.sin(23.0 * (X + Y) / L)
    w, h = size
    cam = Camera(imgsz=size, f=(0.9 * w, 0.9 * w), c=(0.004 * w, -0.003 * h), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.005),
                 p=(0.001, -0.002), xyz=(0.503 * L, 0.021 * L, 0.15 * L), viewdir=(1.5, -25.0, 0.7), correction=True)
    return Raster(z, x=x, y=y), cam


def same(a, b):
    return all(np.array_equal(u, v, equal_nan=u.dtype.kind == "f") for u, v in zip(a, b))


def shape(name, reps):
    from glimpse_amd import _lib

    n, size = SHAPES[name]
    dem, cam = scene(n, size)
    res = {"dem": [n, n], "frame": list(size), "rays": size[0] * size[1]}
    wall = {b: [] for b in BLOCKS}
    split = {b: [] for b in BLOCKS}
    results = {}
    for k in range(reps + 1):
        for b in BLOCKS:  # (alternating: what else runs on the machine meets both alike)
            t = time.perf_counter()
            cam.xyz_map(dem, return_depth=True, block=b)
            elapsed = time.perf_counter() - t
            *arrays, times = dem._cast_rays(cam.correction, b, return_times=True, cam=cam.vector24, step=1)
            if k:
                wall[b].append(1e3 * elapsed)
                split[b].append(times)
            else:
                results[b] = arrays
    for b in BLOCKS:
        entry = {"call_ms": statistics.median(wall[b])}
        for key in _lib.RAYCAST_TIMES:
            entry[key] = statistics.median(s[key] for s in split[b])
        entry["march_ms_min_max"] = [min(s["march_ms"] for s in split[b]), max(s["march_ms"] for s in split[b])]
        res[f"block_{b}"] = entry
    status = results[0][3]
    res["status_share"] = {s: float((status == k).mean()) for k, s in enumerate(_lib.RAYCAST_STATUS)}
    res["equal_to_block_0"] = same(results[0], results[16])
    res["march_speedup_block_16"] = res["block_0"]["march_ms"] / res["block_16"]["march_ms"]
    res["call_speedup_block_16"] = res["block_0"]["call_ms"] / res["block_16"]["call_ms"]
    return res


def cpu(step):
    from glimpse_amd import _lib

    n, size = SHAPES["small"]
    dem, cam = scene(n, size)
    uv = raycast_rule.grid_uv(size, step).reshape(-1, 2)
    d = _lib.stage_unproject(cam.vector24, uv)
    grid = (dem.array, float(dem.x[0]), float(dem.y[0]), float(dem.d[0]), float(dem.d[1]))
    correction = (cam.correction["radius"], cam.correction["refraction"])
    res = {"dem": [n, n], "cpu_step": step, "rays": len(uv)}
    got = dem._cast_rays(cam.correction, 16, cam=cam.vector24, uv=uv)
    for b in BLOCKS:
        t = time.perf_counter()
        want = raycast_rule.cast(np.array(cam.xyz), d, *grid, correction=correction, block=b)
        res[f"block_{b}_s"] = time.perf_counter() - t
        res[f"block_{b}_device_equal"] = same(want, got)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--cpu-step", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    result = {"device": torch.cuda.get_device_name(0), "repetitions": a.reps,
              "rule": "median of repetitions after one warm-up call of each block size, the block sizes alternating"}
    for name in a.shapes:
        result[name] = shape(name, a.reps)
        print(name, json.dumps(result[name]), flush=True)
    result["cpu"] = cpu(a.cpu_step)
    print("cpu", json.dumps(result["cpu"]), flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(json.dumps(result, indent=1) + "\n")
