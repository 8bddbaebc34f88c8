"""Times of Image.orthorectify / Observer.orthorectify on one GPU, and of the rule's NumPy / SciPy restatement on the CPU.

    python tools/orthorectify_probe.py [--frames 20] [--reps 5] [--out profiles/orthorectify_probe.json]

Two shapes: a 2000 x 2000 DEM with 4000 x 3000 RGB uint8 frames (`large`) and a 500 x 500 DEM with 1920 x 1080 frames
(`small`); cells of 2 m, rolling terrain, a camera with the full distortion model above the DEM's southern edge looking
north and down, so that the frame's footprint lies inside the DEM.  Every GPU figure is the median of `--reps` calls
after one warm-up call of the same shape.

* `image_ms`: one `Image.orthorectify(dem, viewshed=visible)` call, wall time (allocation, copies and kernel).
* `observer_ms`: one `Observer.orthorectify` call over `--frames` frames with that viewshed, wall time.
* the split: `upload_ms` (the DEM, its coordinates, the mask and one frame, host to device through pinned memory, alone),
  `viewshed_ms` (one `dem.viewshed(cam.xyz)` call, what `viewshed=True` adds), `kernel_ms` (the kernel of one frame, from
  HIP events inside the library call), `download_ms` (one result, device to host through pinned memory, alone).
* `kernel_share_of_8TBs`: the algorithmic bytes -- the DEM, the mask, the output, and once every frame pixel a seen
  cell's sample reads -- over the kernel time, as a share of the 8 TB/s HBM peak.
* `rule_cpu_s`: tests/ortho_rule.py (NumPy + scipy's RegularGridInterpolator) on the host of the same machine, with the
  same viewshed; one run (`large`) or the median of three (`small`).
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import ortho_rule  # noqa: E402

CELL = 2.0
SHAPES = {"large": (2000, (4000, 3000)), "small": (500, (1920, 1080))}
PEAK = 8e12  # bytes / s


def terrain(n):
    x = (np.arange(n) + 0.5) * CELL
    y = x[::-1].copy()
    X, Y = np.meshgrid(x, y)
    L = n * CELL
    z = 0.05 * Y + 0.02 * L * np.sin(7.0 * X / L) * np.cos(5.0 * Y / L) + 0.01 * L * np.sin(23.0 * (X + Y) / L)
    return x, y, z


def camera(n, size):
    from glimpse_amd import Camera

    L = n * CELL
    w, h = size
    return Camera(imgsz=size, f=(0.9 * w, 0.9 * w), c=(0.004 * w, -0.003 * h), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.005),
                  p=(0.001, -0.002), xyz=(0.503 * L, 0.021 * L, 0.4 * L), viewdir=(1.5, -38.0, 0.7), correction=True)


def frames_of(size, n):
    w, h = size
    rng = np.random.default_rng(5)
    v, u = np.mgrid[0:h, 0:w].astype(np.float32)
    z = np.stack([0.4 * np.sin(0.02 * u + c) + 0.4 * np.cos(0.03 * v - c) for c in range(3)], axis=2)
    base = np.floor((z + 0.2 * rng.random(z.shape, dtype=np.float32) + 0.8) / 1.81 * 256.0).astype(np.uint8)
    return [np.roll(base, 7 * i, axis=1) for i in range(n)]


def timed(fn, reps):
    fn()  # (warm-up)
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return statistics.median(out)


def pinned_copy_ms(nbytes, to_device, reps):
    import torch

    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
    dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = []
    for k in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        (dev if to_device else host).copy_(host if to_device else dev, non_blocking=True)
        b.record()
        torch.cuda.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return statistics.median(out)


def shape(name, args):
    from glimpse_amd import Image, Observer, Raster, _lib

    n, size = SHAPES[name]
    x, y, z = terrain(n)
    dem = Raster(z, x=x, y=y)
    cam = camera(n, size)
    t0 = datetime.datetime(2020, 1, 1)
    images = [Image(cam=cam.copy(), array=f, datetime=t0 + datetime.timedelta(days=i))
              for i, f in enumerate(frames_of(size, args.frames))]
    for i, img in enumerate(images):  # (a view direction that wanders a little, as a time-lapse camera's does)
        img.cam.viewdir = cam.viewdir + (0.3 * np.sin(i), 0.2 * np.cos(i), 0.0)
    visible = dem.viewshed(cam.xyz, correction=cam.correction)
    seen = visible[None].view(np.uint8)
    frame, cams = images[0].read()[None], cam.vector24[None]
    res = {"dem": [n, n], "frame": [size[0], size[1], 3], "dtype": "uint8", "frames": args.frames}
    res["image_ms"] = 1e3 * timed(lambda: images[0].orthorectify(dem, viewshed=visible), args.reps)
    res["image_viewshed_true_ms"] = 1e3 * timed(lambda: images[0].orthorectify(dem, viewshed=True), args.reps)
    obs = Observer(images)
    res["observer_ms"] = 1e3 * timed(lambda: obs.orthorectify(dem, viewshed=visible), args.reps)
    res["observer_ms_per_frame"] = res["observer_ms"] / args.frames
    res["viewshed_ms"] = 1e3 * timed(lambda: dem.viewshed(cam.xyz, correction=cam.correction), args.reps)
    kernel = []
    for k in range(args.reps + 1):
        out, ms = _lib.stage_orthorectify(frame, cams, z, dem.x, dem.y, seen, None, "linear", return_kernel_ms=True)
        if k:
            kernel.append(ms)
    res["kernel_ms"] = statistics.median(kernel)
    up_bytes = z.nbytes + 8 * 2 * n + seen.nbytes + frame.nbytes
    res["upload_ms"] = pinned_copy_ms(up_bytes, True, args.reps)
    res["download_ms"] = pinned_copy_ms(out.nbytes, False, args.reps)
    # the frame pixels a seen cell's bilinear sample reads, each counted once
    valued = ~np.isnan(out[0, :, :, 0])
    X, Y = np.meshgrid(dem.x, dem.y)
    uv = cam.xyz_to_uv(np.column_stack((X[valued], Y[valued], z[valued])))
    iu = np.clip(np.floor(uv[:, 0] - 0.5).astype(np.int64), 0, size[0] - 2)
    iv = np.clip(np.floor(uv[:, 1] - 0.5).astype(np.int64), 0, size[1] - 2)
    touched = np.zeros((size[1], size[0]), dtype=bool)
    for du in (0, 1):
        for dv in (0, 1):
            touched[iv + dv, iu + du] = True
    res["valued_share"] = float(valued.mean())
    res["frame_pixels_read"] = int(touched.sum())
    res["algorithmic_bytes"] = int(z.nbytes + seen.nbytes + out.nbytes + 3 * touched.sum())
    res["kernel_share_of_8TBs"] = res["algorithmic_bytes"] / (1e-3 * res["kernel_ms"]) / PEAK
    cpu = []
    for _ in range(1 if name == "large" else 3):
        t = time.perf_counter()
        want = ortho_rule.orthorectify(cam, frame[0], dem.x, dem.y, z, viewshed=visible)[0]
        cpu.append(time.perf_counter() - t)
    res["rule_cpu_s"] = statistics.median(cpu)
    res["rule_cpu_nan_pattern_equal"] = bool((np.isnan(want) == np.isnan(out[0])).all())
    res["rule_cpu_max_abs_diff"] = float(np.nanmax(np.abs(want - out[0])))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    result = {"device": torch.cuda.get_device_name(0), "repetitions": a.reps, "cpu_threads": os.cpu_count(),
              "rule": "median of repetitions after one warm-up call"}
    for name in a.shapes:
        result[name] = shape(name, a)
        print(name, json.dumps(result[name]), flush=True)
    text = json.dumps(result, indent=1)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")
