"""Times of Image.project / Observer.project on one GPU, and of the reference's Image.project on the CPU.

    python tools/reproject_probe.py [--frames 64] [--reps 5] [--out profiles/reproject_probe.json]
    python tools/reproject_probe.py --reference [--out profiles/reproject_reference_cpu.json]   (needs the reference)

The GPU figures: a 2048 x 2048 RGB uint8 frame with the full camera model, resampled into an ideal camera turned by
1.5 degrees (`ideal`) and into a camera that is itself distorted (`distorted`: 20 undistortion iterations per pixel).
Every figure is the median of `--reps` repetitions, each repetition the SECOND of two back-to-back runs (an idle device
starts slowly).  `kernel_ms` is the sum of the kernels' durations from HIP events inside the library call;
`copy_ms_per_frame` is one frame up and one frame down through pinned memory (torch), for comparison: the batch form is
expected to be bound by those copies, not by the kernel.
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

SIZE = 2048
FULL = dict(f=(2600.0, 2650.0), c=(12.5, -8.0), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.005), p=(0.001, -0.002),
            xyz=(1.0, 2.0, 3.0))


def frame_of(seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:SIZE, 0:SIZE].astype(np.float32)
    z = np.stack([0.4 * np.sin(0.02 * x + c) + 0.4 * np.cos(0.03 * y - c) for c in range(3)], axis=2)
    return np.floor((z + 0.2 * rng.random(z.shape, dtype=np.float32) + 0.8) / 1.81 * 256.0).astype(np.uint8)


def second_of_two(fn):
    fn()
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def gpu(args):
    import torch

    from glimpse_amd import Camera, Image, Observer, _lib

    t0 = datetime.datetime(2020, 1, 1)
    targets = {"ideal": Camera(imgsz=(SIZE, SIZE), f=FULL["f"], xyz=FULL["xyz"], viewdir=(11.5, 5.7, 1.0)),
               "distorted": Camera(imgsz=(SIZE, SIZE), viewdir=(11.5, 5.7, 1.0), **FULL)}
    base = frame_of(0)
    images = [Image(cam=Camera(imgsz=(SIZE, SIZE), viewdir=(10.0 + 0.5 * np.sin(i), 5.0 + 0.3 * np.cos(i), 2.0), **FULL),
                    array=np.roll(base, 7 * i, axis=1), datetime=t0 + datetime.timedelta(days=i)) for i in range(args.frames)]
    obs = Observer(images)
    stack = np.stack([img.read() for img in images])
    cams = np.stack([img.cam.vector24 for img in images])
    res = {"device": torch.cuda.get_device_name(0), "frame": [SIZE, SIZE, 3], "dtype": "uint8", "frames": args.frames,
           "repetitions": args.reps, "rule": "median of repetitions, each the second of two back-to-back runs"}
    for name, cam in targets.items():
        one, batch, call, kernel = [], [], [], []
        for _ in range(args.reps):
            one.append(second_of_two(lambda: images[0].project(cam))[0])
            batch.append(second_of_two(lambda: obs.project(cam))[0])
            dt, (_, ms) = second_of_two(lambda: _lib.stage_reproject(stack, cams, cam.vector24, cam.imgsz, "linear",
                                                                     return_kernel_ms=True))
            call.append(dt)
            kernel.append(ms)
        res[name] = {"image_project_ms": 1e3 * statistics.median(one),
                     "observer_project_frames_per_s": args.frames / statistics.median(batch),
                     "library_call_frames_per_s": args.frames / statistics.median(call),
                     "library_call_ms_per_frame": 1e3 * statistics.median(call) / args.frames,
                     "kernel_ms_per_frame": statistics.median(kernel) / args.frames}
    # one frame up and one down through pinned memory, alone
    host = torch.empty(base.size, dtype=torch.uint8).pin_memory()
    dev = torch.empty(base.size, dtype=torch.uint8, device="cuda")
    copies = []
    for _ in range(args.reps):
        for k in range(2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dev.copy_(host, non_blocking=True)
            host.copy_(dev, non_blocking=True)
            b.record()
            torch.cuda.synchronize()
        copies.append(a.elapsed_time(b))
    res["copy_ms_per_frame"] = statistics.median(copies)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings

    import refstubs

    glimpse = refstubs.import_reference()
    src = glimpse.Camera(imgsz=(SIZE, SIZE), viewdir=(10.0, 5.0, 2.0), **FULL)
    targets = {"ideal": glimpse.Camera(imgsz=(SIZE, SIZE), f=FULL["f"], xyz=FULL["xyz"], viewdir=(11.5, 5.7, 1.0)),
               "distorted": glimpse.Camera(imgsz=(SIZE, SIZE), viewdir=(11.5, 5.7, 1.0), **FULL)}
    img = glimpse.Image("synthetic", cam=src, datetime=datetime.datetime(2020, 1, 1))
    img.array = frame_of(0)
    res = {"what": "the reference's Image.project (NumPy + SciPy, one core)", "frame": [SIZE, SIZE, 3], "dtype": "uint8",
           "repetitions": args.reps, "threads": os.cpu_count()}
    for name, cam in targets.items():
        times = []
        for _ in range(args.reps):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t = time.perf_counter()
                img.project(cam)
                times.append(time.perf_counter() - t)
        res[name] = {"image_project_s": statistics.median(times)}
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
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
