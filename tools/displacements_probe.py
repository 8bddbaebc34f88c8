"""Times of glimpse_amd.displacements on one GPU, and of the rule's NumPy restatement on one CPU core.

    python tools/displacements_probe.py [--reps 5] [--out profiles/displacements_probe.json]

Two frames of 4000 x 3000 pixels, white noise and its copy moved by (3, -2) pixels, as uint8 (the integer path) and as
float32 (the float path).  Two shapes: `wide`, 10 000 points with 31 x 31 templates and a reach of 16, and `dense`,
100 000 points with 15 x 15 templates and a reach of 8; the points are a regular grid over the frame's interior.  Every
figure is the median of `--reps` calls after one warm-up call.

* `call_ms`: one `glimpse_amd.displacements(a, b, uv, ...)` call, wall time (template boxes, stacking the two frames,
  allocations, copies, the kernel).
* `upload_ms`, `kernel_ms`, `download_ms`: the split of one library call by HIP events (both frames and the points in,
  through pageable memory; the kernel; duv, score and status out).
* `byte_products`: the algorithmic work, n (2 rx + 1) (2 ry + 1) products of a template and a window pixel per point, and
  `products_per_s` = that over `kernel_ms`.
* `share_of_packed_dot_peak` (integer path): `products_per_s` over the nominal rate of v_dot4_u32_u8, taken as the vector
  issue rate times four -- 256 CUs x 4 SIMDs x 32 lanes a cycle x 4 products x 2.4 GHz = 3.15e14 products/s.  The kernel
  also spends issue slots on v_alignbyte_b32, LDS reads and the running sums, so the share of that bound it can reach is
  below one half by construction.
* `recovered`: the share of points whose displacement is within half a pixel of (3, -2).
* `cpu`: tests/displacement_rule.py, NumPy held to one thread, on `cpu_points` points of each shape and path, scaled to
  the shape's point count (`cpu_s_scaled`), and whether the device returns its bytes for those points.
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

from tests import displacement_rule  # noqa: E402

FRAME = (3000, 4000)  # rows, cols
SHIFT = (3, -2)
SHAPES = {"wide": (10_000, (31, 31), (16, 16)), "dense": (100_000, (15, 15), (8, 8))}
PACKED_DOT_PEAK = 256 * 4 * 32 * 4 * 2.4e9


def frames(path):
    a = displacement_rule.noise_u8(FRAME, seed=1)
    b = displacement_rule.shifted(a, *SHIFT, seed=2)
    return (a, b) if path == "integer" else (a.astype(np.float32), b.astype(np.float32))


def grid(n, margin=64):
    rows, cols = FRAME
    nx = int(round(np.sqrt(n * (cols - 2 * margin) / (rows - 2 * margin))))
    ny = -(-n // nx)
    u, v = np.meshgrid(np.linspace(margin, cols - margin, nx), np.linspace(margin, rows - margin, ny))
    return np.column_stack([u.ravel(), v.ravel()])[:n]


def shape(name, path, reps, cpu_points):
    import glimpse_amd
    from glimpse_amd import _lib
    from glimpse_amd.displacements import template_boxes

    n, size, reach = SHAPES[name]
    a, b = frames(path)
    uv = grid(n)
    corners, inside = template_boxes(uv, size, FRAME)
    stack, pairs = np.stack([a, b]), np.array([[0, 1]], dtype=np.int32)
    wall, split = [], []
    for k in range(reps + 1):
        t = time.perf_counter()
        duv, score, status = glimpse_amd.displacements(a, b, uv, size=size, reach=reach)
        elapsed = time.perf_counter() - t
        *_, times = _lib.stage_displacements(stack, pairs, corners, inside.astype(np.uint8), None, size, reach,
                                             return_times=True)
        if k:
            wall.append(1e3 * elapsed)
            split.append(times)
    res = {"points": n, "template": list(size), "reach": list(reach), "frame": [FRAME[1], FRAME[0]],
           "call_ms": statistics.median(wall)}
    for key in _lib.DISPLACEMENTS_TIMES:
        res[key] = statistics.median(s[key] for s in split)
    res["kernel_ms_min_max"] = [min(s["kernel_ms"] for s in split), max(s["kernel_ms"] for s in split)]
    res["byte_products"] = n * size[0] * size[1] * (2 * reach[0] + 1) * (2 * reach[1] + 1)
    res["products_per_s"] = res["byte_products"] / (1e-3 * res["kernel_ms"])
    if path == "integer":
        res["share_of_packed_dot_peak"] = res["products_per_s"] / PACKED_DOT_PEAK
    res["status_share"] = {s: float((status == k).mean()) for k, s in enumerate(_lib.DISPLACEMENT_STATUS)}
    res["recovered"] = float((np.abs(duv - SHIFT) <= 0.5).all(axis=1).mean())
    pick = np.linspace(0, n - 1, cpu_points).astype(int)
    t = time.perf_counter()
    want = displacement_rule.displacements(a, b, uv[pick], size=size, reach=reach)
    cpu_s = time.perf_counter() - t
    res["cpu_points"] = cpu_points
    res["cpu_s_scaled"] = cpu_s * n / cpu_points
    res["cpu_device_equal"] = all(g[pick].tobytes() == w.tobytes() for g, w in zip((duv, score, status), want))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--cpu-points", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps,
              "rule": "median of repetitions after one warm-up call", "packed_dot_peak_products_per_s": PACKED_DOT_PEAK}
    for name in args.shapes:
        for path in ("integer", "float"):
            result[f"{name}_{path}"] = shape(name, path, args.reps, args.cpu_points)
            print(name, path, json.dumps(result[f"{name}_{path}"]), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(json.dumps(result, indent=1) + "\n")
