"""Times of glimpse_amd.velocity_field on one GPU, and of the rule's NumPy restatement on one CPU core.

    python tools/velocity_field_probe.py [--reps 5] [--out profiles/velocity_field_probe.json]

Two shapes: `large`, 100 000 nodes (250 x 400) x 1000 pairs at radius 1, and `small`, 10 000 nodes (100 x 100) x 100 pairs
at radius 2.  The field is smooth with noise of 0.3 px; a tenth of the vectors are no candidates and a twentieth are
moved by some pixels.  Every figure is the median of `--reps` calls after one warm-up call.  No time is asserted anywhere.

* `call_ms`: one `glimpse_amd.velocity_field(duv, score, status, grid, ...)` call, wall time (checks, allocations, copies,
  both kernels).
* `upload_ms`, `test_ms`, `stack_ms`, `download_ms`: the split of one library call by HIP events (duv, score, status and
  dt in, through pageable memory; the neighbour test; the stack; v, sigma, count and kept out).
* `test_bytes`, `stack_bytes`: the algorithmic traffic -- the test reads duv, score and status of every pair and node
  once and writes kept (26 bytes a vector); the stack reads kept and duv (17 bytes a vector) and writes v, sigma and count
  (36 bytes a node) -- and `test_share_of_hbm`, `stack_share_of_hbm`: that over the kernel's time, over 8 TB/s.
* `kept_share`: the share of vectors kept.
* `cpu`: tests/velocity_field_rule.py, NumPy held to one thread.  `small` is run whole.  `large` is run on its first
  `cpu_rows` rows of nodes (all pairs) and the time scaled by rows / cpu_rows (`cpu_s_scaled`, `cpu_scaled_from_rows`);
  `cpu_device_equal`: the device, given the same input, returns the restatement's bytes.
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

from tests import velocity_field_rule  # noqa: E402

SHAPES = {"large": ((250, 400), 1000, 1, 10), "small": ((100, 100), 100, 2, 100)}  # grid, pairs, radius, cpu_rows
HBM_BYTES_PER_S = 8e12


def field(grid, pairs, seed=1):
    rng = np.random.default_rng(seed)
    rows, cols = grid
    n = rows * cols
    r, c = np.divmod(np.arange(n), cols)
    duv = np.empty((pairs, n, 2))
    truth = np.column_stack([3 + 0.015 * c + 0.005 * r, -2 + 0.01 * r - 0.002 * c])
    for p in range(pairs):  # (pair by pair: no second copy of 1.6 GB)
        duv[p] = truth + rng.normal(0.0, 0.3, size=(n, 2))
        wrong = rng.random(n) < 0.05
        duv[p, wrong] += rng.uniform(-9.0, 9.0, size=(int(wrong.sum()), 2))
    score = rng.uniform(0.2, 1.0, size=(pairs, n))
    status = (rng.random((pairs, n)) < 0.1).astype(np.uint8) * 4
    duv[status == 4] = np.nan
    dt = np.linspace(86400.0, 10 * 86400.0, pairs)
    return duv, score, status, dt


def shape(name, reps):
    import glimpse_amd
    from glimpse_amd import _lib

    grid, pairs, radius, cpu_rows = SHAPES[name]
    n = grid[0] * grid[1]
    duv, score, status, dt = field(grid, pairs)
    options = dict(radius=radius, min_neighbors=3, threshold=2.0, epsilon=0.1, min_count=1)
    wall, split = [], []
    for k in range(reps + 1):
        t = time.perf_counter()
        got = glimpse_amd.velocity_field(duv, score, status, grid, dt=dt, scale=(2.0, -2.0), return_kept=True, **options)
        elapsed = time.perf_counter() - t
        *_, times = _lib.stage_velocity_field(duv, score, status, grid, dt, (2.0, -2.0), 0.0, True, radius, 3, 2.0, 0.1, 1,
                                              return_times=True)
        if k:
            wall.append(1e3 * elapsed)
            split.append(times)
    res = {"grid": list(grid), "nodes": n, "pairs": pairs, "radius": radius, "call_ms": statistics.median(wall)}
    for key in _lib.VELOCITY_FIELD_TIMES:
        res[key] = statistics.median(s[key] for s in split)
    res["test_bytes"], res["stack_bytes"] = 26 * pairs * n, 17 * pairs * n + 36 * n
    res["test_share_of_hbm"] = res["test_bytes"] / (1e-3 * res["test_ms"]) / HBM_BYTES_PER_S
    res["stack_share_of_hbm"] = res["stack_bytes"] / (1e-3 * res["stack_ms"]) / HBM_BYTES_PER_S
    res["kept_share"] = float(got[3].mean())
    m = cpu_rows * grid[1]
    sub = (duv[:, :m], score[:, :m], status[:, :m], (cpu_rows, grid[1]))
    t = time.perf_counter()
    want = velocity_field_rule.velocity_field(*sub, dt=dt, scale=(2.0, -2.0), **options)
    cpu_s = time.perf_counter() - t
    res["cpu_scaled_from_rows"] = None if cpu_rows == grid[0] else cpu_rows
    res["cpu_s_scaled"] = cpu_s * grid[0] / cpu_rows
    same = glimpse_amd.velocity_field(*sub, dt=dt, scale=(2.0, -2.0), return_kept=True, **options)
    res["cpu_device_equal"] = all(g.tobytes() == w.tobytes() for g, w in zip(same, want))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    result = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps,
              "rule": "median of repetitions after one warm-up call", "hbm_bytes_per_s": HBM_BYTES_PER_S}
    for name in args.shapes:
        result[name] = shape(name, args.reps)
        print(name, json.dumps(result[name]), flush=True)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(json.dumps(result, indent=1) + "\n")
