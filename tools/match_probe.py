"""Times of one descriptor search (_lib.Matcher.knn2) on one GPU, on both paths, and of the same search in NumPy on one
CPU core of the same box.

    python tools/match_probe.py [--sizes 2000 20000] [--dim 128] [--reps 5] [--out profiles/r18_match_probe.json]

A size N is N x N descriptors of `--dim` elements: SIFT-like uint8 rows (a gamma law cut at 255), the train set noisy
copies of a random half of the query set's features, so that nearest neighbours are as near as real ones are.  The
integer path takes them as they are, the float path as float32 (`path="float"`); the two results are compared bit for bit.

Figures: the library's own HIP events (upload / prepare as measured when the sets were put; search / merge / download of
the call), median of `--reps` calls after one warm-up call.  `search_ops_share`: the operations the algorithm needs --
integer path 2 N N dim (multiply-adds of q.t, as two operations each) against the int8 MFMA peak of 5.0e15 /s (twice the
2.5e15 of bf16, MI355X_MICROARCH); float path 3 N N dim (subtract, multiply, add) against the FP32 vector peak of 157.3e12 /s
-- over the search kernel's time.  `cpu_ms`: float32 distances by |q|^2 + |t|^2 - 2 q.t' (one sgemm per 2000 queries)
and np.argpartition for the two smallest, the process pinned to one core; it is not tie-exact and is here for scale only.
cv2 is not installed, so the reference's own matcher cannot be timed.  Nothing here asserts a speed.
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

INT8_PEAK, FP32_PEAK = 5.0e15, 157.3e12


def descriptors(n, dim, seed=1):
    rng = np.random.default_rng(seed)
    q = np.minimum(rng.gamma(0.6, 40.0, (n, dim)), 255).astype(np.uint8)
    t = np.minimum(rng.gamma(0.6, 40.0, (n, dim)), 255).astype(np.uint8)
    shared = rng.permutation(n)[: n // 2]
    t[rng.permutation(n)[: n // 2]] = np.clip(q[shared].astype(int) + rng.integers(-8, 9, (n // 2, dim)), 0, 255)
    return q, t


def cpu_knn2(q, t, block=2000):
    q, t = q.astype(np.float32), t.astype(np.float32)
    tt = (t * t).sum(1)
    idx = np.empty((len(q), 2), np.int64)
    for a in range(0, len(q), block):
        qb = q[a:a + block]
        d2 = (qb * qb).sum(1)[:, None] + tt[None, :] - 2 * (qb @ t.T)
        two = np.argpartition(d2, 1, axis=1)[:, :2]
        order = np.argsort(np.take_along_axis(d2, two, axis=1), axis=1, kind="stable")
        idx[a:a + block] = np.take_along_axis(two, order, axis=1)
    return idx


def one_core(call, reps):
    cpus = os.sched_getaffinity(0)
    os.sched_setaffinity(0, {min(cpus)})
    try:
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = call()
            times.append((time.perf_counter() - t0) * 1e3)
    finally:
        os.sched_setaffinity(0, cpus)
    return out, statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from glimpse_amd import _lib

    result = {"dim": args.dim, "reps": args.reps, "int8_peak_ops": INT8_PEAK, "fp32_peak_flops": FP32_PEAK, "cases": []}
    with _lib.Matcher() as m:
        for n in args.sizes:
            q, t = descriptors(n, args.dim)
            case = {"n_q": n, "n_t": n}
            found = {}
            for path, ops, peak in (("integer", 2.0 * n * n * args.dim, INT8_PEAK), ("float", 3.0 * n * n * args.dim, FP32_PEAK)):
                assert m.put(0, q, path=None if path == "integer" else "float") == path
                m.put(1, t, path=None if path == "integer" else "float")
                m.knn2(0, 1)  # warm-up: the code object, the result buffers
                runs, wall = [], []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    *found[path], times = m.knn2(0, 1, return_times=True)
                    wall.append((time.perf_counter() - t0) * 1e3)
                    runs.append(times)
                split = {k + "_ms": statistics.median(r[k] for r in runs) for k in _lib.MATCH_TIMES}
                case[path] = {**split, "call_wall_ms": statistics.median(wall), "search_ops": ops,
                              "search_ops_per_s": ops / (split["search_ms"] * 1e-3),
                              "search_ops_share": ops / (split["search_ms"] * 1e-3) / peak}
            case["paths_agree_bit_for_bit"] = bool(np.array_equal(found["integer"][0], found["float"][0])
                                                   and np.array_equal(found["integer"][1], found["float"][1]))
            case["integer_over_float_search"] = case["float"]["search_ms"] / case["integer"]["search_ms"]
            if not args.no_cpu:
                idx, case["cpu_ms"] = one_core(lambda: cpu_knn2(q, t), args.reps)
                case["cpu_nearest_agrees"] = float((idx[:, 0] == found["integer"][0][:, 0]).mean())
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
