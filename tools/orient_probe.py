"""Times of optimize.ObserverCameras on one GPU, and of the same callback on one CPU core.

    python tools/orient_probe.py [--cases 40x2 1000x4] [--matches 2000] [--reps 5] [--out profiles/r14_orient_probe.json]
    python tools/orient_probe.py --reference [--out profiles/r14_orient_reference_cpu.json]   (needs the reference)

A case IxK is a synthetic sequence of I images at one position, each matched with its next K neighbours (pairs (i, i + 1)
.. (i + K)), `--matches` matches per pair: camera coordinates uniform in the frame of image i, carried through the true
view directions ([10, -3, 1] plus N(0, 0.3 deg) per image) into image j, plus N(0, 3e-4) (0.3 px at f = 1000) on both.
The fit starts N(0, 0.2 deg) off the truth with image 0 as anchor.

GPU figures: `eval_ms` is the wall time of one callback (`ObserverCameras.evaluate`: R and Rprime on the host, the
library call, the anchor term; median of `--reps`, each the second of two back-to-back calls) and the split is the
library's own HIP events inside such a call (upload / map / reduce / download).  `map_share_of_8TBps` is the map
kernel's algorithmic bytes (32 per match: two 16-byte loads) over its time, as a share of 8 TB/s.  `fit_s` is a whole
`fit` (upload of the matches included) with its nit and nfev; the large case is cut at `--maxiter`.  `cpu_eval_ms` is
tests/orient_restated.py's callback (NumPy, one core) on the same box; with --reference it is the reference's own closure,
on whatever machine runs it -- another than the GPU's host, so the two are set side by side, not divided.  Nothing here
asserts a speed.
"""
import argparse
import contextlib
import datetime
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import orient_restated as rs  # noqa: E402

INTERNALS = dict(imgsz=(800, 536), f=(1000, 1010), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))


def sequence(n_images, neighbours, n_matches, seed=1):
    """(true, start view directions, [(i, j, xy_i, xy_j)])"""
    from glimpse_amd.camera import rotations

    rng = np.random.default_rng(seed)
    true = np.array([10.0, -3.0, 1.0]) + rng.normal(0, 0.3, (n_images, 3))
    start = true + rng.normal(0, 0.2, (n_images, 3))
    R, _ = rotations(true)
    pairs = []
    for i in range(n_images):
        for j in range(i + 1, min(i + 1 + neighbours, n_images)):
            xy = rng.uniform((-0.36, -0.22), (0.36, 0.22), (n_matches, 2))
            d = np.column_stack((xy, np.ones(n_matches))) @ R[i]  # R_i^T x^
            c = d @ R[j].T
            pairs.append((i, j, xy + rng.normal(0, 3e-4, xy.shape), c[:, :2] / c[:, 2:3] + rng.normal(0, 3e-4, xy.shape)))
    return true, start, pairs


def model_of(start, pairs, package):
    """ObserverCameras of `package` (glimpse_amd, or the reference) on the sequence."""
    cams = [package.Camera(viewdir=v, **INTERNALS) for v in start]
    if package.__name__ == "glimpse_amd":
        images = [package.Image(cam=cam, array=np.zeros((2, 2), np.uint8),
                                datetime=datetime.datetime(2020, 1, 1) + datetime.timedelta(minutes=n))
                  for n, cam in enumerate(cams)]
        matches = {(i, j): package.optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], xys=[a, b]) for i, j, a, b in pairs}
    else:
        import make_golden_orient as mg

        images = [package.Image("synthetic", cam=cam, datetime=datetime.datetime(2020, 1, 1) + datetime.timedelta(minutes=n))
                  for n, cam in enumerate(cams)]
        # (the reference wants image coordinates to exist; it computes with the camera coordinates)
        matches = mg.coo_of([package.optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], uvs=[a, b], xys=[a, b])
                             for i, j, a, b in pairs], [(i, j) for i, j, _, _ in pairs])
    return package.optimize.ObserverCameras(package.Observer(images), matches=matches, anchors=[0])


def gpu(args):
    import torch

    import glimpse_amd
    from glimpse_amd import _lib
    from glimpse_amd.camera import rotations

    res = {"device": torch.cuda.get_device_name(0), "repetitions": args.reps, "matches_per_pair": args.matches,
           "rule": "median of repetitions, each the second of two back-to-back calls", "cases": {}}
    for case in args.cases:
        n_images, neighbours = (int(v) for v in case.split("x"))
        true, start, pairs = sequence(n_images, neighbours, args.matches)
        model = model_of(start, pairs, glimpse_amd)
        n_matches = sum(len(p[2]) for p in pairs)
        t = time.perf_counter()
        handle = model.upload()
        upload_s = time.perf_counter() - t
        calls, splits = [], []
        R, Rprime = rotations(start)
        for _ in range(args.reps):
            model.evaluate(handle, start)
            t = time.perf_counter()
            objective, _ = model.evaluate(handle, start)
            calls.append(time.perf_counter() - t)
            splits.append(handle.eval(R, Rprime, return_times=True)[2])
        handle.close()
        med = {k + "_ms": statistics.median(s[k] for s in splits) for k in _lib.ORIENT_TIMES}
        t = time.perf_counter()
        cpu_objective, _ = rs.callback(start, start, [0], 1e6, pairs, rotations)
        cpu_s = time.perf_counter() - t
        options = {"maxiter": args.maxiter} if n_images > 100 else {}
        t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            result = model.fit(options=options)
        fit_s = time.perf_counter() - t
        x = result.x.reshape(-1, 3)
        entry = {"images": n_images, "pairs": len(pairs), "matches": n_matches, "matches_upload_s": upload_s,
                 "eval_ms": 1e3 * statistics.median(calls), "eval_ms_all": [1e3 * c for c in calls], **med,
                 "map_share_of_8TBps": 32.0 * n_matches / (med["map_ms"] * 1e-3) / 8e12 if med["map_ms"] else None,
                 "cpu_eval_ms": 1e3 * cpu_s, "objective_equal_to_restatement": bool(objective == cpu_objective),
                 "fit_s": fit_s, "fit_options": options, "fit_nit": int(result.nit), "fit_nfev": int(result.nfev),
                 "fit_success": bool(result.success), "fit_fun": float(result.fun),
                 "start_error_deg": float(np.abs((start - start[0]) - (true - true[0])).max()),
                 "fit_error_deg": float(np.abs((x - x[0]) - (true - true[0])).max())}
        res["cases"][case] = entry
        print(case, json.dumps(entry), flush=True)
    return res


def reference(args):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_orient as mg

    res = {"what": "the reference's ObserverCameras callback (NumPy, one core), one evaluation at the start",
           "repetitions": args.reps, "matches_per_pair": args.matches, "cases": {}}
    for case in args.cases:
        n_images, neighbours = (int(v) for v in case.split("x"))
        _, start, pairs = sequence(n_images, neighbours, args.matches)
        model = model_of(start, pairs, mg.glimpse)
        times = []

        def timed(fun, x0, **kwargs):
            for _ in range(args.reps):
                t = time.perf_counter()
                fun(np.ravel(np.array(x0, dtype=float)))
                times.append(time.perf_counter() - t)
            return mg.scipy.optimize.OptimizeResult(success=True, x=np.ravel(x0), message="probe")

        mg.with_minimize(model, timed)
        res["cases"][case] = {"images": n_images, "pairs": len(pairs), "matches": sum(len(p[2]) for p in pairs),
                              "eval_ms": 1e3 * statistics.median(times)}
        print(case, json.dumps(res["cases"][case]), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["40x2", "1000x4"])
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=20)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = reference(a) if a.reference else gpu(a)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(text + "\n")
