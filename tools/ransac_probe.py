"""Times of optimize.ransac over a Cameras model on one GPU: the host loop (`batched=False`, the reference's, one
`Cameras.fit` after the other) against `batched=True` (every sample fitted and scored in one device call, every distinct
consensus set refitted in a second one).

    python tools/ransac_probe.py [--reps 5] [--warmup 1] [--box "AMD Instinct MI355X"] [--out profiles/ransac_probe.json]

Two shapes:
  scenario   the reference's own test of optimize on a synthetic frame of 400 x 268: the frame projected into a camera
             turned by (2, 2, 2), SIFT on both, matched with max_ratio=0.8; ransac(n=12, max_error=5, min_inliers=10,
             iterations=10) over Cameras(viewdir) of the turned camera
  matches    2 000 designed matches between two cameras at one position, 30 % of them outliers displaced by 20 .. 60 px,
             the rest with N(0, 0.3 px); ransac(n=12, max_error=3, min_inliers=100, iterations=100), fitting viewdir

Per shape, after `--warmup` calls of each path, the median wall time of `--reps` calls under one np.random.seed:
  host_ms      ransac(batched=False)
  batched_ms   ransac(batched=True), and `batched_split_ms`, the medians of its parts: upload (the controls and each
               call's arguments), fit_score and refit (the library's HIP events of the two device calls), download, host
               (sorting the hypotheses into distinct sets), final_fit (the host's `Cameras.fit` on the winning set and
               whatever sets it had to try before) and calls (the wall time of the two library calls, events included)
  distinct_sets, hypotheses, converged   what the refit saw
`device` is the runtime's name for the GPU, `box` the caller's (`--box`: the runtime does not always know the product
name).  Nothing here asserts a speed.
"""
import argparse
import contextlib
import copy
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


def scenario():
    import glimpse_amd
    from glimpse_amd import optimize, synth

    frame = synth.make_texture(400, seed=3)[:268].astype(np.uint8)
    a = glimpse_amd.Image(cam=glimpse_amd.Camera(imgsz=(400, 268), f=(480, 480)), array=frame, datetime=datetime.datetime(2020, 1, 1))
    b = copy.deepcopy(a)
    b.cam.viewdir = (2, 2, 2)
    keypoints = [optimize.detect_keypoints(x, method=optimize.SIFT) for x in (a.read(), a.project(b.cam)[:, :, 0])]
    uvs = optimize.match_keypoints(*keypoints, max_ratio=0.8)
    model = optimize.Cameras(cams=[b.cam], controls=[optimize.Matches(cams=(a.cam, b.cam), uvs=uvs)], cam_params=[{"viewdir": True}])
    return model, dict(n=12, max_error=5, min_inliers=10, iterations=10)


def matches(rows=2000, outliers=0.3, seed=1):
    import glimpse_amd
    from glimpse_amd import optimize
    from oracle import camera as oc

    rng = np.random.default_rng(seed)
    internals = dict(imgsz=(4000, 3000), f=(3500, 3500), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))
    true, other = (oc.make_camera(viewdir=v, **internals) for v in ((12.0, -6.0, 3.0), (15.5, -4.0, 1.0)))
    uv1 = rng.uniform((200, 200), (3800, 2800), (rows, 2))
    uv0 = oc.xyz_to_uv(true, oc.uv_to_xyz(other, uv1))
    out = rng.random(rows) < outliers
    angle, length = rng.uniform(0, 2 * np.pi, rows), rng.uniform(20, 60, rows)
    uv0 += np.where(out[:, None], np.column_stack((np.cos(angle), np.sin(angle))) * length[:, None], rng.normal(0, 0.3, (rows, 2)))
    fitted = glimpse_amd.Camera(viewdir=(12.8, -6.5, 3.4), **internals)
    model = optimize.Cameras([fitted], [optimize.Matches(cams=[fitted, glimpse_amd.Camera(viewdir=other[3:6], **internals)],
                                                         uvs=[uv0, uv1])], cam_params=[{"viewdir": True}])
    return model, dict(n=12, max_error=3, min_inliers=100, iterations=100)


def measure(model, call, reps, warmup, seed=0):
    from glimpse_amd import optimize

    def run(**kwargs):
        np.random.seed(seed)
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = optimize.ransac(model, **call, **kwargs)
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(warmup):
        run()
        run(batched=True)
    host = [run() for _ in range(reps)]
    batched = [run(batched=True, return_info=True) for _ in range(reps)]
    info = batched[-1][1][2]
    return {"rows": int(model.size), "call": call, "host_ms": statistics.median(t for t, _ in host),
            "host_ms_all": [t for t, _ in host], "batched_ms": statistics.median(t for t, _ in batched),
            "batched_ms_all": [t for t, _ in batched],
            "batched_split_ms": {key: statistics.median(float(out[2]["times_ms"][key]) for _, out in batched) for key in info["times_ms"]},
            "hypotheses": len(info["status"]), "converged": int((info["status"] > 0).sum()), "distinct_sets": len(info["sets"]),
            "inliers": [len(host[-1][1][1]), len(batched[-1][1][1])],
            "values": [host[-1][1][0].tolist(), batched[-1][1][0].tolist()]}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--box", default="", help="the machine's name, where the runtime's device name does not say it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_probe.json"))
    args = ap.parse_args()
    out = {"tool": "tools/ransac_probe.py", "when": datetime.datetime.now().isoformat(timespec="seconds"),
           "device": torch.cuda.get_device_name(0), "box": args.box, "reps": args.reps, "warmup": args.warmup}
    for name, make in (("scenario", scenario), ("matches", matches)):
        model, call = make()
        out[name] = measure(model, call, args.reps, args.warmup)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
