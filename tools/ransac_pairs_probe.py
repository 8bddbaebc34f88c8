"""Times of optimize.ransac_pairs on one GPU -- RANSAC over every image pair of a sequence in one device pass -- against the
way the same work was done before it: a Python loop of `ransac(..., batched=True)` over the pairs under the same seed.

    python tools/ransac_pairs_probe.py [--reps 5] [--warmup 1] [--loop-pairs 16] [--box "AMD Instinct MI355X"]
                                       [--out profiles/ransac_pairs_probe.json]

Two shapes:
  scenario   the reference's own test of optimize (tools/ransac_probe.py: scenario) replicated over 40 x 2 = 80 pairs, each
             with its own two cameras: n=12, max_error=5, min_inliers=10, iterations=10, viewdir
  sequence   1000 images x 4 neighbours = 3990 pairs of 2000 designed matches, 30 % of them outliers displaced by
             20 .. 60 px, the rest with N(0, 0.3 px): n=12, max_error=3, min_inliers=100, iterations=100, viewdir

Per shape, after `--warmup` calls, the medians of `--reps` calls under one np.random.seed:
  pairs_ms        the wall time of ransac_pairs, and `split_ms`, the medians of its `times_ms`: sampling (the host's
                  `_ransac_samples`), host (planning and packing), upload, fit, score, refit, final_score, download
  loop_ms         the loop of ransac(batched=True).  At the sequence shape it runs over the first `--loop-pairs` pairs only
                  and `loop_ms` is that time scaled by pairs / loop_pairs: `loop_pairs` and `loop_ms_measured` say so
  pairs, rows, hypotheses, accepted (refitted), winners, chunks
  device_samples  the same call with samples="device" (the seed words from np.random under the same np.random.seed), beside
                  the host leg: pairs_ms, split_ms (sampling: counting the hypotheses and enumerating short pairs on the
                  host; draw: the device's draw kernel), hypotheses, accepted, winners, inliers_mean, and `sampling_ms`
                  of both legs (sampling + draw)
`device` is the runtime's name for the GPU, `box` the caller's.  Nothing here asserts a speed.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def scenario(pairs=80):
    import glimpse_amd
    from glimpse_amd import optimize

    import ransac_probe

    model, call = ransac_probe.scenario()
    m = model.controls[0]
    out = {}
    for k in range(pairs):
        a, b = (glimpse_amd.Camera(viewdir=c.viewdir, imgsz=c.imgsz, f=c.f) for c in m.cams)
        out[2 * k, 2 * k + 1] = optimize.Matches(cams=(a, b), uvs=[uv.copy() for uv in m.uvs])
    return out, call


def sequence(images=1000, neighbours=4, rows=2000, outliers=0.3, seed=1):
    import glimpse_amd
    from glimpse_amd import optimize
    from oracle import camera as oc

    rng = np.random.default_rng(seed)
    internals = dict(imgsz=(4000, 3000), f=(3500, 3500), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))
    directions = np.array([12.0, -6.0, 3.0]) + np.cumsum(rng.normal(0, 0.3, (images, 3)), axis=0)
    true = [oc.make_camera(viewdir=v, **internals) for v in directions]
    cams = [glimpse_amd.Camera(viewdir=v + rng.normal(0, 0.3, 3), **internals) for v in directions]
    out = {}
    for i in range(images):
        for j in range(i + 1, min(i + 1 + neighbours, images)):
            uv1 = rng.uniform((200, 200), (3800, 2800), (rows, 2))
            uv0 = oc.xyz_to_uv(true[i], oc.uv_to_xyz(true[j], uv1))
            bad = rng.random(rows) < outliers
            angle, length = rng.uniform(0, 2 * np.pi, rows), rng.uniform(20, 60, rows)
            uv0 += np.where(bad[:, None], np.column_stack((np.cos(angle), np.sin(angle))) * length[:, None], rng.normal(0, 0.3, (rows, 2)))
            out[i, j] = optimize.Matches(cams=(cams[i], cams[j]), uvs=[uv0, uv1])
    return out, dict(n=12, max_error=3, min_inliers=100, iterations=100)


def measure(matches, call, reps, warmup, loop_pairs=None, seed=0):
    from glimpse_amd import optimize

    def pairs(**mode):
        np.random.seed(seed)
        t0 = time.perf_counter()
        out = optimize.ransac_pairs(matches, return_info=True, **call, **mode)
        return (time.perf_counter() - t0) * 1e3, out

    def split(runs):
        return {key: statistics.median(float(out[1]["times_ms"][key]) for _, out in runs) for key in runs[-1][1][1]["times_ms"]}

    subset = list(matches.values())[:loop_pairs]

    def loop():
        np.random.seed(seed)
        t0 = time.perf_counter()
        found = 0
        with contextlib.redirect_stdout(io.StringIO()):
            for m in subset:
                try:
                    optimize.ransac(optimize.Cameras([m.cams[1]], [m], cam_params=[{"viewdir": True}]), batched=True, **call)
                    found += 1
                except ValueError:
                    pass
        return (time.perf_counter() - t0) * 1e3, found

    for _ in range(warmup):
        pairs()
        pairs(samples="device")
        loop()
    new = [pairs() for _ in range(reps)]
    drawn = [pairs(samples="device") for _ in range(reps)]
    old = [loop() for _ in range(reps)]
    results, info = drawn[-1][1]
    device_split = split(drawn)
    device = {"pairs_ms": statistics.median(t for t, _ in drawn), "pairs_ms_all": [t for t, _ in drawn], "split_ms": device_split,
              "sampling_ms": device_split["sampling"] + device_split["draw"], "seed": info["seed"],
              "hypotheses": len(info["status"]), "converged": int((info["status"] > 0).sum()),
              "accepted": int((info["refit_status"] != -100).sum()), "winners": int((info["winner"] >= 0).sum()),
              "chunks": info["chunks"],
              "inliers_mean": float(np.mean([len(r[1]) for r in results if r is not None])) if any(r is not None for r in results) else 0.0}
    results, info = new[-1][1]
    measured = statistics.median(t for t, _ in old)
    accepted = int((info["refit_status"] != -100).sum())
    return {"pairs": len(matches), "rows": int(sum(m.size for m in matches.values())), "call": call,
            "pairs_ms": statistics.median(t for t, _ in new), "pairs_ms_all": [t for t, _ in new],
            "split_ms": split(new), "sampling_ms": split(new)["sampling"], "device_samples": device,
            "loop_pairs": len(subset), "loop_ms_measured": measured, "loop_ms_all": [t for t, _ in old],
            "loop_ms": measured * len(matches) / len(subset), "loop_scaled": len(subset) != len(matches),
            "loop_winners": old[-1][1],
            "hypotheses": len(info["status"]), "converged": int((info["status"] > 0).sum()), "accepted": accepted,
            "winners": int((info["winner"] >= 0).sum()), "chunks": info["chunks"],
            "inliers_mean": float(np.mean([len(r[1]) for r in results if r is not None])) if any(r is not None for r in results) else 0.0}


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-pairs", type=int, default=16, help="the pairs of the sequence shape that the loop runs over")
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--box", default="", help="the machine's name, where the runtime's device name does not say it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_pairs_probe.json"))
    args = ap.parse_args()
    out = {"tool": "tools/ransac_pairs_probe.py", "when": datetime.datetime.now().isoformat(timespec="seconds"),
           "device": torch.cuda.get_device_name(0), "box": args.box, "reps": args.reps, "warmup": args.warmup}
    matches, call = scenario()
    out["scenario"] = measure(matches, call, args.reps, args.warmup)
    print(json.dumps(out["scenario"]), flush=True)
    matches, call = sequence(images=args.images)
    out["sequence"] = measure(matches, call, args.reps, args.warmup, loop_pairs=args.loop_pairs)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
