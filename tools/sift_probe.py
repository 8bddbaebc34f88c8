"""Times of one SIFT detection (_lib.Sift.detect) on one GPU by stage, and of the NumPy restatement on one CPU core.

    python tools/sift_probe.py [--sizes 640x480 1920x1080 4000x3000] [--cpu-size 256x192] [--reps 5]
                               [--out profiles/sift_probe.json]

An image is the seeded 512 x 512 texture of the tests (tests/sift_cases.py) tiled to the given size, every second tile
mirrored (drawing the texture itself at 4000 x 3000 takes minutes of CPU).  Figures: the library's own HIP
events (upload / base / pyramid / extrema / refine / describe / download), median of `--reps` calls after one warm-up call
(the first call of a size allocates the pyramid).  `blur_share`: the bytes the blur passes need by the algorithm -- every
pass reads a float32 layer once and writes one, two passes a blur, S + 2 blurs an octave plus the base's -- over the
`base` + `pyramid` time (which also holds the doubling, the decimations and the differences), against 8 TB/s.
`cpu_ms`: tests/sift_restated.py on `--cpu-size`, the process pinned to one core; cv2 is not installed, so the reference's
own detector cannot be timed.  Nothing here asserts a speed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def size(text):
    w, h = text.lower().split("x")
    return int(w), int(h)


def picture(w, h):
    import numpy as np

    from tests import sift_cases as sc

    tile = sc.texture(512, 512)
    tile = np.concatenate([tile, tile[:, ::-1]], axis=1)
    tile = np.concatenate([tile, tile[::-1]], axis=0)
    return np.ascontiguousarray(np.tile(tile, (-(-h // 1024), -(-w // 1024)))[:h, :w])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=size, default=[(640, 480), (1920, 1080), (4000, 3000)])
    ap.add_argument("--cpu-size", type=size, default=(256, 192))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sift_probe.json"))
    args = ap.parse_args()

    from glimpse_amd import _lib
    from tests import sift_cases as sc
    from tests import sift_restated as sr

    result = {"reps": args.reps, "hbm_peak_bytes_per_s": HBM_PEAK, "gpu": [], "cpu": None}
    S = 3
    with _lib.Sift() as sift:
        for w, h in args.sizes:
            img = picture(w, h)
            sift.detect(img)
            runs = [sift.detect(img, return_times=True) for _ in range(args.reps)]
            times = {k: statistics.median(r[2][k] for r in runs) for k in _lib.SIFT_TIMES}
            cells = sum(a * b for a, b in sr.octave_sizes(h, w))
            blur_bytes = (cells * (S + 2) + 4 * w * h) * 2 * 2 * 4  # blurs x passes x (read + write) x float32
            blur_ms = times["base"] + times["pyramid"]
            result["gpu"].append({"width": w, "height": h, "keypoints": len(runs[0][0]), "candidates": sift.counts()["candidates"],
                                  "octaves": sift.counts()["octaves"], "times_ms": times, "total_ms": sum(times.values()),
                                  "blur_bytes": blur_bytes, "blur_share": blur_bytes / (blur_ms * 1e-3) / HBM_PEAK})
            print(result["gpu"][-1], flush=True)
    w, h = args.cpu_size
    img = sc.texture(h, w)
    cpus = os.sched_getaffinity(0)
    os.sched_setaffinity(0, {min(cpus)})
    try:
        t = time.perf_counter()
        kps, _ = sr.detect(img)
        cpu_ms = (time.perf_counter() - t) * 1e3
    finally:
        os.sched_setaffinity(0, cpus)
    result["cpu"] = {"width": w, "height": h, "keypoints": len(kps), "cpu_ms": cpu_ms}
    print(result["cpu"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
