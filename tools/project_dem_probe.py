"""Times Camera.project_dem: the device's call and its stages, and the reference on one CPU core.

    python tools/project_dem_probe.py [--sizes 1024,4096,10000] [--reps 5] [--out profiles/r08_project_dem_probe.json]
    python tools/project_dem_probe.py --reference [--sizes 1024] [--out profiles/r08_project_dem_reference_cpu.json]

A square DEM of 10 m cells (seeded terrain, repeated beyond 2048 cells a side) with one float32 value layer and the depth
map, into a 4288 x 2848 image from a camera that stands outside the DEM and looks across it; tiles of 256, overlap 1.
One warm-up call, then the median of `--reps` calls: the wall clock of the whole call (host preparation, transfers,
kernels) and the HIP-event split of the library.  `--reference` runs the reference package instead (it must be
importable through tools/refstubs.py), pinned to one core.
"""
import json
import os
import platform
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests import viewshed_terrain as vt  # noqa: E402

IMGSZ = (4288, 2848)


def scene(n):
    base = vt.terrain((min(n, 2048), min(n, 2048)), 2908)
    reps = -(-n // base.shape[0])
    z = np.tile(base, (reps, reps))[:n, :n] + np.linspace(0.0, 0.02 * n, n)[None, :]
    values = (np.random.default_rng(8).integers(0, 2 ** 16, size=(n, n)) / 16.0).astype(np.float32)
    side = 10.0 * n
    cam = dict(imgsz=IMGSZ, f=3000.0, xyz=(-0.35 * side, 0.5 * side + 3.0, float(z.max()) + 0.08 * side),
               viewdir=(90.0, -14.0, 0.0))
    return z, values, (0.0, side), (side, 0.0), cam


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def main():
    reference = "--reference" in sys.argv
    sizes = [int(v) for v in arg("--sizes", "1024" if reference else "1024,4096,10000").split(",")]
    reps = int(arg("--reps", "1" if reference else "5"))
    out = arg("--out", os.path.join(ROOT, "profiles", "r08_project_dem_reference_cpu.json" if reference
                                    else "r08_project_dem_probe.json"))
    results = []
    if reference:
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
        import refstubs

        glimpse = refstubs.import_reference()
    else:
        from glimpse_amd import Camera, Raster, _lib
    for n in sizes:
        z, values, xlim, ylim, cam_args = scene(n)
        if reference:
            cam, dem = glimpse.Camera(**cam_args), glimpse.Raster(z, x=xlim, y=ylim)
        else:
            cam, dem = Camera(**cam_args), Raster(z, x=xlim, y=ylim)
        walls, splits, img = [], [], None
        for k in range(reps + (0 if reference else 1)):
            t0 = time.perf_counter()
            if reference:
                img = cam.project_dem(dem, values=values, return_depth=True)
            else:
                tiles = dem.tile_indices((256, 256), (1, 1))
                rows = list(dict.fromkeys((i.start, i.stop) for i, _ in tiles))
                cols = list(dict.fromkeys((j.start, j.stop) for _, j in tiles))
                img, split = _lib.stage_project_dem(
                    cam.vector24, z, values[:, :, None], None,
                    cols, np.concatenate([dem._tile_coordinates(0, a, b) for a, b in cols]),
                    rows, np.concatenate([dem._tile_coordinates(1, a, b) for a, b in rows]), return_depth=True,
                    return_times=True)
            wall = (time.perf_counter() - t0) * 1e3
            if reference or k > 0:  # (the device's first call is the warm-up)
                walls.append(wall)
                if not reference:
                    splits.append(split)
        row = dict(cells=n * n, side=n, imgsz=IMGSZ, reps=len(walls), call_ms_median=float(np.median(walls)),
                   call_ms_all=[round(w, 3) for w in walls], pixels_hit=int(np.isfinite(img[:, :, -1]).sum()))
        if splits:
            row["split_median"] = {k: float(np.median([s[k] for s in splits])) for k in splits[0]}
        print(json.dumps(row), flush=True)
        results.append(row)
    doc = dict(what="reference Camera.project_dem, one CPU core" if reference else "glh_stage_project_dem, one MI355X",
               host=platform.processor() or platform.machine(), python=platform.python_version(), numpy=np.__version__,
               tile_size=(256, 256), tile_overlap=(1, 1), layers="one float32 value layer + depth", results=results)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("->", out)


if __name__ == "__main__":
    main()
