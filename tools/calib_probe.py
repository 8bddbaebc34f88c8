"""Times of optimize.Cameras on one GPU, and of the same residuals evaluated control by control on one CPU core.

    python tools/calib_probe.py [--cameras 50] [--width 4000] [--observed 2000] [--matches 2000] [--reps 5]
                                [--out profiles/r17_calib_probe.json]

The case: `--cameras` cameras at one position, view directions 4 degrees apart, `--width` x 3/4 `--width` pixels,
f = 0.875 `--width`, radial and tangential distortion.  Each camera has a Lines control -- a horizon of 721 world vertices
all round, projected at density 1 (about one point per pixel of image width) against `--observed` traced points -- and a
Points control of 15 surveyed points; neighbours share a Matches control of `--matches` matches.  Observations come from
the true cameras plus N(0, 0.3 px); the fit starts N(0, 0.3 deg) and 2 % of f off the truth and fits every camera's
viewdir and one f for all: 3 `--cameras` + 2 parameters.

GPU figures (wall times are medians of `--reps`; the split is the library's HIP events of one call, plus the host's
segment tables):
  residual_ms   one `Cameras.residuals()` through the open handle: every control at one set of cameras
  jacobian_ms   one `Cameras.jacobian()`: every (control, parameter) block the sparsity marks, one device call;
                `jacobian_jobs` says how many, `jacobian_split_ms` where the time goes
  fit_s         a whole `Cameras.fit()` (upload included), with its nfev
  sequential_residual_ms   the same residuals control by control, each `predicted()` a device call of its own
CPU figure: `cpu_residual_ms`, the residuals by tests/calib_restated.py and oracle.camera (NumPy, one core), the
reference's loop over the controls.  Nothing here asserts a speed.
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

from tests import calib_restated as rs  # noqa: E402


def build(n_cams, width, n_observed, n_matches, seed=1):
    import glimpse_amd
    from glimpse_amd.optimize import Cameras, Lines, Matches, Points

    rng = np.random.default_rng(seed)
    internals = dict(imgsz=(width, 3 * width // 4), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))
    f_true = 0.875 * width
    true_viewdirs = np.column_stack((4.0 * np.arange(n_cams), np.full(n_cams, 2.0), np.zeros(n_cams))) + rng.normal(0, 0.3, (n_cams, 3))
    start_viewdirs = true_viewdirs + rng.normal(0, 0.3, (n_cams, 3))
    az = np.deg2rad(np.linspace(-180, 180, 721))
    horizon = np.column_stack((5000 * np.sin(az), 5000 * np.cos(az), 300 + 120 * np.sin(7 * az) + 40 * np.cos(31 * az)))
    true = [glimpse_amd.Camera(f=f_true, viewdir=v, **internals) for v in true_viewdirs]
    cams = [glimpse_amd.Camera(f=1.02 * f_true, viewdir=v, **internals) for v in start_viewdirs]
    controls, n_projected = [], []
    for i in range(n_cams):
        puv = np.vstack(Lines(true[i], uvs=[np.zeros((1, 2))], xyzs=[horizon])._xyzs_to_uvs())
        n_projected.append(len(puv))
        traced = puv[rng.choice(len(puv), n_observed)] + rng.normal(0, 0.3, (n_observed, 2))
        uv = rng.uniform((0.1 * width, 0.1 * width), (0.9 * width, 0.65 * width), (15, 2))
        xyz = true[i].uv_to_xyz(uv, directions=False, depth=rng.uniform(500, 3000, 15))
        controls += [Points(cams[i], uv=uv + rng.normal(0, 0.3, uv.shape), xyz=xyz), Lines(cams[i], uvs=[traced], xyzs=[horizon])]
    for i in range(n_cams - 1):
        uv_i = rng.uniform((0.55 * width, 0.1 * width), (0.95 * width, 0.65 * width), (n_matches, 2))
        uv_j = true[i + 1].xyz_to_uv(true[i].uv_to_xyz(uv_i), directions=True)
        controls.append(Matches(cams=[cams[i], cams[i + 1]], uvs=[uv_i + rng.normal(0, 0.3, uv_i.shape),
                                                                  uv_j + rng.normal(0, 0.3, uv_j.shape)]))
    model = Cameras(cams, controls, cam_params=[{"viewdir": True}] * n_cams, group_params={"f": True})
    return model, horizon, n_projected


def median_ms(f, reps):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def cpu_residuals(model, horizon):
    """The residuals control by control in NumPy: oracle.camera for points and matches, the restatement for lines."""
    from glimpse_amd.optimize import Lines, Points
    from oracle import camera as oc

    rows = []
    for control in model.controls:
        if isinstance(control, Lines):
            cam = control.cam.vector24
            rows.append(rs.lines_predicted(cam, oc.rotation_matrix(cam[3:6]), control.uv, [horizon], rs.clip_box(cam)) - control.uv)
        elif isinstance(control, Points):
            rows.append(oc.xyz_to_uv(control.cam.vector24, control.xyz) - control.uv)
        else:
            a, b = (cam.vector24 for cam in control.cams)
            d = oc.uv_to_xyz(b, control.uvs[1]) + a[0:3]  # (rays as points one unit from the shared position)
            rows.append(oc.xyz_to_uv(a, d) - control.uvs[0])
    return np.vstack(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=50)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--observed", type=int, default=2000)
    ap.add_argument("--matches", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_calib_probe.json"))
    args = ap.parse_args()
    model, horizon, n_projected = build(args.cameras, args.width, args.observed, args.matches)
    out = {"tool": "tools/calib_probe.py", "when": datetime.datetime.now().isoformat(timespec="seconds"),
           "case": {"cameras": args.cameras, "width": args.width, "observed_per_line": args.observed,
                    "matches_per_pair": args.matches, "parameters": len(model.params), "control_points": int(model.size),
                    "projected_per_line_min_max": [min(n_projected), max(n_projected)]}, "reps": args.reps}
    out["sequential_residual_ms"] = median_ms(model.residuals, max(1, args.reps // 2))
    with model.upload() as handle:
        through = model.residuals()
        out["residual_ms"] = median_ms(model.residuals, args.reps)
        _, split = model._evaluate(handle, [[cam._vector for cam in model.cams]], [(i, 0) for i in range(len(model.controls))],
                                   return_times=True)
        out["residual_split_ms"] = split
        model.jacobian()
        out["jacobian_ms"] = median_ms(model.jacobian, args.reps)
        J, split = model.jacobian(return_times=True)
        out["jacobian_split_ms"] = split
        out["jacobian_jobs"] = len(model._jacobian_plan()[2])
        out["jacobian_nonzeros"] = int(J.nnz)
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        result = model.fit(full=True)
    out["fit_s"] = time.perf_counter() - t0
    out["fit"] = {"success": bool(result.success), "nfev": int(result.nfev), "njev": int(result.njev),
                  "rmse_start_px": float(np.sqrt((model.errors() ** 2).mean())),
                  "rmse_fit_px": float(np.sqrt((model.errors(params=result.x) ** 2).mean()))}
    t0 = time.perf_counter()
    cpu = cpu_residuals(model, horizon)
    out["cpu_residual_ms"] = (time.perf_counter() - t0) * 1e3
    with np.errstate(invalid="ignore"):
        out["cpu_against_gpu_max_abs_px"] = float(np.nanmax(np.abs(cpu - through)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
