"""Generate tests/golden/calib_*.npz by RUNNING THE REFERENCE's optimize.Points, Lines, Cameras, ransac and Polynomial
(optimize.py:46-459, :985-2188), Camera.edges and the polyline helpers under the stub modules of tools/refstubs.py.
Build-container only; the fixtures hold inputs and the reference's outputs, no reference source.  Re-run with:
python tools/make_golden_calib.py

Two shims, both defined here, let the reference run on this NumPy and without lmfit; neither touches its arithmetic:
  * `np.math = math` (optimize._ransac_samples calls np.math.lgamma, which NumPy 2 no longer has);
  * a stand-in for lmfit: `Parameters` with `add` and `valuesdict`, and `minimize`, which hands `fcn` to
    scipy.optimize.least_squares with the parameters' bounds and the remaining keyword arguments and drops NaN rows for
    nan_policy="omit".  A stand-in, not lmfit: what it pins is the reference's residual function, scales, sparsity and
    bounds driven by SciPy's trust-region solver, which is also what lmfit's "least_squares" method runs.

  calib_helpers.npz  the helpers, Camera.edges, the static methods of Cameras, _ransac_samples(2, 4), ransac + Polynomial
  calib_lines.npz    Lines._xyzs_to_uvs (clip box, points per segment, points) and Lines.predicted for two cameras (with
                     and without k[3:6] and p) x two controls: [in frame, leaving and re-entering, vertices behind the
                     camera, shorter than a step] and [wholly out of frame: the fallback]
  calib_fit.npz      three cameras at one position, each with a Points and a Lines control, and Matches between
                     neighbours: `predicted` of every control at the start, scales, sparsity, and the fit of per-camera
                     viewdir and a group f from the Points and Lines (11 parameters)

The nearest projected point must be unambiguous: every observed point's relative gap between the nearest and the
second-nearest squared distance must exceed 1e-9 (asserted here; the seeds were chosen so that the reference passes).
"""
import contextlib
import io
import math
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refstubs  # noqa: E402
import scipy.optimize  # noqa: E402

np.math = math


class Parameters(dict):
    def add(self, name, value=None, vary=True, min=-np.inf, max=np.inf):
        self[name] = types.SimpleNamespace(value=float(value), min=float(min), max=float(max))

    def valuesdict(self):
        return {name: p.value for name, p in self.items()}


def minimize(fcn, params, kws=None, iter_cb=None, method="least_squares", nan_policy="raise", **kwargs):
    assert method == "least_squares"
    names = list(params)
    count = [0]

    def fun(x):
        for name, value in zip(names, x):
            params[name].value = float(value)
        out = fcn(params, **(kws or {}))
        count[0] += 1
        if iter_cb is not None:
            iter_cb(params, count[0], out)
        r = np.asarray(out).ravel()
        return r[~np.isnan(r)] if nan_policy == "omit" else r

    x0 = np.array([params[name].value for name in names])
    bounds = (np.array([params[name].min for name in names]), np.array([params[name].max for name in names]))
    result = scipy.optimize.least_squares(fun, x0, bounds=bounds, **kwargs)
    final = Parameters()
    for name, value in zip(names, result.x):
        final.add(name, value=value, min=params[name].min, max=params[name].max)
    return types.SimpleNamespace(success=result.success, message=result.message, params=final, nfev=result.nfev,
                                 cost=result.cost, x=result.x)


refstubs.install()
lmfit = types.ModuleType("lmfit")
lmfit.parameter = types.ModuleType("lmfit.parameter")
lmfit.Parameters = lmfit.parameter.Parameters = Parameters
lmfit.minimize = minimize
sys.modules["lmfit"], sys.modules["lmfit.parameter"] = lmfit, lmfit.parameter
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    import glimpse  # noqa: E402  (not refstubs.import_reference(): it would put the permissive lmfit stub back)
warnings.simplefilter("ignore", (DeprecationWarning, RuntimeWarning))
helpers, optimize = glimpse.helpers, glimpse.optimize

OUT = os.path.join(ROOT, "tests", "golden")
MIN_GAP = 1e-9


def ragged(arrays, width):
    arrays = [np.asarray(a, dtype=float).reshape(-1, width) for a in arrays]
    return (np.concatenate(arrays) if arrays else np.empty((0, width)),
            np.concatenate(([0], np.cumsum([len(a) for a in arrays]))).astype(np.int64))


def nearest_gap(observed, puv):
    d = np.sort(((observed[:, None, :] - puv[None, :, :]) ** 2).sum(axis=2), axis=1)
    return float(((d[:, 1] - d[:, 0]) / d[:, 1]).min()) if puv.shape[0] > 1 else np.inf


def quiet(f, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*args, **kwargs)


# ---- helpers -----------------------------------------------------------------------------------------------------------
def helpers_golden():
    rng = np.random.default_rng(3)
    out = {}
    box = np.array([-0.4, -0.3, 0.45, 0.35])
    out["box"] = box
    lines, clipped = [], []
    for n in (2, 5, 9, 30, 30, 30):
        line = np.cumsum(rng.normal(0, 0.2, (n, 2)), axis=0) + rng.uniform(-0.2, 0.2, 2)
        lines.append(line)
        clipped.append(helpers.clip_polyline_box(line, box))
    out["clip_lines"], out["clip_lines_off"] = ragged(lines, 2)
    out["clip_out"], out["clip_out_off"] = ragged([c for cs in clipped for c in cs], 2)
    out["clip_out_count"] = np.array([len(cs) for cs in clipped])
    assert out["clip_out_count"].max() >= 2 and out["clip_out_count"].min() == 0
    origins, distances = rng.uniform(-1, 1, (40, 2)), rng.normal(0, 1, (40, 2))
    t = [helpers.intersect_edge_box(o, d, box) for o, d in zip(origins, distances)]
    out["edge_origin"], out["edge_distance"] = origins, distances
    out["edge_t"] = np.array([np.nan if v is None else v for v in t])
    assert 5 < np.isnan(out["edge_t"]).sum() < 35
    for nd, bx in ((2, box), (3, np.array([-0.4, -0.3, 0.5, 0.45, 0.35, 2.0]))):
        origin, directions = rng.uniform(-1, 1, nd), rng.normal(0, 1, (50, nd))
        directions[0, 0] = 0.0
        with np.errstate(invalid="ignore"):
            tmin, tmax = helpers.intersect_rays_box(origin, directions, bx, t=True)
            xmin, xmax = helpers.intersect_rays_box(origin, directions, bx)
        out[f"rays{nd}_origin"], out[f"rays{nd}_directions"], out[f"rays{nd}_box"] = origin, directions, bx
        out[f"rays{nd}_tmin"], out[f"rays{nd}_tmax"], out[f"rays{nd}_xmin"], out[f"rays{nd}_xmax"] = tmin, tmax, xmin, xmax
    interp = []
    for k, line in enumerate(lines):
        interp.append(helpers.interpolate_line(line, dx=0.013 * (k + 1)))
    interp.append(helpers.interpolate_line(lines[2], n=7))
    interp.append(helpers.interpolate_line(lines[3], xi=np.array([0.0, 0.1, 0.5])))
    out["interp_out"], out["interp_out_off"] = ragged(interp, 2)
    mask = rng.uniform(size=25) < 0.5
    values = np.arange(25.0)
    for include in ("all", "true", "false"):
        for circular in (False, True):
            parts = helpers.boolean_split(values, mask, circular=circular, include=include)
            out[f"split_{include}_{int(circular)}"], out[f"split_{include}_{int(circular)}_off"] = ragged(parts, 1)
    out["split_mask"] = mask
    # Camera.edges, and the static methods of Cameras
    cam = glimpse.Camera(imgsz=(400, 300), f=(500, 510), c=(2, -3), k=(0.1, -0.05, 0.01, 0.02, 0, 0.001), p=(0.001, -0.002),
                         xyz=(10, 20, 30), viewdir=(5, -2, 1))
    out["cam_vector"] = cam.to_array()
    out["edges_1"] = glimpse.Camera(imgsz=(4, 3), f=1).edges()
    out["edges_half"] = cam.edges(step=cam.imgsz / 2)
    out["edges_7_5"] = cam.edges(step=(7, 5))
    pts = optimize.Points(cam, uv=rng.uniform(0, 300, (6, 2)), xyz=rng.uniform(100, 500, (6, 3)))
    out["points_xyz"] = pts.xyz
    out["scales_none"] = optimize.Cameras.camera_scales(cam)
    out["scales_points"] = optimize.Cameras.camera_scales(cam, [pts])
    out["bounds"] = optimize.Cameras.camera_bounds(cam)
    cases = [{"viewdir": True}, {"viewdir": 0, "f": [0, 1]}, {"viewdir": ([0, 1], -np.inf, 180)},
             {"viewdir": ([0, 1], -np.inf, [180, 170]), "k": ([0, 1], None, np.nan), "xyz": False}, {"c": (True, -1, [2, 3])}]
    for n, case in enumerate(cases):
        for name, default in (("none", None), ("cam", out["bounds"])):
            mask, bounds = optimize.Cameras.parse_params(case, default_bounds=default)
            out[f"parse_{n}_{name}_mask"], out[f"parse_{n}_{name}_bounds"] = mask, bounds
        out[f"labels_{n}"] = np.array(list(optimize.Cameras._lmfit_labels(mask, cam=n, group=None)))
        out[f"labels_group_{n}"] = np.array(list(optimize.Cameras._lmfit_labels(mask, cam=None, group=n)))
    out["ransac_samples_2_4"] = np.array(sorted(sorted(int(v) for v in s) for s in optimize._ransac_samples(n=2, size=4)))
    # ransac with Polynomial: a seeded line with outliers
    x = np.linspace(0, 10, 40)
    xy = np.column_stack((x, 0.7 * x - 1.5 + rng.normal(0, 0.05, 40)))
    xy[::5, 1] += rng.uniform(2, 5, 8)
    out["ransac_xy"] = xy
    np.random.seed(12)
    params, inliers = optimize.ransac(optimize.Polynomial(xy, deg=1), n=2, max_error=0.2, min_inliers=10, iterations=50)
    out["ransac_params"], out["ransac_inliers"] = params, inliers
    out["polyfit_all"] = optimize.Polynomial(xy, deg=2).fit()
    out["poly_errors"] = optimize.Polynomial(xy, deg=1).errors(params)
    np.savez_compressed(os.path.join(OUT, "calib_helpers.npz"), **out)
    return out


# ---- Lines -------------------------------------------------------------------------------------------------------------
LINE_CAMERAS = (dict(imgsz=(400, 300), f=(500, 505), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0, 0)),
                dict(imgsz=(400, 300), f=(500, 505), c=(3, -2), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.003), p=(0.001, -0.002)))


def arc(az0, az1, n, r, z):
    """A world polyline at range r around the origin: azimuths az0 .. az1 (degrees from north), heights z(az)."""
    az = np.linspace(az0, az1, n)
    return np.column_stack((r * np.sin(np.deg2rad(az)), r * np.cos(np.deg2rad(az)), z(az)))


def world_lines():
    inframe = arc(-15, 15, 12, 1000.0, lambda a: 20 + 3 * np.sin(a / 4))
    reenter = arc(-18, 18, 25, 800.0, lambda a: 150 + 150 * np.cos(a / 3.0))  # over the top edge and back
    behind = arc(-170, 170, 60, 1200.0, lambda a: -60 + 0.2 * a)
    short = np.array([[0.0, 900.0, -100.0], [0.02, 900.0, -100.0]])  # 0.01 px: rounds to no point
    outside = arc(40, 80, 9, 1000.0, lambda a: 10 + 0 * a)
    return [inframe, reenter, behind, short], [outside]


def lines_golden():
    out = {}
    main, fallback = world_lines()
    rng = np.random.default_rng(21)
    for c, internals in enumerate(LINE_CAMERAS):
        cam = glimpse.Camera(xyz=(0, 0, 0), viewdir=(2, 3, 1), **internals)
        out[f"cam{c}_vector"] = cam.to_array()
        xy_edges = cam._uv_to_xy(cam.edges(step=cam.imgsz / 2))
        out[f"cam{c}_box"] = np.hstack((np.min(xy_edges, axis=0), np.max(xy_edges, axis=0)))
        for name, xyzs, density in (("main", main, 1), ("dense", main, 2.5), ("fallback", fallback, 1)):
            key = f"cam{c}_{name}"
            probe = optimize.Lines(cam, uvs=[np.zeros((1, 2))], xyzs=xyzs, density=density)
            puvs = probe._xyzs_to_uvs()
            puv = np.vstack(puvs)
            # observed points: near the projected lines (or anywhere, for the fallback), in two image polylines
            pick = rng.choice(len(puv), size=min(70, len(puv)), replace=len(puv) < 70)
            uv = puv[pick] + rng.normal(0, 2.0, (len(pick), 2))
            uvs = [uv[:30], uv[30:]] if len(uv) > 30 else [uv]
            lines = optimize.Lines(cam, uvs=uvs, xyzs=xyzs, density=density)
            gap = nearest_gap(lines.uv, puv)
            assert gap > MIN_GAP, f"{key}: relative gap {gap}: choose another seed"
            out[f"{key}_uv"], out[f"{key}_uv_off"] = ragged(uvs, 2)
            out[f"{key}_xyz"], out[f"{key}_xyz_off"] = ragged(xyzs, 3)
            out[f"{key}_density"] = np.array(float(density))
            out[f"{key}_counts"] = np.array([len(p) for p in puvs])
            out[f"{key}_puv"] = puv
            out[f"{key}_predicted"] = lines.predicted()
            index = np.arange(0, lines.size, 3)
            out[f"{key}_index"], out[f"{key}_predicted_index"] = index, lines.predicted(index=index)
            out[f"{key}_gap"] = np.array(gap)
        assert (out[f"cam{c}_main_counts"] == 0).any() and len(out[f"cam{c}_main_counts"]) >= 5
    np.savez_compressed(os.path.join(OUT, "calib_lines.npz"), **out)
    return out


# ---- Cameras.fit -------------------------------------------------------------------------------------------------------
FIT_INTERNALS = dict(imgsz=(400, 300), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))


def fit_golden():
    rng = np.random.default_rng(5)
    n = 3
    true_viewdirs = np.array([[-20.0, 2.0, 1.0], [0.0, 3.0, -1.0], [20.0, 1.0, 0.5]])
    start_viewdirs = true_viewdirs + rng.normal(0, 0.7, (n, 3))
    true_f, start_f = 500.0, 520.0
    horizon = arc(-60, 60, 80, 2000.0, lambda a: 150 + 60 * np.sin(a / 9.0) + 20 * np.cos(a / 2.0))
    true = [glimpse.Camera(f=true_f, viewdir=v, **FIT_INTERNALS) for v in true_viewdirs]
    cams = [glimpse.Camera(f=start_f, viewdir=v, **FIT_INTERNALS) for v in start_viewdirs]
    out = {"true_viewdirs": true_viewdirs, "start_viewdirs": start_viewdirs, "true_f": np.array(true_f),
           "start_f": np.array(start_f), "horizon": horizon,
           "internals": np.concatenate([np.asarray(FIT_INTERNALS[key], dtype=float) for key in ("imgsz", "c", "k", "p")])}
    controls, matches = [], []
    for i in range(n):
        uv = rng.uniform((30, 30), (370, 270), (15, 2))
        xyz = true[i].uv_to_xyz(uv, directions=False, depth=rng.uniform(500, 3000, 15))
        points = optimize.Points(cams[i], uv=uv + rng.normal(0, 0.3, uv.shape), xyz=xyz)
        puv = np.vstack(optimize.Lines(true[i], uvs=[np.zeros((1, 2))], xyzs=[horizon])._xyzs_to_uvs())
        traced = puv[:: max(1, len(puv) // 100)] + rng.normal(0, 0.3, (len(puv[:: max(1, len(puv) // 100)]), 2))
        lines = optimize.Lines(cams[i], uvs=[traced], xyzs=[horizon])
        controls += [points, lines]
        out[f"points{i}_uv"], out[f"points{i}_xyz"], out[f"lines{i}_uv"] = points.uv, points.xyz, lines.uv
    for i in range(n - 1):
        uv_i = rng.uniform((250, 30), (370, 270), (65, 2))
        uv_j = true[i + 1].xyz_to_uv(true[i].uv_to_xyz(uv_i), directions=True)
        m = optimize.Matches(cams=[cams[i], cams[i + 1]], uvs=[uv_i + rng.normal(0, 0.3, uv_i.shape),
                                                               uv_j + rng.normal(0, 0.3, uv_j.shape)])
        matches.append(m)
        out[f"matches{i}_uv0"], out[f"matches{i}_uv1"] = m.uvs
        for side in (0, 1):
            out[f"matches{i}_predicted{side}"] = m.predicted(cam=side)
        for name, mtype in (("rotation", optimize.RotationMatches), ("xy", optimize.RotationMatchesXY)):
            r = m.to_type(mtype)
            out[f"matches{i}_xy0"], out[f"matches{i}_xy1"] = r.xys
            out[f"matches{i}_{name}_predicted0"] = r.predicted(cam=0)
    model = optimize.Cameras(cams, controls, cam_params=[{"viewdir": True}] * n, group_params={"f": True})
    out["labels"] = np.array(list(model.params))
    out["scales"], out["sparsity"] = model.scales, model.sparsity.toarray()
    out["x0"] = np.array(list(model.params.valuesdict().values()))
    out["lower"] = np.array([p.min for p in model.params.values()])
    out["upper"] = np.array([p.max for p in model.params.values()])
    out["predicted_start"] = model.predicted()
    out["residuals_start"] = model.residuals()
    smallest = np.inf
    for control in controls:
        if isinstance(control, optimize.Lines):
            smallest = min(smallest, nearest_gap(control.uv, np.vstack(control._xyzs_to_uvs())))
    assert smallest > MIN_GAP, f"relative gap {smallest}: choose another seed"
    out["gap_start"] = np.array(smallest)
    result = quiet(model.fit, full=True)
    assert result.success
    out["fit_x"], out["fit_nfev"] = np.asarray(result.x), np.array(int(result.nfev))
    out["rmse_start"] = np.array(float(np.sqrt((model.errors() ** 2).mean())))
    out["rmse_fit"] = np.array(float(np.sqrt((model.errors(params=result.x) ** 2).mean())))
    assert np.array_equal(np.array([c.viewdir for c in cams]), start_viewdirs)
    # the model with matches, for `predicted` through the handle
    both = optimize.Cameras(cams, controls + matches, cam_params=[{"viewdir": True}] * n, group_params={"f": True})
    out["predicted_start_matches"] = both.predicted()
    np.savez_compressed(os.path.join(OUT, "calib_fit.npz"), **out)
    return out


if __name__ == "__main__":
    h = helpers_golden()
    print("helpers", len(h), "arrays; ransac", h["ransac_params"], len(h["ransac_inliers"]), "inliers")
    g = lines_golden()
    print("lines", {k: v.tolist() for k, v in g.items() if k.endswith(("_counts", "_gap"))})
    f = fit_golden()
    print("fit", f["fit_x"], "nfev", int(f["fit_nfev"]), "rmse", float(f["rmse_start"]), "->", float(f["rmse_fit"]),
          "gap", float(f["gap_start"]))
    for name in ("calib_helpers.npz", "calib_lines.npz", "calib_fit.npz"):
        print(name, os.path.getsize(os.path.join(OUT, name)), "bytes")
