"""Admission of the designed RANSAC cases (tests/ransac_cases.py) on the CPU: every case is run through RANSAC in
NumPy -- the residuals by oracle/camera.py, the fits by scipy.optimize.least_squares with the model's bounds and scales --
and must keep every decision the GPU test compares well away from its threshold.  These are conditions on the inputs, not
measurements of the package: nothing here projects through its kernels."""
import functools

import numpy as np
import pytest

from oracle import camera as oc
from tests import ransac_cases as rc

ERROR_GAP = 1e-2  # px: no row's error this close to max_error
COUNT_GAP = 2     # no consensus count this close to min_inliers
MEAN_GAP = 0.01   # the best and the second-best distinct set differ by more than this, relative


def predicted(d, v, c):
    """`predicted` of the control arrays `c` of the case arrays `d` with the fitted camera at the vector `v`, by the
    formulas of oracle/camera.py (every camera stands at the origin, so a ray is a point)."""
    if c["kind"] == "points":
        return oc.xyz_to_uv(v, c["xyz"])
    first, second = (v, d["other"]) if d["side"] == 0 else (d["other"], v)
    if c["kind"] == "matches":
        rays = oc.uv_to_xyz(second, c["uv1"])
    else:  # Camera._xy_to_xyz: R.T[:, 0:2] @ xy + R.T[:, 2]
        R = oc.rotation_matrix(second[3:6])
        rays = c["xy1"] @ R[0:2] + R[2]
    return oc.xyz_to_uv(first, rays)


@functools.lru_cache(maxsize=None)
def numpy_ransac(name):
    """RANSAC over the case `name` as optimize.ransac runs it, in NumPy.  Returns a dict: per hypothesis the fitted
    values (None where the fit failed), the errors of all rows and the consensus count; the distinct sets with their
    refitted values and mean errors; the winner and the final errors."""
    import scipy.optimize
    from glimpse_amd.optimize import _ransac_samples

    model, d = rc.model(name)
    call = rc.call(name)
    slots = np.flatnonzero(model.cam_masks[0])
    x0, lb, ub = model._values_bounds()
    uv = np.vstack([c["uv" if c["kind"] == "points" else "uv0"] for c in d["controls"]])
    w = np.ones((len(uv), 1)) if model.weights is None else model.weights

    def residuals(x, rows=slice(None)):
        v = d["start"].copy()
        v[slots] = x
        with np.errstate(invalid="ignore"):
            return (np.vstack([predicted(d, v, c) for c in d["controls"]])[rows] - uv[rows]) * w[rows]

    def errors(x, rows=slice(None)):
        return np.linalg.norm(residuals(x, rows), axis=1)

    def fit(rows):
        def fun(x):
            r = residuals(x, rows).ravel()
            return r[~np.isnan(r)]

        if len(fun(x0)) < len(x0):
            return None
        result = scipy.optimize.least_squares(fun, x0, bounds=(lb, ub), x_scale=model.scales)
        return result.x if result.success else None

    np.random.seed(rc.CASES[name]["seed"])
    samples = list(_ransac_samples(n=call["n"], size=len(uv), iterations=call["iterations"]))
    full = np.arange(len(uv))
    hypotheses, sets = [], {}
    for h, sample in enumerate(samples):
        x = fit(sample)
        if x is None:
            hypotheses.append(dict(values=None, errors=None, count=0))
            continue
        e = errors(x)
        test = np.delete(full, sample)
        with np.errstate(invalid="ignore"):
            also = test[e[test] < call["max_error"]]
        hypotheses.append(dict(values=x, errors=e, count=len(also)))
        if len(also) > call["min_inliers"]:
            members = np.sort(np.concatenate((sample, also)))
            sets.setdefault(members.tobytes(), dict(rows=members, hypothesis=h))
    sets = list(sets.values())
    for s in sets:
        s["values"] = fit(s["rows"])
        s["mean"] = np.nan if s["values"] is None else float(np.mean(errors(s["values"], s["rows"])))
    usable = [k for k in np.argsort([s["mean"] for s in sets], kind="stable") if not np.isnan(sets[k]["mean"])]
    final = errors(sets[usable[0]]["values"]) if usable else None
    return dict(samples=samples, hypotheses=hypotheses, sets=sets, order=usable, final=final, call=call, data=d)


def test_the_cases_cover_the_shapes():
    sizes = sorted(sum(rows for _, rows in case["controls"]) for case in rc.CASES.values())
    assert set(sizes) >= {63, 64, 65, 127, 128, 129, 255, 256, 257}
    drawn = {name: len(numpy_ransac(name)["samples"]) for name in rc.CASES}
    assert drawn["one_hypothesis_127"] == 1 and drawn["hundred_63"] == 100 and drawn["one_angle_63"] == 63
    assert {1, 2, 70} <= {case["n"] for case in rc.CASES.values()}
    masks = {name: int(rc.model(name)[0].cam_masks[0].sum()) for name in ("one_angle_63", "viewdir_64", "all_parameters_257")}
    assert masks == {"one_angle_63": 1, "viewdir_64": 3, "all_parameters_257": 18}
    assert rc.model("weights_65")[0].weights is not None and len(rc.model("two_kinds_257")[0].controls) == 2
    m, a = rc.model("matches_b_256")[0], rc.model("matches_a_255")[0]
    assert m.controls[0].cams[1] is m.cams[0] and a.controls[0].cams[0] is a.cams[0]
    for name in rc.CASES:
        d = rc.data(name)
        assert rc.CASES[name]["outliers"] == 0 or (~d["inlier"]).sum() >= 5, name


def test_rows_behind_the_camera_have_no_prediction():
    d = rc.data("behind_128")
    c = d["controls"][0]
    for v in (d["true"], d["start"]):
        with np.errstate(invalid="ignore"):
            nan = np.isnan(oc.xyz_to_uv(v, c["xyz"])).any(axis=1)
        assert nan.sum() == rc.CASES["behind_128"]["behind"]


def test_outliers_are_displaced_and_inliers_are_not():
    for name in rc.POINTS_CASES:
        d = rc.data(name)
        uv, xyz = (np.vstack([c[k] for c in d["controls"]]) for k in ("uv", "xyz"))
        with np.errstate(invalid="ignore"):
            off = np.linalg.norm(oc.xyz_to_uv(d["true"], xyz) - uv, axis=1)
        seen = ~np.isnan(off)
        assert (off[seen & ~d["inlier"]] >= rc.OUT_MIN - 1e-9).all() and (off[d["inlier"]] < 6 * rc.SIGMA).all(), name


@pytest.mark.parametrize("name", list(rc.CASES))
def test_admission(name):
    """No row's error within ERROR_GAP of max_error under any hypothesis's fit or the final fit; no consensus count within
    COUNT_GAP of min_inliers; the two best distinct sets more than MEAN_GAP apart in mean error; and a winner exists."""
    got = numpy_ransac(name)
    call = got["call"]
    gaps = [np.nanmin(np.abs(h["errors"] - call["max_error"])) for h in got["hypotheses"] if h["errors"] is not None]
    counts = np.array([h["count"] for h in got["hypotheses"] if h["values"] is not None])
    means = [got["sets"][k]["mean"] for k in got["order"]]
    print(name, ": smallest |error - max_error|", min(gaps), "final", np.nanmin(np.abs(got["final"] - call["max_error"])),
          "; consensus counts", sorted(set(counts.tolist())), "against", call["min_inliers"], "; distinct sets", len(got["sets"]),
          "mean errors", means[:3])
    assert got["order"], "no set qualifies"
    assert min(gaps) > ERROR_GAP and np.nanmin(np.abs(got["final"] - call["max_error"])) > ERROR_GAP
    assert (np.abs(counts - call["min_inliers"]) > COUNT_GAP).all()
    assert len(means) < 2 or means[1] - means[0] > MEAN_GAP * means[0]
