"""Designed cases for `optimize.ransac(batched=True)` (tests/test_ransac_cases.py admits them on the CPU,
tests/test_gpu_ransac.py runs them): a camera with k1 and p1 set, world points and rays placed by oracle/camera.py,
inliers with Gaussian noise of SIGMA px, outliers displaced by OUT_MIN .. OUT_MAX px, max_error = MAX_ERROR.  Nothing here
needs a GPU.

The shapes are the smallest at which the kernels can go wrong: row counts either side of a wave (63, 64, 65), of the fit
kernel's workgroup (127, 128, 129: CAL_FIT_TB rows at a time) and of the scoring kernel's (255, 256, 257); samples from the
smallest that determines the parameters (one row for one angle, two for three) to 70 (more than a wave of rows in a
sample); 1, 3 and 18 parameters (the largest mask: xyz, viewdir, f, c, k, p); 1 and 100 hypotheses drawn (one_hypothesis_127,
hundred_63: `_ransac_samples` draws no more samples than there are combinations, so 100 need n >= 2 on 63 rows).

Seeds: a case's seed is replaced here, and said so, if the case fails admission.  Replaced so far: weights_65 3 -> 303
(errors within 1e-2 px of max_error, or no clean sample, under the seeds tried between), one_hypothesis_127 4 -> 64 (its one sample
has to be clean), all_parameters_257 10 -> 12 (an error within 1e-2 px of max_error).  rotation_129 6 -> 15, matches_b_256
8 -> 13, two_kinds_257 9 -> 28 (an error within 1e-2 px of max_error each).  Under a contaminated sample the errors of the
other rows spread over tens of pixels and some row lands within 1e-2 px of max_error sooner or later, so the cases with many
rows keep their hypotheses few and their outliers rare: a clean sample of 12 among 30 % outliers would take about 70 draws.
"""
import numpy as np

from oracle import camera as oc

SIGMA, OUT_MIN, OUT_MAX, MAX_ERROR = 0.3, 20.0, 60.0, 3.0
IMGSZ, F, C, K1, P1 = (400.0, 268.0), (420.0, 415.0), (3.0, -2.0), 0.03, 0.002
TRUE_VIEWDIR, START_OFFSET = np.array([12.0, -6.0, 3.0]), np.array([1.2, -0.8, 0.6])
OTHER_VIEWDIR = np.array([15.5, -4.0, 1.0])  # the second camera of the match controls
ALL = {"xyz": True, "viewdir": True, "f": True, "c": True, "k": True, "p": True}

# name -> controls [(kind, rows)], n, cam_params, iterations, min_inliers, outlier share, seed and the extras
CASES = {
    # (one angle is fitted: the start differs from the truth in that angle alone)
    "one_angle_63": dict(controls=[("points", 63)], n=1, params={"viewdir": 0}, iterations=100, min_inliers=20, outliers=0.3, seed=1,
                         offset=(1.2, 0.0, 0.0)),
    # (100 samples are drawn: 63 rows have 1953 pairs.  one_angle_63 asks for 100 too and gets the 63 there are.)
    "hundred_63": dict(controls=[("points", 63)], n=2, params={"viewdir": True}, iterations=100, min_inliers=20, outliers=0.1, seed=20),
    "viewdir_64": dict(controls=[("points", 64)], n=2, params={"viewdir": True}, iterations=12, min_inliers=20, outliers=0.3, seed=2),
    "weights_65": dict(controls=[("points", 65)], n=12, params={"viewdir": True}, iterations=12, min_inliers=20, outliers=0.3, seed=303,
                       weights=True),
    "one_hypothesis_127": dict(controls=[("points", 127)], n=4, params={"viewdir": True}, iterations=1, min_inliers=40, outliers=0.3,
                               seed=64),
    "behind_128": dict(controls=[("points", 128)], n=6, params={"viewdir": True}, iterations=12, min_inliers=40, outliers=0.25,
                       seed=5, behind=10),
    "rotation_129": dict(controls=[("rotation", 129)], n=12, params={"viewdir": True}, iterations=10, min_inliers=40, outliers=0.1,
                         seed=15),
    "matches_a_255": dict(controls=[("matches", 255)], n=12, params={"viewdir": True}, iterations=6, min_inliers=80, outliers=0.04,
                          seed=7),
    "matches_b_256": dict(controls=[("matches", 256)], n=12, params={"viewdir": True}, iterations=6, min_inliers=80, outliers=0.04,
                          seed=13, side=1),
    "two_kinds_257": dict(controls=[("points", 129), ("matches", 128)], n=12, params={"viewdir": True}, iterations=10, min_inliers=80,
                          outliers=0.1, seed=28),
    "all_parameters_257": dict(controls=[("points", 257)], n=40, params=ALL, iterations=3, min_inliers=80, outliers=0.02, seed=12),
    "clean_257": dict(controls=[("points", 257)], n=70, params={"viewdir": True}, iterations=10, min_inliers=100, outliers=0.0, seed=11),
}
POINTS_CASES = [name for name, case in CASES.items() if all(kind == "points" for kind, _ in case["controls"])]


def vector(viewdir):
    return oc.make_camera(imgsz=IMGSZ, f=F, c=C, k=(K1,), p=(P1,), viewdir=viewdir)


def _observe(rng, uv, outliers, behind=0):
    """`uv` with the inliers' noise; the last rows displaced as outliers.  Returns (observed, is_inlier)."""
    n = len(uv)
    n_out = int(round(outliers * (n - behind)))
    inlier = np.ones(n, dtype=bool)
    inlier[n - n_out:] = False
    angle, length = rng.uniform(0, 2 * np.pi, n), rng.uniform(OUT_MIN, OUT_MAX, n)
    shift = np.where(inlier[:, None], rng.normal(0, SIGMA, (n, 2)), np.column_stack((np.cos(angle), np.sin(angle))) * length[:, None])
    return uv + shift, inlier


def data(name):
    """The arrays of case `name`: per control a dict (kind; points: uv, xyz; matches: uv0, uv1; rotation: uv0, uv1, xy0,
    xy1), rows shuffled so that inliers, outliers and the rows behind the camera mix; `inlier` (which rows were placed as
    inliers), the camera vectors `true`, `start` and `other`, and `side`."""
    case = CASES[name]
    rng = np.random.default_rng(1000 + case["seed"])
    true, start, other = vector(TRUE_VIEWDIR), vector(TRUE_VIEWDIR + case.get("offset", START_OFFSET)), vector(OTHER_VIEWDIR)
    side = case.get("side", 0)
    controls, inliers = [], []
    for kind, rows in case["controls"]:
        uv = np.column_stack((rng.uniform(10, IMGSZ[0] - 10, rows), rng.uniform(10, IMGSZ[1] - 10, rows)))
        behind = case.get("behind", 0) if kind == "points" else 0
        order = rng.permutation(rows)
        if kind == "points":
            depth = rng.uniform(40, 400, rows)
            depth[:behind] *= -1  # (behind the true camera, and behind every camera within a few degrees of it)
            xyz = oc.uv_to_xyz(true, uv, directions=False, depth=depth)
            with np.errstate(invalid="ignore"):
                exact = oc.xyz_to_uv(true, xyz)
            exact[:behind] = uv[:behind]
            observed, inlier = _observe(rng, exact, case["outliers"], behind)
            inlier[:behind] = False
            controls.append(dict(kind=kind, uv=observed[order], xyz=xyz[order]))
        else:
            # `uv` lies in the camera whose points are unprojected: the second of the control.  The fitted camera is the
            # control's first (side 0) or its second (side 1); the other one is `other`.
            first, second = (true, other) if side == 0 else (other, true)
            exact = oc.xyz_to_uv(first, oc.uv_to_xyz(second, uv))
            observed, inlier = _observe(rng, exact, case["outliers"])
            control = dict(kind=kind, uv0=observed[order], uv1=uv[order])
            if kind == "rotation":  # the camera coordinates the control would compute from the image coordinates
                for i in (0, 1):
                    v = (true, other)[i]
                    control[f"xy{i}"] = oc.undistort(v, (control[f"uv{i}"] - (v[6:8] / 2 + v[10:12])) * (1 / v[8:10]))
            controls.append(control)
        inliers.append(inlier[order])
    return dict(controls=controls, inlier=np.concatenate(inliers), true=true, start=start, other=other, side=side)


def weights(name):
    """One weight per row, between 0.5 and 2 (Cameras normalises them to a mean of 1)."""
    size = sum(rows for _, rows in CASES[name]["controls"])
    return np.random.default_rng(2000 + CASES[name]["seed"]).uniform(0.5, 2.0, size) if CASES[name].get("weights") else None


def camera_of(v):
    import glimpse_amd

    return glimpse_amd.Camera(xyz=v[0:3], viewdir=v[3:6], imgsz=v[6:8], f=v[8:10], c=v[10:12], k=v[12:18], p=v[18:20])


def model(name):
    """(Cameras model at the start values, its arrays): the fitted camera is `model.cams[0]`."""
    from glimpse_amd import optimize

    case, d = CASES[name], data(name)
    fitted, other = camera_of(d["start"]), camera_of(d["other"])
    controls = []
    for c in d["controls"]:
        if c["kind"] == "points":
            controls.append(optimize.Points(fitted, uv=c["uv"], xyz=c["xyz"]))
            continue
        cams = [fitted, other] if d["side"] == 0 else [other, fitted]
        if c["kind"] == "matches":
            controls.append(optimize.Matches(cams=cams, uvs=[c["uv0"], c["uv1"]]))
        else:
            controls.append(optimize.RotationMatches(cams=cams, uvs=[c["uv0"], c["uv1"]], xys=[c["xy0"], c["xy1"]]))
    # (rows behind the camera are dropped from a fit's residuals, which scipy's sparsity structure does not allow for)
    m = optimize.Cameras([fitted], controls, cam_params=[case["params"]], weights=weights(name), sparsity=not case.get("behind"))
    return m, d


def call(name):
    """ransac's arguments for case `name`."""
    case = CASES[name]
    return dict(n=case["n"], max_error=MAX_ERROR, min_inliers=case["min_inliers"], iterations=case["iterations"])
