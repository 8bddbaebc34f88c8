"""The host half of the camera calibration (glimpse_amd.optimize: Points, Lines, Cameras, ransac, Polynomial; the polyline
helpers; Camera.edges) against the reference's docstring examples and its recorded outputs (tests/golden/calib_*.npz, made
by tools/make_golden_calib.py), and the NumPy restatement of Lines.predicted (tests/calib_restated.py) against the
reference's.  No GPU: nothing here projects through the package's kernels."""
import numpy as np
import pytest

from tests import calib_restated as rs

TOL = dict(rtol=1e-11, atol=1e-9)  # image coordinates (tests/test_gpu_parity.py)
MIN_GAP = 1e-9
LINE_CASES = [(c, name) for c in (0, 1) for name in ("main", "dense", "fallback")]


def split(flat, off):
    return [flat[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_helper_docstring_examples():
    from glimpse_amd import helpers

    a, mask = np.array([0, 1, 2, 3, 4]), np.array([True, True, False, False, True])
    assert [p.tolist() for p in helpers.boolean_split(a, mask)] == [[0, 1], [2, 3], [4]]
    assert [p.tolist() for p in helpers.boolean_split(a, mask, circular=True)] == [[4, 0, 1], [2, 3]]
    assert [p.tolist() for p in helpers.boolean_split(a, mask, circular=True, include="true")] == [[4, 0, 1]]
    assert helpers.in_box(np.array([(0, 0), (1, 1), (2, 2), (3, 3)]), box=[1, 1, 2.5, 2.5]).tolist() == [False, True, True, False]
    (clipped,) = helpers.clip_polyline_box(np.array([(0, 0), (1, 1), (3, 3)]), (0.5, 0.5, 1.5, 1.5))
    assert clipped.tolist() == [[0.5, 0.5], [1.0, 1.0], [1.5, 1.5]]
    assert helpers.clip_polyline_box(np.array([(0, 0), (10, 10)]), (4, 4, 6, 6)) == []
    box = 1, -1, 2, 2
    assert helpers.intersect_edge_box((0, 0), (1, 1), box) is None and helpers.intersect_edge_box((0, 0), (2, 2), box) == 0.5
    directions = np.array([(1, 0), (1, 1)])
    tmin, tmax = helpers.intersect_rays_box((0, 0), directions, box, t=True)
    assert tmin.tolist() == [[1.0], [1.0]] and tmax.tolist() == [[2.0], [2.0]]
    xmin, xmax = helpers.intersect_rays_box((0, 0), directions, box)
    assert xmin.tolist() == [[1, 0], [1, 1]] and xmax.tolist() == [[2, 0], [2, 2]]
    line = np.array([(0, 0), (1, 0), (1, 1)])
    assert helpers.interpolate_line(line, xi=(1.5, 2)).tolist() == [[1, 0.5], [1, 1]]
    assert helpers.interpolate_line(line, n=2).tolist() == [[0, 0], [1, 1]]
    assert helpers.interpolate_line(line, dx=1).tolist() == [[0, 0], [1, 0], [1, 1]]
    assert helpers.interpolate_line(line, xi=(-1, 3), error=False).tolist() == [[0, 0], [1, 1]]
    with pytest.raises(ValueError, match="outside range"):
        helpers.interpolate_line(line, xi=(-1, 3))


def test_helpers_against_the_reference(golden):
    """Exact: the helpers are the reference's NumPy expressions."""
    from glimpse_amd import helpers

    g = golden("calib_helpers.npz")
    lines = split(g["clip_lines"], g["clip_lines_off"])
    want = split(g["clip_out"], g["clip_out_off"])
    got = [c for line in lines for c in helpers.clip_polyline_box(line, g["box"])]
    assert [len(helpers.clip_polyline_box(line, g["box"])) for line in lines] == g["clip_out_count"].tolist()
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    t = [helpers.intersect_edge_box(o, d, g["box"]) for o, d in zip(g["edge_origin"], g["edge_distance"])]
    assert np.array_equal(np.array([np.nan if v is None else v for v in t]), g["edge_t"], equal_nan=True)
    for nd in (2, 3):
        tmin, tmax = helpers.intersect_rays_box(g[f"rays{nd}_origin"], g[f"rays{nd}_directions"], g[f"rays{nd}_box"], t=True)
        xmin, xmax = helpers.intersect_rays_box(g[f"rays{nd}_origin"], g[f"rays{nd}_directions"], g[f"rays{nd}_box"])
        for a, name in ((tmin, "tmin"), (tmax, "tmax"), (xmin, "xmin"), (xmax, "xmax")):
            assert np.array_equal(a, g[f"rays{nd}_{name}"], equal_nan=True), (nd, name)
    interp = [helpers.interpolate_line(line, dx=0.013 * (k + 1)) for k, line in enumerate(lines)]
    interp.append(helpers.interpolate_line(lines[2], n=7))
    interp.append(helpers.interpolate_line(lines[3], xi=np.array([0.0, 0.1, 0.5])))
    want = split(g["interp_out"], g["interp_out_off"])
    assert len(interp) == len(want) and all(np.array_equal(a, b) for a, b in zip(interp, want))
    values = np.arange(25.0)
    for include in ("all", "true", "false"):
        for circular in (False, True):
            parts = helpers.boolean_split(values, g["split_mask"], circular=circular, include=include)
            want = split(g[f"split_{include}_{int(circular)}"][:, 0], g[f"split_{include}_{int(circular)}_off"])
            assert len(parts) == len(want) and all(np.array_equal(a, b) for a, b in zip(parts, want)), (include, circular)


def camera_of(vector):
    import glimpse_amd

    return glimpse_amd.Camera(xyz=vector[0:3], viewdir=vector[3:6], imgsz=vector[6:8], f=vector[8:10], c=vector[10:12],
                              k=vector[12:18], p=vector[18:20])


PARSE_CASES = [{"viewdir": True}, {"viewdir": 0, "f": [0, 1]}, {"viewdir": ([0, 1], -np.inf, 180)},
               {"viewdir": ([0, 1], -np.inf, [180, 170]), "k": ([0, 1], None, np.nan), "xyz": False}, {"c": (True, -1, [2, 3])}]


def test_camera_edges_scales_bounds_and_params(golden):
    import glimpse_amd
    from glimpse_amd.optimize import Cameras, Points

    g = golden("calib_helpers.npz")
    cam = camera_of(g["cam_vector"])
    assert glimpse_amd.Camera(imgsz=2, f=1).edges().tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [1, 2], [0, 2], [0, 1]]
    assert np.array_equal(glimpse_amd.Camera(imgsz=(4, 3), f=1).edges(), g["edges_1"])
    assert np.array_equal(cam.edges(step=cam.imgsz / 2), g["edges_half"])
    assert np.array_equal(cam.edges(step=(7, 5)), g["edges_7_5"])
    points = Points(cam, uv=np.zeros((6, 2)), xyz=g["points_xyz"])
    assert np.array_equal(Cameras.camera_scales(cam), g["scales_none"])
    assert np.array_equal(Cameras.camera_scales(cam, [points]), g["scales_points"])
    assert np.array_equal(Cameras.camera_bounds(cam), g["bounds"])
    for n, case in enumerate(PARSE_CASES):
        for name, default in (("none", None), ("cam", g["bounds"])):
            mask, bounds = Cameras.parse_params(case, default_bounds=default)
            assert np.array_equal(mask, g[f"parse_{n}_{name}_mask"]) and np.array_equal(bounds, g[f"parse_{n}_{name}_bounds"])
        assert list(Cameras._lmfit_labels(mask, cam=n)) == g[f"labels_{n}"].tolist()
        assert list(Cameras._lmfit_labels(mask, group=n)) == g[f"labels_group_{n}"].tolist()


def test_prune_sparsity_and_the_three_errors(golden):
    import glimpse_amd
    from glimpse_amd.optimize import Cameras, Lines, Matches, Points

    cams = [glimpse_amd.Camera(imgsz=100, f=10), glimpse_amd.Camera(imgsz=100, f=10)]
    controls = [Points(cam=cams[0], uv=[(0, 0)], xyz=[(0, 0, 0)]), Lines(cam=cams[1], uvs=[[(0, 0)]], xyzs=[[(0, 0, 0)]]),
                Matches(cams=cams, uvs=[[(0, 0)], [(0, 0)]])]
    assert Cameras.prune_controls(controls, cams) == controls
    assert Cameras.prune_controls(controls, cams[0:1]) == [controls[0], controls[2]]
    assert Cameras.prune_controls(controls, cams[1:2]) == [controls[1], controls[2]]
    with pytest.raises(ValueError, match="No controls reference the cameras"):
        Cameras([glimpse_amd.Camera(imgsz=100, f=10)], controls)
    other = glimpse_amd.Camera(imgsz=(100, 80), f=10)
    with pytest.raises(ValueError, match="Group 0: 'f' or 'c' in parameters but image sizes not equal"):
        Cameras([cams[0], other], [controls[0], Points(cam=other, uv=[(0, 0)], xyz=[(0, 0, 0)])], group_params={"f": True})
    with pytest.raises(ValueError, match="Some cameras are in multiple groups with overlapping masks"):
        Cameras(cams, controls, group_indices=[[0, 1], [1]], group_params=[{"f": True}, {"f": True}])
    with pytest.raises(ValueError, match="Not all cameras with params appear in controls"):
        Cameras(cams, controls[0:1], cam_params=[{}, {"viewdir": True}])
    # the sparsity, the scales and the parameters of the reference's model
    g = golden("calib_fit.npz")
    model = fit_model(g)
    assert list(model.params) == g["labels"].tolist()
    table = np.array(list(model.params.values()))
    assert np.array_equal(table[:, 0], g["x0"]) and np.array_equal(table[:, 1], g["lower"]) and np.array_equal(table[:, 2], g["upper"])
    assert np.array_equal(model.sparsity.toarray(), g["sparsity"])
    assert np.array_equal(model.scales, g["scales"])
    model.set_cameras(g["fit_x"])
    assert np.array_equal(model.cams[1].viewdir, g["fit_x"][5:8]) and np.array_equal(model.cams[2].f, g["fit_x"][0:2])
    model.reset_cameras()
    assert np.array_equal(model.cams[1].viewdir, g["start_viewdirs"][1])


def fit_internals(g):
    v = g["internals"]
    return dict(imgsz=v[0:2], c=v[2:4], k=v[4:10], p=v[10:12])


def fit_model(g, matches=False):
    import glimpse_amd
    from glimpse_amd.optimize import Cameras, Lines, Matches, Points

    cams = [glimpse_amd.Camera(f=float(g["start_f"]), viewdir=v, **fit_internals(g)) for v in g["start_viewdirs"]]
    controls = []
    for i, cam in enumerate(cams):
        controls += [Points(cam, uv=g[f"points{i}_uv"], xyz=g[f"points{i}_xyz"]), Lines(cam, uvs=[g[f"lines{i}_uv"]], xyzs=[g["horizon"]])]
    if matches:
        controls += [Matches(cams=[cams[i], cams[i + 1]], uvs=[g[f"matches{i}_uv0"], g[f"matches{i}_uv1"]]) for i in range(len(cams) - 1)]
    return Cameras(cams, controls, cam_params=[{"viewdir": True}] * len(cams), group_params={"f": True})


def test_ransac_and_polynomial(golden):
    from glimpse_amd.optimize import Polynomial, _ransac_samples, ransac

    g = golden("calib_helpers.npz")
    assert sorted(sorted(int(v) for v in s) for s in _ransac_samples(n=2, size=4)) == g["ransac_samples_2_4"].tolist()
    assert g["ransac_samples_2_4"].tolist() == [[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]
    with pytest.raises(ValueError, match="Sample size is larger or equal to total size"):
        next(_ransac_samples(n=4, size=4))
    np.random.seed(12)
    params, inliers = ransac(Polynomial(g["ransac_xy"], deg=1), n=2, max_error=0.2, min_inliers=10, iterations=50)
    assert np.array_equal(params, g["ransac_params"]) and np.array_equal(inliers, g["ransac_inliers"])
    assert np.array_equal(Polynomial(g["ransac_xy"], deg=2).fit(), g["polyfit_all"])
    assert np.array_equal(Polynomial(g["ransac_xy"], deg=1).errors(params), g["poly_errors"])
    assert Polynomial(g["ransac_xy"]).size == 40
    with pytest.raises(ValueError, match="Best fit does not meet acceptance criteria"):
        ransac(Polynomial(g["ransac_xy"], deg=1), n=2, max_error=1e-9, min_inliers=30, iterations=5)
    with pytest.raises(NotImplementedError):
        Polynomial(g["ransac_xy"]).plot()


@pytest.mark.parametrize("c,name", LINE_CASES)
def test_lines_restatement_against_the_reference(golden, c, name):
    """Fed the reference's own clip box (its inverse distortion is another code path than the restatement pins): the
    points per segment exactly, the projected points and `predicted` within the image-coordinate tolerance."""
    from oracle import camera as oc

    g = golden("calib_lines.npz")
    key = f"cam{c}_{name}"
    cam = g[f"cam{c}_vector"]
    R = oc.rotation_matrix(cam[3:6])
    xyzs = split(g[f"{key}_xyz"], g[f"{key}_xyz_off"])
    density = float(g[f"{key}_density"])
    puvs = rs.projected(cam, R, xyzs, g[f"cam{c}_box"], density=density)
    assert [len(p) for p in puvs] == g[f"{key}_counts"].tolist()
    np.testing.assert_allclose(np.vstack(puvs), g[f"{key}_puv"], **TOL)
    info = {}
    got = rs.lines_predicted(cam, R, g[f"{key}_uv"], xyzs, g[f"cam{c}_box"], density=density, info=info)
    assert info["gap"] > MIN_GAP and float(g[f"{key}_gap"]) > MIN_GAP
    np.testing.assert_allclose(got, g[f"{key}_predicted"], **TOL)
    index = g[f"{key}_index"]
    np.testing.assert_allclose(rs.lines_predicted(cam, R, g[f"{key}_uv"][index], xyzs, g[f"cam{c}_box"], density=density),
                               g[f"{key}_predicted_index"], **TOL)


def test_linspace_and_interp_rules_are_numpys():
    rng = np.random.default_rng(0)
    for _ in range(200):
        m = int(rng.integers(2, 12))
        x = np.concatenate(([0.0], np.cumsum(rng.uniform(1e-3, 1.0, m - 1))))
        f = rng.normal(size=m)
        n = int(rng.integers(1, 40))
        t = rs.linspace(x[0], x[-1], n)
        assert np.array_equal(t, np.linspace(x[0], x[-1], n))
        assert np.array_equal(rs.interp(t, x, f), np.interp(t, x, f))
    assert np.array_equal(rs.linspace(0.0, 0.0, 1), np.linspace(0.0, 0.0, 1)) and len(rs.linspace(0.0, 1.0, 0)) == 0


def test_restated_fit_against_the_reference(golden):
    """scipy.optimize.least_squares with SciPy's own 2-point differences, the reference's scales, sparsity and bounds, on
    the restated residuals: per parameter within 1e-3 of its `scales` entry (a thousandth of a pixel's worth) of the
    reference's fit.  Measured on the CPU (printed below): the differences are 1.9e-10 .. 7.3e-08 of a scale entry, the
    largest for camera 0's roll; both fits take 6 residual evaluations; the start's residuals differ by at most
    1.2e-13 px."""
    import scipy.optimize
    import scipy.sparse
    from oracle import camera as oc

    g = golden("calib_fit.npz")
    inner = fit_internals(g)
    vectors = [oc.make_camera(imgsz=inner["imgsz"], f=float(g["start_f"]), c=inner["c"], k=inner["k"], p=inner["p"], viewdir=v)
               for v in g["start_viewdirs"]]
    controls = []
    for i in range(len(vectors)):
        controls += [("points", i, g[f"points{i}_uv"], g[f"points{i}_xyz"]), ("lines", i, g[f"lines{i}_uv"], [g["horizon"]])]
    model = rs.HostModel(vectors, controls)
    start = model.residuals(g["x0"])
    print("start residuals: max |difference| =", np.abs(start - g["residuals_start"].ravel()).max())
    np.testing.assert_allclose(start.reshape(-1, 2) + np.vstack([c[2] for c in controls]), g["predicted_start"], **TOL)
    result = scipy.optimize.least_squares(model.residuals, g["x0"], bounds=(g["lower"], g["upper"]), x_scale=g["scales"],
                                          jac_sparsity=scipy.sparse.csr_matrix(g["sparsity"]))
    assert result.success
    scaled = np.abs(result.x - g["fit_x"]) / g["scales"]
    print("fit: |difference| / scales =", scaled, "nfev", result.nfev, "reference", int(g["fit_nfev"]))
    assert (scaled < 1e-3).all()


def test_fit_serves_the_default_method_only(golden):
    model = fit_model(golden("calib_fit.npz"))
    with pytest.raises(NotImplementedError, match="lmfit is not installed"):
        model.fit(method="leastsq")
    with pytest.raises(NotImplementedError, match="out of scope"):
        model.plot()
    with pytest.raises(NotImplementedError, match="out of scope"):
        model.controls[1].plot()
    with pytest.raises(RuntimeError, match="upload"):
        model.jacobian()


def test_weights_sizes_and_resize(golden):
    import glimpse_amd
    from glimpse_amd.optimize import Lines, Points

    g = golden("calib_fit.npz")
    model = fit_model(g)
    assert model.size == sum(c.size for c in model.controls) == len(g["predicted_start"])
    assert np.array_equal(model.observed(), np.vstack([c.observed() for c in model.controls]))
    model.weights = np.arange(1, model.size + 1)
    assert model.weights.shape == (model.size, 1) and np.isclose(model.weights.sum(), model.size)
    cam = glimpse_amd.Camera(imgsz=10, f=1)
    points = Points(cam=cam, uv=[(5, 5)], xyz=[(0, 1, 0)])
    points.resize(0.5)
    assert cam.imgsz.tolist() == [5, 5] and points.uv.tolist() == [[2.5, 2.5]]
    cam.resize(1)
    points.resize()
    assert points.uv.tolist() == [[5, 5]]
    lines = Lines(cam=cam, uvs=[[(2, 4), (4, 4)], [(6, 4), (8, 4)]], xyzs=[[(-10, 1, 0), (0, 1, 0), (10, 1, 0)]], density=10)
    assert lines.size == 4
    lines.resize(0.5)
    assert lines.uv.tolist() == [[1, 2], [2, 2], [3, 2], [4, 2]] and lines.uvs[1].tolist() == [[3, 2], [4, 2]]
    with pytest.raises(ValueError, match="Image and world coordinates have different length"):
        Points(cam=cam, uv=[(5, 5)], xyz=[(0, 1, 0), (0, 2, 0)])
    moved = Points(cam=cam, uv=[(5, 5)], xyz=[(0, 1, 0)], directions=True)
    cam.xyz = (1, 0, 0)
    with pytest.raises(ValueError, match="Camera position has changed and world coordinates are ray directions"):
        moved._test_position()


def test_the_wide_model_meets_the_conditions_of_the_gpu_test():
    """tests/calib_cases.py, asserted without a device: the rows of every control and of every job of one Jacobian, the
    interleaving of the kinds, the distortion, and -- by the formulas of oracle/camera.py -- that the NaN rows of Points
    behind the camera and of match rays behind the other camera lie in a job's second and later workgroups."""
    from glimpse_amd import optimize
    from tests import calib_cases as cc

    model, cams = cc.model()
    kinds = {optimize.Points: "points", optimize.Lines: "lines", optimize.Matches: "matches",
             optimize.RotationMatches: "rotation", optimize.RotationMatchesXY: "rotation_xy"}
    assert [(kinds[type(c)], c.size) for c in model.controls] == [(k, n) for k, _, n in cc.CONTROLS]
    rows = {k: sorted(n for kind, _, n in cc.CONTROLS if kind == k) for k in kinds.values()}
    assert rows == {"points": [1, 255, 256, 257, 600], "lines": [300], "matches": [257, 1000], "rotation": [257, 1000],
                    "rotation_xy": [257, 1000]}
    assert all(cam.k.all() and cam.p.all() for cam in cams) and len(cams) == 3
    first = np.concatenate(([0], np.cumsum([n for _, _, n in cc.CONTROLS])))[:-1]
    assert all(first[i] > 0 for i, (_, _, n) in enumerate(cc.CONTROLS) if n > cc.TB)  # no wide job at row 0 of the output
    order = [k for k, _, _ in cc.CONTROLS]
    assert order.index("points") < order.index("matches") < order.index("lines") < len(order) - 1 - order[::-1].index("points")
    sets, dx, jobs = model._jacobian_plan()
    assert len(sets) == 10 and len(dx) == 9 and jobs[:12] == [(i, 0) for i in range(12)] and len(jobs) > 12
    assert {s for _, s in jobs} == set(range(10)) and max(model.controls[i].size for i, _ in jobs) == 1000
    assert sum(model.controls[i].size > cc.TB for i, _ in jobs) >= 30  # jobs of two to four workgroups
    vectors = cc.oracle_vectors()
    for cam, vector in zip(cams, vectors):
        assert np.array_equal(cam.vector24[:20], vector[:20])
    for n, ((kind, members, size), arrays) in enumerate(zip(cc.CONTROLS, cc.data())):
        if kind == "lines":
            continue
        for side in ((0,) if kind == "points" else (0, 1)):
            nan = np.flatnonzero(np.isnan(cc.oracle_predicted(kind, vectors, members, arrays, side)).any(axis=1))
            print(n, kind, size, "rows, side", side, ":", len(nan), "NaN rows", nan[:8])
            if kind == "points":
                assert nan.tolist() == list(cc.BEHIND.get(n, ()))
            elif kind == "matches":
                assert 0 < len(nan) < size // 4 and (size == 257 or (nan >= 2 * cc.TB).any()) and (nan >= cc.TB).any()
            else:
                assert nan.tolist() == list(cc.FAR[n])
    assert all(max(rows) >= cc.TB for rows in list(cc.BEHIND.values())[1:] + list(cc.FAR.values()))
    # the Lines control between them: more projected points than one LDS tile of the nearest kernel, and no near tie
    lines, v = model.controls[3], vectors[0]
    xy_edges = oc_undistorted_edges(cams[0], v)
    info = {}
    rs.lines_predicted(v, cams[0].R, lines.uv, lines.xyzs, np.hstack((xy_edges.min(axis=0), xy_edges.max(axis=0))), info=info)
    print("lines:", info["n_projected"], "projected points, gap", info["gap"])
    assert info["n_projected"] > rs.TILE and info["gap"] > MIN_GAP


def oc_undistorted_edges(cam, vector):
    """The camera coordinates of the image's edge points (the clip box's corners and mid-points) by oracle/camera.py."""
    from oracle import camera as oc

    return oc.undistort(vector, (cam.edges(step=cam.imgsz / 2) - (vector[6:8] / 2 + vector[10:12])) * (1 / vector[8:10]))
