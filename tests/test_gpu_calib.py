"""The camera calibration on the device (glh_calib_*): Lines.predicted against its NumPy restatement
(tests/calib_restated.py) bit for bit, the handle's evaluation of every kind of job against the package's
one-control-at-a-time `predicted`, Cameras.jacobian against SciPy's own differences of the sequential residuals,
Cameras.fit against the sequential fit and the reference's, and the handle's hygiene."""
import contextlib
import io

import numpy as np
import pytest

from tests import calib_restated as rs
from tests.test_calib_host import MIN_GAP, TOL, fit_internals, fit_model, split

pytestmark = pytest.mark.gpu

T = rs.TILE
INTERNALS = (dict(imgsz=(400, 300), f=(500, 505), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0, 0)),
             dict(imgsz=(400, 300), f=(500, 505), c=(3, -2), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.003), p=(0.001, -0.002)))


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def restated(lines, index=slice(None), info=None):
    """The restatement fed the package's own camera, rotation matrix and clip box."""
    from glimpse_amd.optimize import _clip_box

    cam = lines.cam
    return rs.lines_predicted(cam.vector24, cam.R, lines.uv[index], lines.xyzs, _clip_box(cam), directions=lines.directions,
                              density=lines.density, info=info)


@pytest.mark.parametrize("c", (0, 1))
def test_lines_equal_the_restatement_at_the_tile_edges(c):
    """A straight line across the frame whose projected point count is T - 1, T, T + 1 and 2 T + 3 (T: the LDS tile of
    the nearest kernel; the count is asserted), against 1, 63, 64, 65 and 257 observed points (either side of a wave and
    of a workgroup): bit for bit, and the same bytes from a second call."""
    import glimpse_amd
    from glimpse_amd.optimize import Lines

    rng = np.random.default_rng(40 + c)
    cam = glimpse_amd.Camera(viewdir=(0, 0, 0), **INTERNALS[c])
    for target, density in ((T - 1, 1), (T, 1), (T + 1, 1), (2 * T + 3, 2)):
        # camera coordinates x = X / Y: a line of (target - 0.3) steps of 1 / (density f) rounds to `target` points
        length = (target - 0.3) / (density * cam.f.max())
        world = np.array([[-0.5 * length * 1000.0, 1000.0, 20.0], [0.1 * length * 1000.0, 1000.0, 20.0],
                          [0.5 * length * 1000.0, 1000.0, 20.0]])
        for n_observed in (1, 63, 64, 65, 257):
            uv = np.column_stack((rng.uniform(60, 340, n_observed), rng.uniform(100, 200, n_observed)))
            lines = Lines(cam, uvs=[uv], xyzs=[world], density=density)
            info = {}
            want = restated(lines, info=info)
            assert info["n_projected"] == target and info["gap"] > MIN_GAP
            got, again = lines.predicted(), lines.predicted()
            assert same(got, want) and same(got, again), (target, n_observed)


@pytest.mark.parametrize("c", (0, 1))
@pytest.mark.parametrize("name", ("main", "dense", "fallback"))
def test_lines_equal_the_restatement_on_the_polylines(golden, c, name):
    """The reference's scenes -- in frame, leaving and re-entering, vertices behind the camera, shorter than a step; and
    wholly out of frame, the fallback -- with and without k[3:6] and p, index subsets included; and against the
    reference's own `predicted` within the image-coordinate tolerance."""
    from glimpse_amd.optimize import Lines
    from tests.test_calib_host import camera_of

    g = golden("calib_lines.npz")
    key = f"cam{c}_{name}"
    cam = camera_of(g[f"cam{c}_vector"])
    lines = Lines(cam, uvs=split(g[f"{key}_uv"], g[f"{key}_uv_off"]), xyzs=split(g[f"{key}_xyz"], g[f"{key}_xyz_off"]),
                  density=float(g[f"{key}_density"]))
    info = {}
    got = lines.predicted()
    assert same(got, restated(lines, info=info)) and info["gap"] > MIN_GAP
    assert same(got, lines.predicted())
    np.testing.assert_allclose(got, g[f"{key}_predicted"], **TOL)
    for index in (g[f"{key}_index"], slice(5, None, 7), np.arange(lines.size) % 2 == 0, [0]):
        assert same(lines.predicted(index=index), restated(lines, index=index))
    np.testing.assert_allclose(lines.predicted(index=g[f"{key}_index"]), g[f"{key}_predicted_index"], **TOL)
    assert [len(p) for p in lines._xyzs_to_uvs()] == g[f"{key}_counts"].tolist()
    assert lines.predicted(index=[]).shape == (0, 2)


def test_lines_nan_observed_point_and_ray_directions():
    """A NaN observed point takes projected point 0 (np.argmin); world lines as ray directions."""
    import glimpse_amd
    from glimpse_amd.optimize import Lines

    cam = glimpse_amd.Camera(viewdir=(1, 2, 0.5), **INTERNALS[1])
    az = np.deg2rad(np.linspace(-12, 12, 9))
    rays = np.column_stack((np.sin(az), np.cos(az), 0.05 * np.cos(5 * az)))
    uv = np.array([[100.0, 150.0], [np.nan, 150.0], [300.0, np.nan], [200.0, 140.0]])
    lines = Lines(cam, uvs=[uv], xyzs=[rays], directions=True)
    got = lines.predicted()
    assert same(got, restated(lines))
    first = np.vstack(lines._xyzs_to_uvs())[0]
    assert same(got[1], first) and same(got[2], first)


def sequential(model, sets, jobs):
    """Every job by the package's one-control-at-a-time `predicted`, with the cameras set to the job's set."""
    saved = [cam._vector for cam in model.cams]
    out = []
    try:
        for i, s in jobs:
            for cam, vector in zip(model.cams, sets[s]):
                cam._vector = vector
            out.append(model.controls[i].predicted())
    finally:
        for cam, vector in zip(model.cams, saved):
            cam._vector = vector
    return out


def rotation_model(g):
    """Points plus the two rotation match kinds (and a Matches control to a camera that is not fitted): view directions
    only, since the rotation kinds hold the internal parameters fixed."""
    import glimpse_amd
    from glimpse_amd.optimize import Cameras, Matches, Points, RotationMatches, RotationMatchesXY

    cams = [glimpse_amd.Camera(f=float(g["start_f"]), viewdir=v, **fit_internals(g)) for v in g["start_viewdirs"]]
    fixed = cams.pop()
    controls = [Points(cams[0], uv=g["points0_uv"], xyz=g["points0_xyz"]),
                RotationMatches(cams=[cams[0], cams[1]], uvs=[g["matches0_uv0"], g["matches0_uv1"]]),
                RotationMatchesXY(cams=[cams[0], cams[1]], uvs=[g["matches0_uv0"], g["matches0_uv1"]]),
                Matches(cams=[cams[1], fixed], uvs=[g["matches1_uv0"], g["matches1_uv1"]])]
    return Cameras(cams, controls, cam_params=[{"viewdir": True}] * 2)


@pytest.mark.parametrize("which", ("fit", "rotation"))
def test_handle_evaluation_equals_one_control_at_a_time(golden, which):
    """One job, every control at the base set, and the full job list of one Jacobian: bit for bit."""
    g = golden("calib_fit.npz")
    model = fit_model(g, matches=True) if which == "fit" else rotation_model(g)
    sets, _, jobs = model._jacobian_plan()
    assert len(jobs) > len(model.controls) and {i for i, _ in jobs} == set(range(len(model.controls)))
    with model.upload() as handle:
        for job_list in ([jobs[-1]], [jobs[0]], jobs[:len(model.controls)], jobs):
            got = model._evaluate(handle, sets, job_list)
            want = sequential(model, sets, job_list)
            assert len(got) == len(want) and all(same(a, b) for a, b in zip(got, want)), len(job_list)
        through = model.predicted()
        assert same(through, np.vstack(sequential(model, sets, jobs[:len(model.controls)])))
        _, times = model._evaluate(handle, sets, jobs, return_times=True)
        assert set(times) == {"upload", "points", "line_points", "nearest", "download", "segment_tables_host"}
        assert all(t >= 0 for t in times.values())
    assert not handle._h and model._open() is None
    assert same(model.predicted(), through)  # (control by control again)
    if which == "fit":
        np.testing.assert_allclose(through, g["predicted_start_matches"], **TOL)
        np.testing.assert_allclose(model.controls[6].predicted(cam=1), g["matches0_predicted1"], **TOL)
    else:
        np.testing.assert_allclose(through[15:80], g["matches0_rotation_predicted0"], **TOL)
        np.testing.assert_allclose(through[80:145], g["matches0_xy_predicted0"], rtol=1e-11, atol=1e-12)


def test_match_jobs_predict_in_either_camera(golden):
    """job_side 1: the second camera predicts from the first's points, for the three match kinds."""
    from glimpse_amd.camera import rotations

    g = golden("calib_fit.npz")
    model = rotation_model(g)
    with model.upload() as handle:
        cams24 = np.array([[cam.vector24 for cam in model._dev_cams]])
        rot = rotations(cams24[0, :, 3:6])[0][None]
        for i in (1, 2, 3):
            for side in (0, 1):
                got = handle.eval(cams24, rot, [i], [0], job_side=[side])
                assert same(got, model.controls[i].predicted(cam=side)), (i, side)


def jacobian_model(g):
    """Three cameras, a group f, per-camera viewdir, and camera 0's k[0] sitting at its upper bound; Points, Lines and
    Matches."""
    model = fit_model(g, matches=True)
    from glimpse_amd.optimize import Cameras

    k0 = float(model.cams[0].k[0])
    return Cameras(model.cams, model.controls, cam_params=[{"viewdir": True, "k": ([0], -0.13, k0)}, {"viewdir": True}, {"viewdir": True}],
                   group_params={"f": True})


def test_jacobian_equals_scipys_differences_of_the_sequential_residuals(golden):
    from scipy.optimize._numdiff import approx_derivative

    g = golden("calib_fit.npz")
    model = jacobian_model(g)
    x0, lb, ub = model._values_bounds()
    k0 = list(model.params).index("cam0_k0")
    assert len(x0) == 12 and x0[k0] == ub[k0]  # (at its upper bound: the step turns round)
    assert model._steps(x0, lb, ub)[k0] < 0 < model._steps(x0, lb, ub)[0]

    def fun(x):
        assert model._open() is None
        return model.residuals(x).ravel()

    for index in (slice(None), np.arange(0, model.size, 3)):
        def fun_index(x):
            return model.residuals(x, index=index).ravel()

        structure = model.sparsity
        if not isinstance(index, slice):
            structure = structure.tocsr()[np.dstack((2 * index, 2 * index + 1)).ravel()]
        want = approx_derivative(fun_index, x0, method="2-point", f0=fun_index(x0), bounds=(lb, ub), sparsity=structure)
        with model.upload():
            got = model.jacobian(x0, index=index)
            again = model.jacobian(index=index)
        assert got.shape == want.shape and same(got.toarray(), want.toarray()) and same(got.toarray(), again.toarray())
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
        assert same(got.data, want.data)  # (the stored entries themselves: -0.0 where SciPy has -0.0)
    # without a sparsity structure: every block, dense
    from glimpse_amd.optimize import Cameras

    dense = Cameras(model.cams, model.controls, cam_params=model.cam_params, group_params=model.group_params, sparsity=False)
    want = approx_derivative(fun, x0, method="2-point", f0=fun(x0), bounds=(lb, ub))
    with dense.upload():
        assert same(dense.jacobian(x0), want)


def test_fit_equals_the_sequential_fit_and_the_references(golden):
    """Cameras.fit with the batched Jacobian against scipy.optimize.least_squares on the same residuals, one set at a
    time, with SciPy's own differences: bit for bit.  Against the reference's fit: within 1e-3 of each parameter's scale
    (measured on an MI355X, printed below: 2.2e-9 .. 5.4e-8)."""
    import scipy.optimize

    g = golden("calib_fit.npz")
    model = fit_model(g)
    x0, lb, ub = model._values_bounds()

    def fun(x):
        assert model._open() is None
        return model.residuals(x).ravel()

    want = scipy.optimize.least_squares(fun, x0, bounds=(lb, ub), x_scale=model.scales, jac_sparsity=model.sparsity)
    text = io.StringIO()
    with contextlib.redirect_stdout(text):
        got = model.fit(full=True)
        values = model.fit()
    assert got.success and want.success and same(got.x, want.x) and same(values, got.x)
    assert got.nfev == want.nfev and list(got.params) == g["labels"].tolist()
    assert [v[0] for v in got.params.values()] == got.x.tolist()
    assert text.getvalue().startswith("\r") and text.getvalue().endswith("\n")
    scaled = np.abs(got.x - g["fit_x"]) / g["scales"]
    print("fit against the reference: |difference| / scales =", scaled)
    assert (scaled < 1e-3).all()
    assert model._open() is None and np.array_equal([cam.viewdir for cam in model.cams], g["start_viewdirs"])
    rmse = float(np.sqrt((model.errors(params=values) ** 2).mean()))
    assert abs(rmse - float(g["rmse_fit"])) < 1e-6 and rmse < float(g["rmse_start"])


def test_errors_and_hygiene(golden):
    import glimpse_amd
    from glimpse_amd import _lib
    from glimpse_amd.optimize import Cameras, Matches, Points, RotationMatches

    g = golden("calib_fit.npz")
    cams = [glimpse_amd.Camera(f=float(g["start_f"]), viewdir=v, **fit_internals(g)) for v in g["start_viewdirs"][:2]]
    uvs = [g["matches0_uv0"], g["matches0_uv1"]]
    points = [Points(cam, uv=g[f"points{i}_uv"], xyz=g[f"points{i}_xyz"]) for i, cam in enumerate(cams)]
    # RotationMatches under a varied f
    model = Cameras(cams, points + [RotationMatches(cams=cams, uvs=uvs)], group_params={"f": True})
    with model.upload() as handle:
        base = model.predicted()
        with pytest.raises(ValueError, match=r"Camera internal parameters \(imgsz, f, c, k, p\) have changed"):
            model.jacobian()
        # Matches between cameras that a parameter moves apart
        moving = Cameras(cams, points + [Matches(cams=cams, uvs=uvs)], cam_params=[{"xyz": True}, {}])
        with moving.upload():
            with pytest.raises(ValueError, match="Cameras have different positions"):
                moving.jacobian()
        # ray directions with a moved camera
        rays = Points(cams[0], uv=g["points0_uv"], xyz=g["points0_xyz"], directions=True)
        moved = Cameras(cams[:1], [rays], cam_params=[{"xyz": 0}])
        with moved.upload():
            with pytest.raises(ValueError, match="Camera position has changed and world coordinates are ray directions"):
                moved.jacobian()
        # invalid calls leave the handle usable
        cams24 = np.array([[cam.vector24 for cam in model._dev_cams]])
        rot = np.array([[cam.R for cam in model._dev_cams]])
        for bad in (dict(job_control=[7], job_set=[0]), dict(job_control=[0], job_set=[1]),
                    dict(job_control=[2], job_set=[0], job_side=[2]),
                    dict(job_control=[0], job_set=[0], tables=[(np.array([0, 2]), np.array([3]), np.zeros((1, 5)), np.zeros((2, 3)))])):
            with pytest.raises(_lib.GlhError) as err:
                handle.eval(cams24, rot, **bad)
            assert err.value.code != 0
        grid = cams24.copy()
        grid[0, 0, 23] = 1.0
        with pytest.raises(_lib.GlhError):
            handle.eval(grid, rot, [0], [0])
        with pytest.raises(ValueError):
            handle.eval(cams24[:, :1], rot, [0], [0])
        assert same(model.predicted(), base)
        assert [cam.f.tolist() for cam in cams] == [[float(g["start_f"])] * 2] * 2
    assert not handle._h
    handle.close()  # (twice: nothing)
    with pytest.raises(_lib.GlhError, match="closed"):
        handle.eval(cams24, rot, [0], [0])
    # a Lines job without a segment table, and a lines-only handle that is empty
    with _lib.Calib(1, [_lib.CALIB_KINDS["lines"]], [0], [0], [0], [0, 2], np.zeros((2, 2)), np.zeros((2, 3))) as lonely:
        with pytest.raises(_lib.GlhError):
            lonely.eval(cams24[:, :1], rot[:, :1], [0], [0])
    with pytest.raises(_lib.GlhError):
        _lib.Calib(1, [9], [0], [0], [0], [0, 2], np.zeros((2, 2)), np.zeros((2, 3)))
    with pytest.raises(_lib.GlhError):
        _lib.Calib(1, [0], [1], [0], [0], [0, 2], np.zeros((2, 2)), np.zeros((2, 3)))


# ---- row jobs wider than a workgroup (tests/calib_cases.py; tests/test_calib_host.py asserts what the model holds) ----
def _count(got, want):
    """(blocks that differ in shape, values that differ in any bit) between two lists of blocks."""
    shapes = sum(a.shape != b.shape for a, b in zip(got, want)) + abs(len(got) - len(want))
    return shapes, sum(int(np.count_nonzero(_bits(a) != _bits(b))) for a, b in zip(got, want) if a.shape == b.shape)


@pytest.fixture(scope="module")
def wide():
    """The wide model with its handle open, the plan of one Jacobian and every job of it one control at a time."""
    from tests import calib_cases as cc

    model, cams = cc.model()
    sets, _, jobs = model._jacobian_plan()
    want = sequential(model, sets, jobs)
    with model.upload() as handle:
        yield dict(model=model, cams=cams, sets=sets, jobs=jobs, want=want, handle=handle)


def test_wide_jobs_equal_one_control_at_a_time(wide):
    """Jobs of up to four workgroups of k_calib_rows (CalBlock.first 0, 256, 512, 768) between and behind other jobs, the
    Lines job's blocks among them, NaN rows in the later workgroups: the full job list of one Jacobian, the list
    reversed, and the largest job alone, bit for bit; and the same bytes from a second call."""
    model, sets, jobs, want, handle = (wide[k] for k in ("model", "sets", "jobs", "want", "handle"))
    sizes = [model.controls[i].size for i, _ in jobs]
    largest = int(np.argmax(sizes))
    assert sizes[largest] == 1000 and sum(sizes) > 30000
    for name, picked in (("full", list(range(len(jobs)))), ("reversed", list(range(len(jobs)))[::-1]), ("largest", [largest])):
        got = model._evaluate(handle, sets, [jobs[q] for q in picked])
        again = model._evaluate(handle, sets, [jobs[q] for q in picked])
        expected = [want[q] for q in picked]
        print(name, len(picked), "jobs,", sum(sizes[q] for q in picked), "rows: blocks of another shape, differing values:",
              _count(got, expected), "; second call:", _count(again, got), "; NaN rows",
              int(sum(np.isnan(b).any(axis=1).sum() for b in got)))
        assert _count(got, expected) == (0, 0) and _count(again, got) == (0, 0), name
    assert sum(np.isnan(b).any(axis=1).sum() for b in want[:12]) >= 100  # (NaN equals NaN bit for bit above)


def test_wide_match_jobs_predict_in_the_second_camera(wide):
    """job_side 1 on the three match kinds at 1000 rows."""
    from glimpse_amd.camera import rotations
    from tests import calib_cases as cc

    model, handle = wide["model"], wide["handle"]
    cams24 = np.array([[cam.vector24 for cam in model._dev_cams]])
    rot = rotations(cams24[0, :, 3:6])[0][None]
    picked = [i for i, (kind, _, rows) in enumerate(cc.CONTROLS) if rows == 1000]
    assert [cc.CONTROLS[i][0] for i in picked] == ["rotation", "matches", "rotation_xy"]
    for i in picked:
        got = handle.eval(cams24, rot, [i], [0], job_side=[1])
        again = handle.eval(cams24, rot, [i], [0], job_side=[1])
        expected = model.controls[i].predicted(cam=1)
        print(cc.CONTROLS[i], "side 1: differing values", _count([got], [expected]), "second call", _count([again], [got]))
        assert same(got, expected) and same(again, got), i
        assert not same(got, wide["want"][i])  # (the other side's prediction is another one)


def test_wide_jobs_against_the_oracle(wide):
    """The base set's twelve jobs against formulas that are not the package's: oracle/camera.py for Points and the
    match kinds (both sides), the restatement for Lines.  Tolerances: TOL for image coordinates, rtol 1e-11 / atol 1e-12
    for camera coordinates, as the existing camera tests."""
    from glimpse_amd.camera import rotations
    from tests import calib_cases as cc

    model, handle = wide["model"], wide["handle"]
    got = model._evaluate(handle, wide["sets"], wide["jobs"][:12])
    vectors = cc.oracle_vectors()
    cams24 = np.array([[cam.vector24 for cam in model._dev_cams]])
    rot = rotations(cams24[0, :, 3:6])[0][None]
    for i, ((kind, members, rows), arrays) in enumerate(zip(cc.CONTROLS, cc.data())):
        if kind == "lines":
            info = {}
            expected = restated(model.controls[i], info=info)
            assert info["gap"] > MIN_GAP and info["n_projected"] > T
            print(i, kind, rows, "rows,", info["n_projected"], "projected points: differing values", _count([got[i]], [expected]))
            assert same(got[i], expected)
            continue
        tol = dict(rtol=1e-11, atol=1e-12) if kind == "rotation_xy" else TOL
        for side in ((0,) if kind == "points" else (0, 1)):
            found = got[i] if side == 0 else handle.eval(cams24, rot, [i], [0], job_side=[1])
            expected = cc.oracle_predicted(kind, vectors, members, arrays, side)
            nan = np.isnan(expected).any(axis=1)
            with np.errstate(invalid="ignore"):
                excess = np.abs(found - expected) - (tol["atol"] + tol["rtol"] * np.abs(expected))
            print(i, kind, rows, "rows, side", side, ":", int(nan.sum()), "NaN rows; largest |difference| - tolerance",
                  float(np.nanmax(excess)) if not nan.all() else None)
            assert np.array_equal(np.isnan(found), np.isnan(expected))
            np.testing.assert_allclose(found, expected, **tol)
