"""`optimize.ransac(batched=True)` and `glh_calib_fit_sets` on the GPU, on the designed cases of tests/ransac_cases.py
(admitted on the CPU by tests/test_ransac_cases.py): the device's fit of every hypothesis against `Cameras.fit` on the
existing path, its consensus masks against `Cameras.errors`, the whole call against the host loop, repeated calls byte for
byte, what fails and what is refused, and the reference's own scenario (SIFT, match, RANSAC recovers a 2 degree turn)."""
import contextlib
import datetime
import io

import numpy as np
import pytest

from tests import ransac_cases as rc

pytestmark = pytest.mark.gpu
CRITERION = 1e-3  # |difference| / scales, the calibration's own criterion (tests/test_gpu_calib.py)


def quiet(f, *args, **kwargs):
    """f(...) without the progress lines Cameras.fit writes."""
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*args, **kwargs)


def samples_of(name):
    from glimpse_amd.optimize import _ransac_samples

    np.random.seed(rc.CASES[name]["seed"])
    call = rc.call(name)
    return list(_ransac_samples(n=call["n"], size=sum(rows for _, rows in rc.CASES[name]["controls"]), iterations=call["iterations"]))


def device_fit(model, sets, max_error=None, **kwargs):
    """handle.fit_sets of the row sets `sets` from the model's current values, as optimize._ransac_batched calls it."""
    from glimpse_amd.optimize import _batched_plan

    plan = _batched_plan(model, {})
    offset = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int64)
    rows = np.concatenate([np.asarray(s, dtype=np.int64) for s in sets])
    with model.upload() as handle:
        cams24 = np.array([cam.vector24 for cam in model._dev_cams])
        out = handle.fit_sets(cams24, 0, plan["slots"], plan["x0"], plan["lb"], plan["ub"], plan["x_scale"], offset, rows,
                              weights=plan["weights"], observed=plan["observed"], max_error=max_error, **kwargs)
    model._handle = None
    return out


def test_every_hypothesis_fits_like_cameras_fit():
    """The clean case (no outliers; samples of 70 rows) and three sets of 5, 130 and all 257 rows in one call: the device's
    values against `model.fit(rows)`, |difference| / scales < 1e-3.  Measured on an MI355X (printed below): the largest
    ratio is 2.2e-7."""
    model, _ = rc.model("clean_257")
    sets = samples_of("clean_257") + [np.arange(5), np.arange(100, 230), np.arange(257)]
    assert sorted(len(s) for s in sets)[-3:] == [70, 130, 257]
    values, status, mean_error = device_fit(model, sets)
    assert (status > 0).all(), status
    worst = 0.0
    for s, got, mean in zip(sets, values, mean_error):
        want = quiet(model.fit, list(s))
        worst = max(worst, float((np.abs(got - want) / model.scales).max()))
        assert abs(mean - model.errors(want, list(s)).mean()) < 1e-6
    print("device fit against Cameras.fit: largest |difference| / scales =", worst)
    assert worst < CRITERION


def test_camera_coordinate_matches_fit_and_score():
    """RotationMatchesXY, whose residuals are in normalised camera coordinates (a pixel is 1 / f of them), on the rows of
    the rotation case: sets of its inliers against `model.fit(rows)` within 1e-3 of `scales`, and the masks at an error
    of 3 px / f against `model.errors`.  Measured on an MI355X (printed below): the largest ratio is 1.7e-5
    (gtol is absolute, and these residuals are 1 / f of a pixel's)."""
    from glimpse_amd import optimize

    rotation, d = rc.model("rotation_129")
    control = rotation.controls[0]
    model = optimize.Cameras(rotation.cams, [optimize.RotationMatchesXY(cams=control.cams, xys=control.xys)],
                             cam_params=[{"viewdir": True}])
    good = np.flatnonzero(d["inlier"])
    sets = [good[:2], good[5:70], good]
    max_error = rc.MAX_ERROR / rc.F[0]
    values, status, _, inlier = device_fit(model, sets, max_error=max_error)
    assert (status > 0).all(), status
    worst = 0.0
    for rows, x, mask in zip(sets, values, inlier):
        want = quiet(model.fit, list(rows))
        worst = max(worst, float((np.abs(x - want) / model.scales).max()))
        expected = (model.errors(x) < max_error).astype(np.uint8)
        expected[rows] = 2
        assert np.array_equal(mask, expected)
    print("camera coordinates: largest |difference| / scales =", worst, "; outliers left out by the last set",
          int((inlier[-1] == 0).sum()), "of", int((~d["inlier"]).sum()))
    assert worst < CRITERION and (inlier[-1] == 0).sum() == (~d["inlier"]).sum()


@pytest.mark.parametrize("name", list(rc.CASES))
def test_consensus_masks_equal_the_errors_of_the_existing_path(name):
    """Under the device's own fitted values: inlier == 1 exactly where `model.errors(values) < max_error` outside the
    sample, 2 on the sample's rows, nothing for a hypothesis whose fit failed."""
    model, _ = rc.model(name)
    samples = samples_of(name)
    values, status, _, inlier = device_fit(model, samples, max_error=rc.MAX_ERROR)
    assert inlier.shape == (len(samples), model.size) and (status > 0).any()
    for sample, x, ok, mask in zip(samples, values, status, inlier):
        if ok <= 0:
            assert not (mask == 1).any()
            continue
        with np.errstate(invalid="ignore"):
            want = (model.errors(x) < rc.MAX_ERROR).astype(np.uint8)
        want[sample] = 2
        assert np.array_equal(mask, want), (name, np.flatnonzero(mask != want))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_the_batched_call_equals_the_host_loop(name):
    """Under the same np.random.seed: the same inliers exactly, the values within 1e-3 of each parameter's scale (the two
    calls may pick different representatives of one set, which reorders the rows of the final fit), and the same use of
    np.random."""
    from glimpse_amd import optimize

    model, _ = rc.model(name)
    seed = rc.CASES[name]["seed"]
    np.random.seed(seed)
    params, inliers, info = quiet(optimize.ransac, model, batched=True, return_info=True, **rc.call(name))
    after = np.random.get_state()[1].copy()
    np.random.seed(seed)
    want_params, want_inliers = quiet(optimize.ransac, model, **rc.call(name))
    assert np.array_equal(after, np.random.get_state()[1])
    ratio = float((np.abs(params - want_params) / model.scales).max())
    print(name, ": |difference| / scales =", ratio, "; hypotheses", len(info["status"]), "converged", int((info["status"] > 0).sum()),
          "distinct sets", len(info["sets"]), "winner", info["winner"], "times_ms", info["times_ms"])
    assert np.array_equal(inliers, want_inliers) and ratio < CRITERION
    assert model._handle is None and np.array_equal(model.cams[0].viewdir, rc.data(name)["start"][3:6])
    assert set(info["times_ms"]) >= {"upload", "fit_score", "refit", "download", "final_fit"}
    assert len(info["sets"]) == len(info["mean_errors"]) == len(info["hypothesis"]) and 0 <= info["winner"] < len(info["sets"])


def test_a_repeated_call_returns_the_same_bytes():
    from glimpse_amd import optimize

    model, _ = rc.model("two_kinds_257")
    samples = samples_of("two_kinds_257")
    first, second = (device_fit(model, samples, max_error=rc.MAX_ERROR) for _ in range(2))
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
    runs = []
    for _ in range(2):
        np.random.seed(9)
        runs.append(quiet(optimize.ransac, model, batched=True, return_info=True, **rc.call("two_kinds_257")))
    for key in ("values", "status", "consensus", "mean_errors", "refit_values"):
        assert runs[0][2][key].tobytes() == runs[1][2][key].tobytes(), key
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][2]["sets"], runs[1][2]["sets"]))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and np.array_equal(runs[0][1], runs[1][1])


def test_no_set_qualifies_and_a_sample_behind_the_camera_is_skipped(monkeypatch):
    from glimpse_amd import optimize

    model, d = rc.model("behind_128")
    call = rc.call("behind_128")
    with pytest.raises(ValueError, match="Best fit does not meet acceptance criteria"):
        np.random.seed(5)
        quiet(optimize.ransac, model, batched=True, **{**call, "min_inliers": 127})
    # the first sample: six rows behind the camera
    with np.errstate(invalid="ignore"):
        behind = np.flatnonzero(np.isnan(model.predicted()).any(axis=1))
    assert len(behind) == rc.CASES["behind_128"]["behind"]
    values, status, mean_error, inlier = device_fit(model, [behind[:6], np.arange(128)], max_error=rc.MAX_ERROR)
    assert status[0] == -1 and np.isnan(mean_error[0]) and not (inlier[0] == 1).any() and status[1] > 0
    assert np.isnan(mean_error[1])  # (np.mean over a set with rows that have no prediction)
    drawn = optimize._ransac_samples

    def samples(**kwargs):
        yield [int(r) for r in behind[:6]]
        yield from drawn(**kwargs)

    monkeypatch.setattr(optimize, "_ransac_samples", samples)
    np.random.seed(5)
    params, inliers, info = quiet(optimize.ransac, model, batched=True, return_info=True, **call)
    assert info["status"][0] == -1 and info["consensus"][0] == 0 and len(info["status"]) == call["iterations"] + 1
    monkeypatch.undo()
    np.random.seed(5)
    want_params, want_inliers = quiet(optimize.ransac, model, **call)
    assert np.array_equal(inliers, want_inliers) and (np.abs(params - want_params) / model.scales).max() < CRITERION


def test_what_is_refused_is_refused_before_the_library(monkeypatch):
    import glimpse_amd
    from glimpse_amd import _lib, optimize

    model, d = rc.model("two_kinds_257")
    call = rc.call("two_kinds_257")
    fitted, other = model.cams[0], model.controls[1].cams[1]
    points, matches = model.controls
    lines = optimize.Lines(fitted, uvs=[points.uv[:5]], xyzs=[points.xyz[:5]])

    class GridCamera(glimpse_amd.Camera):
        """A camera whose 24-vector says it is a georeferenced raster image (entry 23), as `Grid.vector24` does."""

        @property
        def vector24(self):
            v = super().vector24
            v[23] = 1.0
            return v

    grid = GridCamera(xyz=fitted.xyz, viewdir=other.viewdir, imgsz=other.imgsz, f=other.f)
    refused = [
        (optimize.Cameras([fitted], [optimize.Matches(cams=[fitted, grid], uvs=matches.uvs)], cam_params=[{"viewdir": True}]), {},
         "raster grid"),
        (optimize.Cameras([grid], [optimize.Points(grid, uv=points.uv, xyz=points.xyz)], cam_params=[{"viewdir": True}]), {},
         "raster grid"),
        (optimize.Polynomial(np.random.default_rng(0).normal(size=(40, 2))), {}, "Polynomial"),
        (optimize.Cameras([fitted], [points, lines], cam_params=[{"viewdir": True}]), {}, "Lines"),
        (optimize.Cameras([fitted, other], [points, matches], cam_params=[{"viewdir": True}, {"viewdir": True}]), {}, "2 fitted cameras"),
        (optimize.Cameras([fitted], [points], group_params=[{"viewdir": True}]), {}, "group_params"),
        (optimize.Cameras([fitted], [matches], cam_params=[{"xyz": True}]), {}, "position"),
        (optimize.Cameras([fitted], [optimize.RotationMatches(cams=[fitted, other], uvs=matches.uvs, xys=matches.uvs)],
                          cam_params=[{"f": True}]), {}, "internal parameters"),
        (model, {"loss": "soft_l1"}, "loss"),
        (model, {"method": "least_squares"}, "method"),
        (model, {"jac": "3-point"}, "jac"),
        (model, {"nan_policy": "raise"}, "nan_policy"),
        (model, {"cam_params": [{"viewdir": True}]}, "cam_params"),
    ]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    for m, kwargs, word in refused:
        with pytest.raises(NotImplementedError, match=word):
            optimize.ransac(m, batched=True, **call, **kwargs)
    assert model._handle is None
    with pytest.raises(ValueError, match="batched=True"):
        optimize.ransac(model, return_info=True, **call)


def test_bad_arguments_leave_the_handle_usable():
    from glimpse_amd import _lib
    from glimpse_amd.optimize import Cameras, Lines, _batched_plan

    model, _ = rc.model("viewdir_64")
    plan = _batched_plan(model, {})
    good = dict(fit_cam=0, slots=plan["slots"], x0=plan["x0"], lb=plan["lb"], ub=plan["ub"], x_scale=plan["x_scale"],
                set_offset=[0, 4, 10], set_rows=np.arange(10))
    bad = [dict(fit_cam=1), dict(fit_cam=-1), dict(slots=[3, 4, 6]), dict(slots=[3, 3, 5]), dict(slots=[3, 4, 20]),
           dict(x0=plan["x0"] + [0, 400, 0], ub=[np.inf, 100, np.inf]), dict(x_scale=[1, 0, 1]), dict(x_scale=[1, np.nan, 1]),
           dict(set_rows=np.arange(55, 65)), dict(set_rows=-np.arange(10)), dict(set_offset=[1, 4, 10]), dict(set_offset=[0, 6, 4]),
           dict(lb=plan["x0"], ub=plan["x0"]), dict(lb=[-np.inf, 20.0, -np.inf], ub=[np.inf, -20.0, np.inf]),
           dict(max_nfev=0), dict(ftol=-1.0), dict(xtol=np.nan),
           dict(slots=np.zeros(0, int), x0=[], lb=[], ub=[], x_scale=[]),
           dict(slots=np.arange(19), x0=np.zeros(19), lb=-np.ones(19), ub=np.ones(19), x_scale=np.ones(19))]
    with model.upload() as handle:
        cams24 = np.array([cam.vector24 for cam in model._dev_cams])
        first = handle.fit_sets(cams24, max_error=3.0, **good)
        for change in bad:
            with pytest.raises(_lib.GlhError) as err:
                handle.fit_sets(cams24, max_error=3.0, **{**good, **change})
            assert err.value.code != 0, change
        grid = cams24.copy()
        grid[0, 23] = 1.0
        with pytest.raises(_lib.GlhError):
            handle.fit_sets(grid, **good)
        with pytest.raises(ValueError):
            handle.fit_sets(cams24[:, :20], **good)
        again = handle.fit_sets(cams24, max_error=3.0, **good)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again)) and (first[1] > 0).all()
    model._handle = None
    with pytest.raises(_lib.GlhError, match="closed"):
        handle.fit_sets(cams24, **good)
    # a Lines control among the rows, or anywhere in a handle that is to be scored
    fitted, points = model.cams[0], model.controls[0]
    mixed = Cameras([fitted], [points, Lines(fitted, uvs=[points.uv[:5]], xyzs=[points.xyz[:5]])], cam_params=[{"viewdir": True}])
    with mixed.upload() as handle:
        with pytest.raises(_lib.GlhError, match="Lines"):
            handle.fit_sets(cams24, **{**good, "set_rows": np.arange(59, 69)})
        with pytest.raises(_lib.GlhError, match="Lines"):
            handle.fit_sets(cams24, max_error=3.0, **good)
        values, status, _ = handle.fit_sets(cams24, **good)  # (rows of the Points control alone: served)
        assert values.tobytes() == first[0].tobytes() and np.array_equal(status, first[1])
    mixed._handle = None
    # a RotationMatches control keeps camera coordinates where the others keep what they are compared with
    rotation, _ = rc.model("rotation_129")
    with rotation.upload() as handle:
        both = np.array([cam.vector24 for cam in rotation._dev_cams])
        with pytest.raises(_lib.GlhError, match="observed"):
            handle.fit_sets(both, **good)
        assert (handle.fit_sets(both, observed=rotation.observed(), **good)[1] > 0).all()
    rotation._handle = None


def test_no_job_and_no_set_leave_the_handle_as_a_fresh_one():
    """`Calib.eval` without a job and `fit_sets` without a set: empty outputs, and the calls that follow on that handle return
    the bytes they return on a fresh handle."""
    from glimpse_amd.camera import rotations
    from glimpse_amd.optimize import _batched_plan

    model, _ = rc.model("viewdir_64")
    plan = _batched_plan(model, {})
    fit = dict(fit_cam=0, slots=plan["slots"], x0=plan["x0"], lb=plan["lb"], ub=plan["ub"], x_scale=plan["x_scale"], max_error=3.0)
    sets, _, jobs = model._jacobian_plan()

    def served(handle, cams24):
        return [*model._evaluate(handle, sets, jobs), *handle.fit_sets(cams24, set_offset=[0, 4, 10], set_rows=np.arange(10), **fit)]

    with model.upload() as handle:
        cams24 = np.array([cam.vector24 for cam in model._dev_cams])
        fresh = served(handle, cams24)
    model._handle = None
    with model.upload() as handle:
        rot = rotations(cams24[:, 3:6])[0].reshape(1, len(cams24), 3, 3)
        assert handle.eval(cams24[None], rot, [], []).shape == (0, 2)
        x, status, mean_error, inlier = handle.fit_sets(cams24, set_offset=[0], set_rows=[], **fit)
        assert x.shape == (0, len(plan["slots"])) and status.shape == mean_error.shape == (0,) and inlier.shape == (0, model.size)
        again = served(handle, cams24)
    model._handle = None
    assert len(fresh) == len(again) == len(jobs) + 4 and all(a.tobytes() == b.tobytes() for a, b in zip(fresh, again))


def test_the_references_scenario():
    """The reference's one test of optimize (its tests/test_optimize.py) on a synthetic frame of 400 x 268: the frame
    projected into a camera turned by (2, 2, 2), SIFT on both, matched with max_ratio=0.8, and RANSAC over
    Cameras(viewdir) recovers the turn to 0.1 degrees on either path.  Texture seed 3 gives 2259 and 1867 keypoints and 1449 matches on an MI355X
    (printed below; at least 100 are asked for)."""
    import copy

    import glimpse_amd
    from glimpse_amd import optimize, synth

    frame = synth.make_texture(400, seed=3)[:268].astype(np.uint8)
    cam = glimpse_amd.Camera(imgsz=(400, 268), f=(480, 480))
    a = glimpse_amd.Image(cam=cam, array=frame, datetime=datetime.datetime(2020, 1, 1))
    b = copy.deepcopy(a)
    viewdir = (2, 2, 2)
    b.cam.viewdir = viewdir
    keypoints = [optimize.detect_keypoints(x, method=optimize.SIFT) for x in (a.read(), a.project(b.cam)[:, :, 0])]
    uvs = optimize.match_keypoints(*keypoints, max_ratio=0.8)
    print("keypoints", [len(k[0]) for k in keypoints], "matches", len(uvs[0]))
    assert len(uvs[0]) >= 100
    matches = optimize.Matches(cams=(a.cam, b.cam), uvs=uvs)
    model = optimize.Cameras(cams=[b.cam], controls=[matches], cam_params=[{"viewdir": True}])
    for batched in (False, True):
        np.random.seed(0)
        values, index = quiet(optimize.ransac, model, n=12, max_error=5, min_inliers=10, iterations=10, batched=batched)
        print("batched" if batched else "host", values, len(index), "inliers")
        assert (np.abs(values - viewdir) < 0.1).all()
