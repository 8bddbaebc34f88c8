"""`optimize.ransac_pairs`, `KeypointMatcher.ransac_matches` and `glh_calib_ransac_groups` on the GPU, on the designed scenes
of tests/ransac_pair_cases.py (admitted on the CPU by tests/test_ransac_pair_cases.py): the whole call against a loop of
`ransac(batched=True)` over the pairs, every hypothesis against `Cameras.fit` and `Cameras.errors` of the pair's model,
repeated and chunked calls byte for byte, a pair alone against the pair among others, the matcher method, and what is
refused."""
import contextlib
import datetime
import functools
import io

import numpy as np
import pytest

from tests import ransac_pair_cases as pc
from tests import test_ransac_pair_cases as admitted

pytestmark = pytest.mark.gpu
CRITERION = 1e-3  # |difference| / scales, the calibration's own criterion (tests/test_gpu_calib.py, test_gpu_ransac.py)
INFO = ("values", "status", "consensus", "refit_values", "refit_status", "mean_errors", "winner", "hyp_offset")
# the pairs of a long scene whose hypotheses are fitted on the host as well (every pair is compared with the loop)
FITTED_ON_THE_HOST = {"many_groups": range(0, 300, 20)}


def quiet(f, *args, **kwargs):
    """f(...) without the progress lines Cameras.fit writes."""
    with contextlib.redirect_stdout(io.StringIO()):
        return f(*args, **kwargs)


def run(name, **changes):
    """One call of ransac_pairs on fresh objects of scene `name`, under the scene's seed."""
    from glimpse_amd import optimize

    cams, matches, d = pc.scene(name)
    np.random.seed(pc.SCENES[name]["seed"])
    results, info = optimize.ransac_pairs(matches, return_info=True, **{**pc.call(name, d), **changes})
    return dict(cams=cams, matches=matches, data=d, results=results, info=info)


@functools.lru_cache(maxsize=None)
def device(name):
    return run(name)


def same_bytes(a, b):
    return all(a[key].tobytes() == b[key].tobytes() for key in INFO)


@pytest.mark.parametrize("name", list(pc.SCENES))
def test_the_call_equals_the_loop_over_the_pairs(name, monkeypatch):
    """Under one seed: for every pair the inliers of `ransac(model_k, batched=True)` exactly, None exactly where the loop
    raises, the values within 1e-3 of each parameter's scale (the largest ratio is printed; measured on an MI355X: at most
    3.1e-7, many_groups)."""
    from glimpse_amd import optimize

    got = device(name)
    cams, matches, d = pc.scene(name)
    call = pc.call(name, d)
    designed = call.pop("samples", None)
    loop = dict(n=call["n"], max_error=call["max_error"], min_inliers=call["min_inliers"], iterations=call["iterations"])
    drawn = optimize._ransac_samples
    np.random.seed(pc.SCENES[name]["seed"])
    worst, rejected = 0.0, 0
    for k, m in enumerate(matches.values()):
        model = pc.pair_model(m, name)
        if designed is not None:
            def samples(n, size, iterations, rows=designed[k]):
                if n >= size:
                    raise ValueError("Sample size is larger or equal to total size")
                yield from ([int(r) for r in s] for s in rows)

            monkeypatch.setattr(optimize, "_ransac_samples", samples)
        try:
            with np.errstate(invalid="ignore"):
                params, inliers = quiet(optimize.ransac, model, batched=True, **loop)
        except ValueError as err:
            assert "acceptance criteria" in str(err) or "Sample size" in str(err)
            assert got["results"][k] is None, (name, k)
            rejected += 1
            continue
        finally:
            monkeypatch.setattr(optimize, "_ransac_samples", drawn)
        assert got["results"][k] is not None, (name, k)
        assert np.array_equal(got["results"][k][1], inliers), (name, k)
        worst = max(worst, float((np.abs(got["results"][k][0] - params) / model.scales).max()))
    print(name, ": largest |difference| / scales =", worst, "; pairs", len(matches), "rejected", rejected, "times_ms",
          got["info"]["times_ms"])
    assert worst < CRITERION
    assert rejected == (2 if name == "rejects" else 0)


@pytest.mark.parametrize("name", list(pc.SCENES))
def test_every_hypothesis_against_the_pairs_model(name):
    """`values` against `Cameras.fit(sample)` of the pair's model within 1e-3 of the scales; `consensus` equal to
    `model.errors(values) < max_error` counted outside the sample; the designed failure's status negative; `winner` the
    admission's.  Measured on an MI355X (printed below): the largest ratio is 8.2e-4, on mixed_rows' samples of two rows,
    which determine the values least (tests/test_ransac_pair_cases.py: DETERMINED); 1.5e-4 and less elsewhere."""
    got = device(name)
    info, call = got["info"], pc.call(name, got["data"])
    samples = admitted.all_samples(name)
    worst = 0.0
    for k in FITTED_ON_THE_HOST.get(name, range(len(got["matches"]))):
        m = list(got["matches"].values())[k]
        first, last = info["hyp_offset"][k:k + 2]
        want = admitted.numpy_ransac(name, k)
        if samples[k] is None:
            assert first == last and info["winner"][k] == -1 and got["results"][k] is None
            continue
        assert last - first == len(samples[k])
        model = pc.pair_model(m, name)
        full = np.arange(m.size)
        for h, sample in enumerate(samples[k]):
            x, status = info["values"][first + h], info["status"][first + h]
            if want["hypotheses"][h]["values"] is None:
                assert status < 0 and info["consensus"][first + h] == 0 and info["refit_status"][first + h] == -100, (name, k, h)
                continue
            assert status > 0, (name, k, h, status)
            host = quiet(model.fit, [int(r) for r in sample])
            worst = max(worst, float((np.abs(x - host) / model.scales).max()))
            with np.errstate(invalid="ignore"):
                inside = model.errors(x) < call["max_error"]
            assert info["consensus"][first + h] == inside[np.delete(full, sample)].sum(), (name, k, h)
        assert info["winner"][k] == (-1 if want["winner"] is None else want["winner"]), (name, k)
    print(name, ": hypotheses against Cameras.fit: largest |difference| / scales =", worst)
    assert worst < CRITERION
    if name == "rejects":
        first = info["hyp_offset"][3]
        assert info["status"][first] < 0 and (info["status"][first + 1:info["hyp_offset"][4]] > 0).all()


def test_a_repeated_call_and_a_chunked_call_return_the_same_bytes():
    first, again = device("mixed_rows"), run("mixed_rows")
    assert same_bytes(first["info"], again["info"])
    # masks: 6 hypotheses x (13, 63, 65, 129, 257) rows = 78, 378, 390, 774 and 1542 bytes: 800 hold the first two together
    split = run("mixed_rows", budget=800)
    assert split["info"]["chunks"] >= 3 and first["info"]["chunks"] == 1
    assert same_bytes(first["info"], split["info"])
    for a, b in zip(first["results"], split["results"]):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    many, chunked = device("many_groups"), run("many_groups", budget=64 * 100)
    assert chunked["info"]["chunks"] >= 3 and same_bytes(many["info"], chunked["info"])


def test_a_pair_does_not_depend_on_the_others_and_no_camera_is_modified():
    from glimpse_amd import optimize

    got = device("mixed_rows")
    assert all(np.array_equal(cam._vector[:20], v[:20]) for cam, v in zip(got["cams"], got["data"]["start"]))
    cams, matches, d = pc.scene("mixed_rows")
    call = pc.call("mixed_rows", d)
    first, last = got["info"]["hyp_offset"][1:3]
    samples = admitted.all_samples("mixed_rows")
    alone, info = optimize.ransac_pairs({(1, 2): matches[1, 2]}, return_info=True, samples=[samples[1]], **call)
    for key in INFO[:6]:
        assert info[key].tobytes() == got["info"][key][first:last].tobytes(), key
    assert info["winner"][0] == got["info"]["winner"][1]
    assert alone[0][0].tobytes() == got["results"][1][0].tobytes() and np.array_equal(alone[0][1], got["results"][1][1])
    assert all(np.array_equal(cam._vector[:20], v[:20]) for cam, v in zip(cams, d["start"]))


def test_the_matcher_filters_every_pair_and_empties_the_rejected():
    """A matcher whose matches are those of mixed_rows, weights and rejects, as one sequence of images."""
    import glimpse_amd
    from glimpse_amd import optimize

    scenes = [pc.scene(name) for name in ("mixed_rows", "weights", "rejects")]
    call = pc.call("rejects", scenes[2][2])
    rejects = list(call.pop("samples"))
    images, keys, data, samples = [], [], [], []
    for cams, matches, _ in scenes:
        shift = len(images)
        images += [glimpse_amd.Image(cam=cam, array=np.zeros((2, 2), np.uint8), datetime=datetime.datetime(2020, 1, 1, 0, shift + k))
                   for k, cam in enumerate(cams)]
        keys += [(i + shift, j + shift) for i, j in matches]
        data += list(matches.values())
    some = np.array([[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [1, 5, 9, 12]])  # (rows of the shortest pair, 13)
    samples = [some] * (len(data) - len(rejects)) + rejects
    first = len(data) - len(rejects)  # the first pair of `rejects`, and its first image
    shift = len(images) - len(scenes[2][0])
    matcher = optimize.KeypointMatcher(images)
    matcher.matches = optimize.PairMatches(data, [i for i, _ in keys], [j for _, j in keys], (len(images), len(images)))
    sizes = [m.size for m in data]
    before = [(m.uvs[0].copy(), m.uvs[1].copy(), None if m.weights is None else np.array(m.weights)) for m in data]
    want = optimize.ransac_pairs(dict(zip(keys, _copies(data, before))), samples=samples, **call)
    counts = matcher.ransac_matches(samples=samples, **call)
    print("inliers per pair", list(counts), "of", sizes)
    assert list(counts) == [-1 if r is None else len(r[1]) for r in want]
    assert counts[first] == -1 and counts[first + 1] == -1 and (counts[first + 2:] > 20).all()
    for m, count, r, (uv0, uv1, w) in zip(data, counts, want, before):
        assert m.size == max(count, 0) == len(m.uvs[1])
        keep = np.zeros(len(uv0), dtype=bool) if r is None else np.isin(np.arange(len(uv0)), r[1])
        assert np.array_equal(m.uvs[0], uv0[keep]) and np.array_equal(m.uvs[1], uv1[keep], equal_nan=True)
        assert (m.weights is None) == (w is None) and (w is None or np.array_equal(m.weights, w[keep]))
    assert any(m.weights is not None for m in data)
    per_image = matcher.matches_per_image()
    assert per_image.sum() == 2 * counts[counts > 0].sum() and per_image.sum() < 2 * sum(sizes)
    assert per_image[shift] == 0  # (the first image of `rejects` has the short pair alone)
    assert matcher.images_per_image()[shift] == 0 and len(matcher.matches.data) == len(data)


def _copies(data, before):
    from glimpse_amd import optimize

    return [optimize.Matches(cams=m.cams, uvs=[uv0, uv1], weights=w) for m, (uv0, uv1, w) in zip(data, before)]


def test_what_is_refused_is_refused_before_the_library(monkeypatch):
    import glimpse_amd
    from glimpse_amd import _lib, optimize

    cams, matches, d = pc.scene("kinds_px")
    call = pc.call("kinds_px", d)
    plain, rotation = matches[0, 1], matches[1, 2]

    class GridCamera(glimpse_amd.Camera):
        """A camera whose 24-vector says it is a georeferenced raster image (entry 23), as `Grid.vector24` does."""

        @property
        def vector24(self):
            v = super().vector24
            v[23] = 1.0
            return v

    grid = GridCamera(xyz=cams[0].xyz, viewdir=cams[0].viewdir, imgsz=cams[0].imgsz, f=cams[0].f)
    xyz = optimize.RotationMatchesXYZ(cams=rotation.cams, uvs=rotation.uvs, xys=rotation.xys)
    points = optimize.Points(cams[0], uv=plain.uvs[0][:5], xyz=np.ones((5, 3)))
    refused = [
        ({(0, 1): plain}, {"cam_params": {"xyz": True}}, "position"),
        ({(1, 2): rotation}, {"cam_params": {"viewdir": True, "f": True}}, "internal parameters"),
        ({(0, 1): optimize.Matches(cams=[grid, cams[1]], uvs=plain.uvs)}, {}, "raster grid"),
        ({(0, 1): plain}, {"loss": "soft_l1"}, "loss"),
        ({(0, 1): plain}, {"nan_policy": "raise"}, "nan_policy"),
        ({(0, 1): plain}, {"max_nfev": None}, "max_nfev"),
        ({(0, 1): plain, (1, 2): xyz}, {}, "RotationMatchesXYZ"),
        ({(0, 1): plain, (1, 2): points}, {}, "Points"),
        ({(0, 1): plain}, {"cam_params": {}}, "without a parameter"),
    ]
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was called"))
    for pairs, change, word in refused:
        with pytest.raises(NotImplementedError, match=word):
            optimize.ransac_pairs(pairs, **{**call, **change})
    with pytest.raises(ValueError, match="x0"):  # (a view direction outside the bounds given for it)
        optimize.ransac_pairs({(0, 1): plain}, **{**call, "cam_params": {"viewdir": (True, 100.0, 200.0)}})
    with pytest.raises(ValueError, match="strictly less"):
        optimize.ransac_pairs({(0, 1): plain}, **{**call, "cam_params": {"viewdir": (True, 20.0, -20.0)}})
    assert optimize.ransac_pairs({}, **call) == [] and optimize.ransac_pairs([], **call) == []
    assert optimize.ransac_pairs(np.full((3, 3), None, dtype=object), **call) == []


def test_fit_sets_and_ransac_groups_fit_a_sample_to_the_same_bytes():
    """Both entry points run one fit (glh_calib.hip: team_fit), so the same samples of the same rows give the same `values`
    and `status`, byte for byte: through `fit_sets` as sets (always a team of two waves) and through `ransac_groups` as the
    hypotheses of one group that accepts nothing (`min_inliers` above the row count; a team of one wave up to 64 rows,
    whose sums equal the two-wave team's because the idle wave adds +0.0 to each).  One handle with the pair of
    `six_parameters` (257 rows); samples of 2 .. 200 rows either side of a wave and of the tile of 128, four each; the
    view direction (p = 3, the small instantiation) and the scene's five parameters (the general one), whose sizes start
    at the scene's own 40: two rows are four residuals for five parameters, which the admission's rule (every sample
    determines its values) excludes."""
    from glimpse_amd import _lib
    from glimpse_amd.optimize import _pairs_plan, match_pairs

    cams, matches, d = pc.scene("six_parameters")
    (m,) = matches.values()
    rows = m.size
    assert rows == 257
    cams24 = np.array([cam.vector24 for cam in cams])
    src = np.column_stack((m.uvs[1], np.zeros(rows)))
    different = []
    with _lib.Calib(2, [_lib.CALIB_KINDS["matches"]], [0], [1], [0], [0, rows], m.uvs[0], src) as handle:
        for params, sizes in ((pc.VIEWDIR, (2, 63, 64, 65, 128, 129, 200)), (pc.GENERAL, (40, 63, 64, 65, 128, 129, 200))):
            plan = _pairs_plan(match_pairs(matches), 1, params, {})
            x0, lb, ub, scale = (np.array(v) for v in plan["values"][0])
            for n in sizes:
                rng = np.random.default_rng(n)
                samples = np.array([rng.permutation(rows)[:n] for _ in range(4)], dtype=np.int64)
                values, status, _ = handle.fit_sets(cams24, 1, plan["slots"], x0, lb, ub, scale, np.arange(5) * n,
                                                    samples.reshape(-1))
                groups = handle.ransac_groups(cams24, [0], [1], plan["slots"], x0[None], lb[None], ub[None], scale[None],
                                              [0, 4], samples, max_error=3.0, min_inliers=rows + 1)
                print("p", len(plan["slots"]), "n", n, "status", status, groups["status"])
                assert (status > 0).all() and (groups["refit_status"] == _lib.CALIB_NOT_REFITTED).all()
                if values.tobytes() != groups["values"].tobytes() or status.tobytes() != groups["status"].tobytes():
                    different.append((len(plan["slots"]), n, float(np.abs(values - groups["values"]).max())))
    assert not different, different


def test_bad_arguments_leave_the_handle_usable():
    from glimpse_amd import _lib
    from glimpse_amd.optimize import _pairs_plan, match_pairs

    cams, matches, d = pc.scene("fitted_first")
    plan = _pairs_plan(match_pairs(matches), 0, pc.VIEWDIR, {})
    x0, lb, ub, scale = (np.array([v[q] for v in plan["values"]]) for q in range(4))
    ms = list(matches.values())
    obs = np.concatenate([m.uvs[0] for m in ms])
    src = np.concatenate([np.column_stack((m.uvs[1], np.zeros(m.size))) for m in ms])
    K = _lib.CALIB_KINDS
    samples = np.array([[0, 5], [7, 40], [64, 70], [100, 127]])
    good = dict(group_control=[0, 1], group_cam=[0, 1], slots=plan["slots"], x0=x0, lb=lb, ub=ub, x_scale=scale,
                hyp_offset=[0, 2, 4], samples=samples, max_error=3.0, min_inliers=20)
    bad = [dict(group_control=[0, 2]), dict(group_control=[-1, 1]), dict(group_control=[1, 0]), dict(group_control=[0, 0]),
           dict(group_cam=[0, 3]), dict(group_cam=[2, 1]), dict(group_cam=[0, 0]),
           dict(samples=np.array([[0, 64], [7, 40], [64, 70], [100, 127]])), dict(samples=samples[:, ::-1][::-1].copy()),
           dict(samples=-samples), dict(samples=samples[:, :0]),
           dict(slots=[3, 4, 6]), dict(slots=[3, 3, 5]), dict(slots=[3, 4, 20]),
           dict(x0=x0 + [0, 400, 0], ub=np.array([[np.inf, 100, np.inf]] * 2)), dict(lb=x0, ub=x0),
           dict(lb=np.array([[-np.inf, 20.0, -np.inf]] * 2), ub=np.array([[np.inf, -20.0, np.inf]] * 2)),
           dict(x_scale=np.array([[1, 0, 1]] * 2)), dict(x_scale=np.array([[1, np.nan, 1]] * 2)),
           dict(hyp_offset=[1, 2, 4]), dict(hyp_offset=[0, 3, 2]), dict(max_nfev=0), dict(ftol=-1.0), dict(xtol=np.nan),
           dict(max_error=np.nan),
           dict(group_control=[0], group_cam=[0], x0=x0[:1], lb=lb[:1], ub=ub[:1], x_scale=scale[:1], hyp_offset=[0, 2]),
           dict(slots=np.arange(19), **{k: np.ones((2, 19)) * s for k, s in (("x0", 0), ("lb", -1), ("ub", 1), ("x_scale", 1))})]
    cams24 = np.array([cam.vector24 for cam in cams])
    with _lib.Calib(3, [K["matches"]] * 2, [0, 1], [1, 2], [0, 0], [0, 64, 128], obs, src) as handle:
        first = handle.ransac_groups(cams24, **good)
        for change in bad:
            with pytest.raises(_lib.GlhError) as err:
                handle.ransac_groups(cams24, **{**good, **change})
            assert err.value.code != 0 and "ransac groups" in str(err.value), change
        grid = cams24.copy()
        grid[2, 23] = 1.0
        with pytest.raises(_lib.GlhError, match="raster grid"):
            handle.ransac_groups(grid, **good)
        with pytest.raises(ValueError):
            handle.ransac_groups(cams24[:, :20], **good)
        again = handle.ransac_groups(cams24, **good)
        assert all(first[key].tobytes() == again[key].tobytes() for key in first) and (first["status"] > 0).all()
        # weights of one multiply every residual by 1.0: the same bytes through the weighted path
        unit = handle.ransac_groups(cams24, weights=np.ones((128, 2)), **good)
        assert all(first[key].tobytes() == unit[key].tobytes() for key in first)
    # a POINTS control among the groups; a ROTATION control without `observed`
    with _lib.Calib(3, [K["matches"], K["points"]], [0, 1], [1, 1], [0, 0], [0, 64, 128], obs, src) as handle:
        with pytest.raises(_lib.GlhError, match="POINTS or LINES"):
            handle.ransac_groups(cams24, **good)
    with _lib.Calib(3, [K["matches"], K["rotation"]], [0, 1], [1, 2], [0, 0], [0, 64, 128], obs, src) as handle:
        with pytest.raises(_lib.GlhError, match="observed"):
            handle.ransac_groups(cams24, **good)
        assert (handle.ransac_groups(cams24, observed=obs, **good)["status"] > 0).any()
    with pytest.raises(_lib.GlhError, match="closed"):
        handle.ransac_groups(cams24, **good)
    assert list(_lib.ransac_chunks([13, 63, 65, 129, 257], [6] * 5, 800)) == [0, 0, 1, 2, 3]
