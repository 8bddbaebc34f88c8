"""Admission of the designed scenes of `optimize.ransac_pairs` (tests/ransac_pair_cases.py) on the CPU, by the method of
tests/test_ransac_cases.py: every pair of every scene is run through RANSAC in NumPy -- the residuals by oracle/camera.py,
the fits by scipy.optimize.least_squares with the bounds and scales of the pair's `Cameras` model -- and must keep every
decision the GPU test compares well away from its threshold.  These are conditions on the inputs, met by the NumPy
reference alone: nothing here projects through the package's kernels."""
import functools

import numpy as np
import pytest

from oracle import camera as oc
from tests import ransac_pair_cases as pc
from tests.test_ransac_cases import COUNT_GAP, ERROR_GAP, MEAN_GAP, predicted

# sigma_min of a hypothesis's Jacobian in scaled variables over |r| at its minimum: how well the sample determines the values.
# The criterion the GPU test holds the values to (1e-3 of a scale, between two fits that stop at ftol = 1e-8) presupposes
# a minimum that is determined; the yardstick is the least determined of the scenes whose parameters the brief fixes
# (samples of two rows for a view direction: 0.0108), rounded down.
DETERMINED = 0.01
# The pairs of a long scene that the NumPy RANSAC is run over here.  (All 300 pairs of many_groups pass with this entry
# removed; that takes half a minute of SciPy fits, so every run admits each twentieth.)
SUBSET = {"many_groups": range(0, 300, 20)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return pc.scene(name)


def pairs_checked(name):
    return list(SUBSET.get(name, range(len(pc.SCENES[name]["pairs"]))))


def samples_of(name):
    """Per pair the samples the call draws under the scene's seed (or the designed ones), None for a pair too short."""
    from glimpse_amd.optimize import _ransac_samples

    call = pc.call(name, scene(name)[2])
    if "samples" in call:
        return [s if len(s) else None for s in call["samples"]]
    np.random.seed(pc.SCENES[name]["seed"])
    out = []
    for _, _, _, rows, _ in pc.SCENES[name]["pairs"]:
        out.append(np.array(list(_ransac_samples(n=call["n"], size=rows, iterations=call["iterations"]))) if rows > call["n"] else None)
    return out


@functools.lru_cache(maxsize=None)
def all_samples(name):
    return samples_of(name)


def pair_predicted(pair, v, held, fitted):
    """`predicted` of the pair's arrays with the fitted camera at `v` and the other at `held` (every camera stands at the
    origin, so a ray is a point)."""
    if pair["kind"] != "rotation_xy":
        return predicted(dict(other=held, side=0 if fitted == 0 else 1), v, pair)
    first, second = (v, held) if fitted == 0 else (held, v)
    R = oc.rotation_matrix(second[3:6])
    return oc.xyz_to_xy(first, pair["xy1"] @ R[0:2] + R[2])


@functools.lru_cache(maxsize=None)
def numpy_ransac(name, k):
    """RANSAC over pair `k` of scene `name` as optimize.ransac runs it, in NumPy: per hypothesis the fitted values (None
    where the fit failed), the errors of all rows and the consensus count; per accepted hypothesis the refit's mean error;
    the winner (a hypothesis, None if there is none) and the final errors."""
    import scipy.optimize

    _, matches, d = scene(name)
    call = pc.call(name, d)
    pair = d["pairs"][k]
    m = matches[pair["i"], pair["j"]]
    samples = all_samples(name)[k]
    if samples is None:
        return dict(samples=None, hypotheses=[], winner=None, final=None, call=call)
    fitted = call["fitted"]
    model = pc.pair_model(m, name)
    slots = np.flatnonzero(model.cam_masks[0])
    x0, lb, ub = model._values_bounds()
    start, held = d["start"][(pair["i"], pair["j"])[fitted]], d["start"][(pair["i"], pair["j"])[1 - fitted]]
    observed = pair["xy0"] if pair["kind"] == "rotation_xy" else pair["uv0"]

    def errors(x, rows=slice(None)):
        v = start.copy()
        v[slots] = x
        with np.errstate(invalid="ignore"):
            return np.linalg.norm((pair_predicted(pair, v, held, fitted) - observed)[rows], axis=1)

    def fit(rows):
        def fun(x):
            v = start.copy()
            v[slots] = x
            with np.errstate(invalid="ignore"):
                r = (pair_predicted(pair, v, held, fitted) - observed)[rows].ravel()
            return r[~np.isnan(r)]

        if len(fun(x0)) < len(x0):
            return None
        result = scipy.optimize.least_squares(fun, x0, bounds=(lb, ub), x_scale=model.scales)
        return result.x if result.success else None

    def determined(x, rows):
        """sigma_min of the Jacobian in scaled variables over |r|, both at x (see test_admission)."""
        def r(y):
            v = start.copy()
            v[slots] = y
            with np.errstate(invalid="ignore"):
                out = (pair_predicted(pair, v, held, fitted) - observed)[rows].ravel()
            return out[~np.isnan(out)]

        r0 = r(x)
        J = np.column_stack([(r(x + 1e-6 * model.scales[i] * np.eye(len(x))[i]) - r0) / 1e-6 for i in range(len(x))])
        return float(np.linalg.svd(J, compute_uv=False)[-1] / max(np.linalg.norm(r0), 1e-300))

    full = np.arange(len(observed))
    hypotheses = []
    for sample in samples:
        x = fit(sample)
        if x is None:
            hypotheses.append(dict(values=None, errors=None, count=0, mean=np.nan, rows=None))
            continue
        e = errors(x)
        test = np.delete(full, sample)
        with np.errstate(invalid="ignore"):
            also = test[e[test] < call["max_error"]]
        h = dict(values=x, errors=e, count=len(also), mean=np.nan, rows=None, determined=determined(x, sample))
        if len(also) > call["min_inliers"]:
            h["rows"] = np.sort(np.concatenate((sample, also)))
            better = fit(h["rows"])
            if better is not None:
                h["refit"] = better
                h["mean"] = float(np.mean(errors(better, h["rows"])))
        hypotheses.append(h)
    means = np.array([h["mean"] for h in hypotheses])
    winner = int(np.nanargmin(means)) if np.isfinite(means).any() else None
    final = errors(hypotheses[winner]["refit"]) if winner is not None else None
    return dict(samples=samples, hypotheses=hypotheses, winner=winner, final=final, call=call)


def unit(name):
    """The unit of the scene's errors in pixels: 1, or 1 / f for camera coordinates."""
    return pc.SCENES[name].get("max_error", pc.rc.MAX_ERROR) / pc.rc.MAX_ERROR


@pytest.mark.parametrize("name", list(pc.SCENES))
def test_admission(name):
    """Pair by pair: no row's error within ERROR_GAP (px, or px / f) of max_error under any hypothesis that fitted or under
    the winner; no consensus count within COUNT_GAP of min_inliers; the best and the second-best distinct set more than
    MEAN_GAP apart in mean error; every sample determines its values (DETERMINED)."""
    for k in pairs_checked(name):
        got = numpy_ransac(name, k)
        call = got["call"]
        fitted = [h for h in got["hypotheses"] if h["errors"] is not None]
        if not fitted:
            continue
        gap = min(np.nanmin(np.abs(h["errors"] - call["max_error"])) for h in fitted)
        counts = np.array([h["count"] for h in fitted])
        sets = {}
        for h in got["hypotheses"]:
            if h["rows"] is not None and not np.isnan(h["mean"]):
                sets.setdefault(h["rows"].tobytes(), h["mean"])
        means = sorted(sets.values())
        final = np.inf if got["final"] is None else np.nanmin(np.abs(got["final"] - call["max_error"]))
        print(name, k, ": smallest |error - max_error|", gap, "final", final, "; consensus", sorted(set(counts.tolist())), "against",
              call["min_inliers"], "; distinct sets", len(means), "means", means[:3])
        assert gap > ERROR_GAP * unit(name) and final > ERROR_GAP * unit(name), (name, k)
        assert (np.abs(counts - call["min_inliers"]) > COUNT_GAP).all(), (name, k)
        assert len(means) < 2 or means[1] - means[0] > MEAN_GAP * means[0], (name, k)
        assert min(h["determined"] for h in fitted) > DETERMINED, (name, k, [h["determined"] for h in fitted])


def test_what_each_scene_is_for():
    rows = {name: [p[3] for p in s["pairs"]] for name, s in pc.SCENES.items()}
    assert rows["mixed_rows"] == [13, 63, 65, 129, 257] and pc.SCENES["mixed_rows"]["n"] == 2
    # camera 1 is fitted in pair (0, 1) and held in pair (1, 2)
    cams, matches, _ = scene("mixed_rows")
    assert matches[0, 1].cams[1] is cams[1] and matches[1, 2].cams[0] is cams[1]
    assert all(len(s) == 6 for s in all_samples("mixed_rows"))
    assert all(numpy_ransac("mixed_rows", k)["winner"] is not None for k in range(5))
    kinds = [type(m).__name__ for name in ("kinds_px", "kinds_xy") for m in scene(name)[1].values()]
    assert kinds == ["Matches", "RotationMatches", "RotationMatchesXY"] and rows["kinds_px"] + rows["kinds_xy"] == [129] * 3
    assert pc.SCENES["fitted_first"]["fitted"] == 0 and rows["fitted_first"] == [64, 64]
    assert len(pc.SCENES["many_groups"]["pairs"]) == 300 and set(rows["many_groups"]) == {16}
    assert all(len(s) == 4 for s in all_samples("many_groups"))
    assert all(m.weights is not None for m in scene("weights")[1].values()) and rows["weights"] == [65, 65]
    model = pc.pair_model(next(iter(scene("six_parameters")[1].values())), "six_parameters")
    assert int(model.cam_masks[0].sum()) == 5 and pc.SCENES["six_parameters"]["n"] == 40
    assert numpy_ransac("six_parameters", 0)["winner"] is not None
    # rejects: too few rows; nothing accepted; one hypothesis; a hypothesis that cannot be fitted beside ones that can
    got = [numpy_ransac("rejects", k) for k in range(4)]
    assert got[0]["samples"] is None and rows["rejects"][0] == pc.SCENES["rejects"]["n"]
    assert got[1]["winner"] is None and len(got[1]["hypotheses"]) == 6
    assert len(got[2]["hypotheses"]) == 1 and got[2]["winner"] == 0
    assert got[3]["hypotheses"][0]["values"] is None and got[3]["winner"] is not None
    assert sum(h["values"] is not None for h in got[3]["hypotheses"]) == 5


def test_the_plan_is_the_models():
    """What `ransac_pairs` hands the device per pair (`_pairs_plan`) is what `_batched_plan` makes of the pair's model."""
    from glimpse_amd.optimize import _batched_plan, _pairs_plan, match_pairs

    for name in ("mixed_rows", "kinds_px", "kinds_xy", "fitted_first", "six_parameters"):
        _, matches, d = scene(name)
        call = pc.call(name, d)
        plan = _pairs_plan(match_pairs(matches), call["fitted"], call["cam_params"], {"ftol": 1e-9})
        assert plan["options"] == {"ftol": 1e-9}
        for m, values in zip(matches.values(), plan["values"]):
            want = _batched_plan(pc.pair_model(m, name), {})
            assert np.array_equal(plan["slots"], want["slots"])
            for got, key in zip(values, ("x0", "lb", "ub", "x_scale")):
                assert np.array_equal(got, want[key]), (name, key)
