"""glimpse_amd.optimize on the device: glh_orient_eval against its restatement (tests/orient_restated.py) bit for bit, the
match classes against the reference's outputs, ObserverCameras.fit against the restatement-driven fit and against the
reference's own fit, and the handle's hygiene."""
import contextlib
import io

import numpy as np
import pytest

from tests import orient_cases as oc
from tests import orient_restated as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    _lib.load()
    return _lib


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.mark.parametrize("fixture", oc.FIXTURES)
def test_eval_equals_the_restatement_bit_for_bit(golden, lib, fixture):
    """The objective and every gradient entry, with anchor_weight 0 and 1e6, at the start and at the three probe points;
    and a second evaluation on the same handle gives the same bytes."""
    from glimpse_amd.camera import rotations

    g = golden(fixture)
    model, _ = oc.observer_of(g)
    pairs = oc.pairs_of(g)
    with model.upload() as handle:
        for point in (g["viewdirs_start"], *g["points"]):
            R, Rprime = rotations(point)
            d = {}
            want = rs.evaluate(len(point), pairs, R, Rprime, d)
            assert d["min_abs_dxyz"] > 1e-9  # (the condition on the fixture's noise)
            got = handle.eval(R, Rprime)
            again = handle.eval(R, Rprime)
            assert _bits(got[0]) == _bits(want[0]) == _bits(again[0])
            assert np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(_bits(got[1]), _bits(again[1]))
            for weight in (0.0, 1e6):
                objective, gradient = model.evaluate(handle, point, anchor_weight=weight)
                want = rs.callback(point, g["viewdirs_start"], g["anchors"], weight, pairs, rotations)
                assert _bits(objective) == _bits(want[0])
                assert np.array_equal(_bits(gradient), _bits(want[1]))
        _, _, times = handle.eval(R, Rprime, return_times=True)
        assert set(times) == {"upload", "map", "reduce", "download"} and all(t >= 0 for t in times.values())
    if fixture == "orient_chunks.npz":
        assert not got[1][5].any()  # the image in no pair


def _differing(a, b):
    return int(np.count_nonzero(_bits(a) != _bits(b)))


@pytest.mark.parametrize("n_images", oc.SYNTHETIC)
def test_sequences_past_one_workgroup_equal_the_restatement_and_the_longdouble_sums(lib, n_images):
    """`orient_cases.synthetic` (256, 257, 300 and 600 images: 1, 2, 2 and 3 image workgroups of k_orient_reduce, 803 to
    1487 pairs: 4 to 6 turns of the objective's lanes, pairs of one to three chunks in a lane's first and second turn, a
    hub image with 300 pairs in its incidence list, images in no pair either side of image 256;
    tests/test_optimize_host.py asserts all of it) through `_lib.Orient`: the restatement bit for bit, the same bytes
    twice, and inside the derived bound of plain longdouble sums, which share nothing of the kernel's structure.

    Ratio of the error to u sum |addend| on an MI355X, as on the CPU (the restatement is equal bit for bit): objective
    0.26, 0.13, 1.2, 0.39 and gradient 2.2, 2.8, 14, 4.1 for 256, 257, 300 and 600 images (the largest is the hub image's,
    which 22 684 addends feed); the bound's factor n_adds is 58 064 or more for the objective, and no entry uses more than
    0.15 % of its bound."""
    case = oc.synthetic_case(n_images)
    want, details = case["want"], case["details"]
    assert details["min_abs_dxyz"] > 1e-9
    with lib.Orient(n_images, *oc.flat(case["pairs"])) as handle:
        got = handle.eval(case["R"], case["Rprime"])
        again = handle.eval(case["R"], case["Rprime"])
    bound_o, bound_g = oc.longdouble_bounds(details, case["exact"][2])
    (err_o, ratio_o), (err_g, ratio_g) = oc.longdouble_ratios(got, case["exact"], details)
    print(n_images, "images,", len(case["pairs"]), "pairs: differing from the restatement: objective", _differing(got[0], want[0]),
          "gradient entries", _differing(got[1], want[1]), "of", got[1].size, "; second call:", _differing(got[0], again[0]),
          _differing(got[1], again[1]), "; against longdouble, ratio to u sum |addend|: objective", ratio_o, "of",
          bound_o / (oc.U * details["abs_objective"]), "gradient", ratio_g, "; largest share of its bound",
          float((err_g[bound_g > 0] / bound_g[bound_g > 0]).max()))
    assert _bits(got[0]) == _bits(want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert _bits(again[0]) == _bits(got[0]) and np.array_equal(_bits(again[1]), _bits(got[1]))
    isolated = oc.synthetic_isolated(n_images)
    assert not _bits(got[1][isolated]).any()  # the images in no pair: exactly +0
    assert err_o <= bound_o and (err_g <= bound_g).all()


def test_a_handle_made_after_a_larger_one_was_destroyed(lib):
    """600 images evaluated and destroyed, then 257: what the allocator hands back holds the larger sequence's lists,
    partial sums and gradient.  Image 256 of the 257, the only one of the second workgroup, is in no pair: a kernel that
    never wrote its row would pass on fresh memory that happens to be zero, and fails here."""
    big, small = oc.synthetic_case(600), oc.synthetic_case(257)
    with lib.Orient(600, *oc.flat(big["pairs"])) as handle:
        handle.eval(big["R"], big["Rprime"])
    with lib.Orient(257, *oc.flat(small["pairs"])) as handle:
        got = handle.eval(small["R"], small["Rprime"])
    print("differing from the restatement: objective", _differing(got[0], small["want"][0]), "gradient entries",
          _differing(got[1], small["want"][1]), "of", got[1].size)
    assert _bits(got[0]) == _bits(small["want"][0]) and np.array_equal(_bits(got[1]), _bits(small["want"][1]))


def test_observer_cameras_of_257_images_through_the_public_surface(lib):
    """ObserverCameras built from a dict of 803 matches between 257 images: `evaluate` with anchor_weight 0 and 1e6 at the
    start and half a degree off it, against the restatement's callback bit for bit."""
    from glimpse_amd.camera import rotations

    model, pairs = oc.synthetic_observer(257)
    start = oc.synthetic_case(257)["viewdirs"]
    assert np.array_equal(model.viewdirs, start) and len(model.matches) == len(pairs) == 803
    with model.upload() as handle:
        for point in (start, oc.synthetic_probe(start)):
            for weight in (0.0, 1e6):
                d = {}
                want = rs.callback(point, start, model.anchors, weight, pairs, rotations, d)
                assert d["min_abs_dxyz"] > 1e-9
                objective, gradient = model.evaluate(handle, point, anchor_weight=weight)
                print("anchor_weight", weight, "anchors' objective", d["anchor_objective"], ": differing objective",
                      _differing(objective, want[0]), "gradient entries", _differing(gradient, want[1]), "of", gradient.size)
                assert _bits(objective) == _bits(want[0]) and np.array_equal(_bits(gradient), _bits(want[1]))
                assert gradient.shape == (257, 3) and (weight == 0.0 or point is start or d["anchor_objective"] > 0)


def test_match_classes_against_the_reference(golden):
    """`predicted` of the four classes on pair (1, 2) of the fixture, both cameras, and the camera coordinates the classes
    make, against the reference's.  Tolerances are those of the existing camera tests: rtol 1e-11, atol 1e-12 for what
    `uv_to_xyz` yields (tests/test_gpu_api.py: camera coordinates and rays), and for image coordinates, which pass through
    `xyz_to_uv` as well, its atol 1e-9 (tests/test_gpu_parity.py) with the looser rtol of the two."""
    import glimpse_amd
    from glimpse_amd import optimize

    g = golden("orient_sequence.npz")
    cams = [glimpse_amd.Camera(viewdir=v, **oc.internals(g)) for v in g["viewdirs_start"]]
    off = g["offsets"]
    for p, (i, j) in enumerate(zip(g["pair_i"], g["pair_j"])):
        uvs = [g["uv_i"][off[p]:off[p + 1]], g["uv_j"][off[p]:off[p + 1]]]
        m = optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], uvs=uvs)
        np.testing.assert_allclose(m.xys[0], g["xy_i"][off[p]:off[p + 1]], rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(m.xys[1], g["xy_j"][off[p]:off[p + 1]], rtol=1e-11, atol=1e-12)
    p = 2
    pair = [cams[g["pair_i"][p]], cams[g["pair_j"][p]]]
    uvs = [g["uv_i"][off[p]:off[p + 1]], g["uv_j"][off[p]:off[p + 1]]]
    plain = optimize.Matches(cams=pair, uvs=uvs)
    for name, mtype, tol in (("matches", optimize.Matches, dict(rtol=1e-11, atol=1e-9)),
                             ("rotation", optimize.RotationMatches, dict(rtol=1e-11, atol=1e-9)),
                             ("xy", optimize.RotationMatchesXY, dict(rtol=1e-11, atol=1e-12)),
                             ("xyz", optimize.RotationMatchesXYZ, dict(rtol=1e-11, atol=1e-12))):
        m = plain.to_type(mtype)  # (Matches -> the rotation classes: camera coordinates made on the device)
        assert type(m) is mtype and m.size == 64
        for c in (0, 1):
            np.testing.assert_allclose(m.predicted(cam=c), g[f"predicted_{name}_{c}"], **tol)
            np.testing.assert_allclose(m.predicted(cam=pair[c], index=slice(3, 9)), g[f"predicted_{name}_{c}"][3:9], **tol)
    back = plain.to_type(optimize.RotationMatches).to_type(optimize.Matches)
    assert type(back) is optimize.Matches and np.array_equal(back.uvs[0], uvs[0])
    # xys only -> image coordinates on the host -> the reference's uv within the round trip's tolerance
    made = optimize.RotationMatchesXYZ(cams=pair, xys=[g["xy_i"][off[p]:off[p + 1]], g["xy_j"][off[p]:off[p + 1]]])
    np.testing.assert_allclose(made.to_type(optimize.Matches).uvs[1], uvs[1], rtol=1e-11, atol=1e-9)


def test_filter_selects_the_reference_indices(golden):
    import glimpse_amd
    from glimpse_amd import optimize

    g = golden("orient_sequence.npz")
    cams = [glimpse_amd.Camera(viewdir=v, **oc.internals(g)) for v in g["viewdirs_start"]]
    off, p = g["offsets"], 5
    uvs = [g["uv_i"][off[p]:off[p + 1]], g["uv_j"][off[p]:off[p + 1]]]
    for name in ("error", "distance", "both", "scaled"):
        max_error, max_distance, cam, scaled, min_weight = g[f"filter_{name}_args"]
        m = optimize.Matches(cams=[cams[2], cams[4]], uvs=[uv.copy() for uv in uvs], weights=g["filter_weights"].copy())
        m.filter(max_error=max_error or None, max_distance=max_distance or None, cam=int(cam), scaled=bool(scaled),
                 min_weight=min_weight or None)
        keep = g[f"filter_{name}"]
        assert 0 < len(keep) < len(uvs[0])
        assert np.array_equal(m.uvs[0], uvs[0][keep]) and np.array_equal(m.uvs[1], uvs[1][keep])
        assert np.array_equal(m.weights, g["filter_weights"][keep])


def _fit(model, **kwargs):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        result = model.fit(**kwargs)
    return result, out.getvalue()


@pytest.fixture(scope="module")
def fits(golden, lib):
    """{name: (the device's fit, what it printed, the restatement-driven fit)} for maxiter = 5 and run to convergence."""
    from glimpse_amd.camera import rotations

    g = golden("orient_sequence.npz")
    model, cams = oc.observer_of(g)
    out = {}
    for name, options in (("maxiter5", {"maxiter": 5}), ("converged", {})):
        result, printed = _fit(model, options=options)
        assert all(np.array_equal(cam.viewdir, v) for cam, v in zip(cams, g["viewdirs_start"]))  # the cameras are back
        want = rs.fit(g["viewdirs_start"], g["viewdirs_start"], g["anchors"], 1e6, oc.pairs_of(g), rotations, options=options)
        out[name] = (result, printed, want)
    return out


@pytest.mark.parametrize("name", ["maxiter5", "converged"])
def test_fit_equals_the_restatement_driven_fit(fits, name):
    """The same SciPy with callback values that are equal in every bit takes the same path: x, fun, nit and nfev are
    equal, x and fun bit for bit.  The progress line and, on failure, the message are printed as the reference prints."""
    result, printed, want = fits[name]
    assert result.nit == want.nit and result.nfev == want.nfev and result.success == want.success
    assert np.array_equal(_bits(result.x), _bits(want.x))
    assert _bits(result.fun) == _bits(want.fun)
    assert result.x.shape == (15,)
    assert printed.count("\r") == result.nfev and printed.startswith("\r")
    assert ("\r" + str(result.fun)) in printed
    if not result.success:
        assert printed.endswith("\n" + str(result.message) + "\n")


@pytest.mark.parametrize("name", ["maxiter5", "converged"])
def test_fit_against_the_reference_fit(golden, fits, name):
    """The fit against the reference's own, recorded by tools/make_golden_orient.py.  The restatement-driven fit (which the
    device's equals bit for bit, above) was measured against it on the CPU of the build machine:

        maxiter = 5:  max |dx| = 1.07e-13 deg, |dfun| = 1.44e-12;   converged:  max |dx| = 6.72e-5 deg, |dfun| = 2.35e-7

    (nit 5 / 5 and 27 / 27, nfev 11 / 11 and 105 / 100).  The difference is the summation order's ulps passing through
    BFGS's line search; the test allows ten times the measured values, which covers another path through the same
    rounding and hides no error of the callback (that is pinned bit for bit).  The converged fits differ by less than
    1e-4 deg, so their x is compared too."""
    measured = {"maxiter5": (1.07e-13, 1.44e-12), "converged": (6.72e-5, 2.35e-7)}[name]
    g = golden("orient_sequence.npz")
    result = fits[name][0]
    dx = np.abs(result.x - g[f"fit_{name}_x"]).max()
    dfun = abs(result.fun - g[f"fit_{name}_fun"])
    print(name, "max |dx|", dx, "deg, |dfun|", dfun, "nit", result.nit, int(g[f"fit_{name}_nit"]))
    assert dx <= 10 * measured[0]
    assert dfun <= 10 * measured[1]
    assert result.nit == g[f"fit_{name}_nit"]
    assert bool(result.success) == bool(g[f"fit_{name}_success"])


def test_fit_takes_the_other_forms_of_matches(golden, fits):
    g = golden("orient_sequence.npz")
    model, _ = oc.observer_of(g)
    as_dict = model.matches
    model.matches = type("Coo", (), dict(data=list(as_dict.values()), row=g["pair_i"], col=g["pair_j"]))()
    result, _ = _fit(model, options={"maxiter": 5})
    assert np.array_equal(_bits(result.x), _bits(fits["maxiter5"][0].x))


def test_handles_come_and_go(golden, lib):
    g = golden("orient_sequence.npz")
    pairs = oc.pairs_of(g)
    args = (5, g["pair_i"], g["pair_j"], g["offsets"], g["xy_i"], g["xy_j"])
    for _ in range(50):
        lib.Orient(*args).close()
    handle = lib.Orient(*args)
    handle.close()
    handle.close()
    with pytest.raises(lib.GlhError, match="closed"):
        handle.eval(np.zeros((5, 3, 3)), np.zeros((5, 3, 3, 3)))
    # no pair at all: an objective of 0 and no gradient
    with lib.Orient(3, [], [], [0], np.empty((0, 2)), np.empty((0, 2))) as empty:
        objective, gradient = empty.eval(np.zeros((3, 3, 3)), np.zeros((3, 3, 3, 3)))
        assert objective == 0.0 and gradient.shape == (3, 3) and not gradient.any()
        assert not _bits(objective).any() and not _bits(gradient).any()  # exactly +0, not -0
    assert len(pairs) == 6


@pytest.mark.parametrize("change, message", [
    (dict(offsets=[0, 1, 64, 60, 193, 450, 1450]), "pair_offset decreases at pair 2"),
    (dict(offsets=[1, 1, 64, 128, 193, 450, 1450]), r"pair_offset\[0\] is 1, not 0"),
    (dict(pair_j=[1, 2, 2, 3, 1, 5]), "pair 5 joins images 2 and 5 of 5"),
    (dict(pair_i=[0, 0, -1, 1, 3, 2]), "pair 2 joins images -1 and 2 of 5"),
    (dict(n_images=0), "0 images"),
])
def test_create_refuses_inconsistent_arguments(golden, lib, change, message):
    """GLH_E_INVALID with a message, before a device is touched (the checks precede hipSetDevice in glh_orient_create: an
    absurd device number is not even looked at)."""
    g = golden("orient_sequence.npz")
    kw = dict(n_images=5, pair_i=g["pair_i"], pair_j=g["pair_j"], offsets=g["offsets"])
    kw.update(change)
    with pytest.raises(lib.GlhError, match=message) as e:
        lib.Orient(kw["n_images"], kw["pair_i"], kw["pair_j"], kw["offsets"], g["xy_i"], g["xy_j"], device_id=1 << 20)
    assert e.value.code == -1
    with pytest.raises(ValueError, match="N >= pair_offset.max"):  # rows the offsets name must exist: refused on the host
        lib.Orient(5, g["pair_i"], g["pair_j"], g["offsets"], g["xy_i"][:-1], g["xy_j"][:-1])
