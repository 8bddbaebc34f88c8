"""glimpse_amd.optimize without a device: the restatement of the orientation kernel (tests/orient_restated.py) against the
reference's own callback, the rotation matrices, and the host behaviour of the match classes and of ObserverCameras."""
import types

import numpy as np
import pytest

from tests import orient_cases as oc
from tests import orient_restated as rs

import glimpse_amd
from glimpse_amd import optimize
from glimpse_amd.camera import rotations

U = oc.U


@pytest.mark.parametrize("fixture", oc.FIXTURES)
def test_restatement_against_the_reference_callback(golden, fixture):
    """The restated objective and gradient against those recorded from the reference's closure `fun` at three probe
    points, with anchor_weight 0 (the matches alone) and 1e6.  The bound is derived, not tuned; M is the number of matches.

    matches, objective.  An addend is a component |d_i[r] - d_j[r]| of two unit vectors: per side a 3-term dot, a 3-term
      norm, a reciprocal and a product, then one subtraction, on numbers <= 1: 16 * 2^-53 per addend, 3 M addends.  The
      two sums run in different orders over the same addends: M * 2^-53 * sum |addends|.
    matches, gradient of an image.  The same form: its addends sign * (Rprime[r, w, :] . [x, y, 1]) are below 1 in size
      (Rprime carries pi / 180), 3 per match and component: M * 16 * 2^-53 + M * 2^-53 * sum |addends| of that image.
    anchors.  The reference adds every pair onto the accumulator that already holds the anchor term, so each of those
      additions rounds at the anchor term's size, on top of the few roundings of the term itself: relative to its size,
      (pairs + 4) * 2^-53 * |anchor term|, added to the bounds above when anchor_weight is 1e6.
    Measured on the build machine: at most 2.8e-14 (objective) and 2.3e-13 (gradient) for the matches alone against
    bounds of 7.7e-12 and 2.6e-12 or more; 1.8e-12 and 2.9e-11 with the anchors against 1.6e-11 and 3.2e-10."""
    g = golden(fixture)
    pairs = oc.pairs_of(g)
    n = len(g["viewdirs_start"])
    for tag, weight in (("w0", 0.0), ("w1e6", 1e6)):
        for k, point in enumerate(g["points"]):
            d = {}
            objective, gradient = rs.callback(point, g["viewdirs_start"], g["anchors"], weight, pairs, rotations, d)
            assert d["min_abs_dxyz"] > 1e-9  # (the condition on the fixture's noise: no sign is rounding noise)
            M = d["matches"]
            assert M == g["offsets"][-1]
            bound_o = 3 * M * 16 * U + M * U * d["abs_objective"] + (len(pairs) + 4) * U * abs(d["anchor_objective"])
            bound_g = M * 16 * U + M * U * d["abs_gradient"] + (len(pairs) + 4) * U * np.abs(d["anchor_gradient"])
            err_o = abs(objective - g[f"probe_objective_{tag}"][k])
            err_g = np.abs(gradient - g[f"probe_gradient_{tag}"][k])
            print(fixture, tag, k, "objective", err_o, "of", bound_o, "gradient", err_g.max(), "of", bound_g.min())
            assert gradient.shape == (n, 3)
            assert err_o <= bound_o
            assert (err_g <= bound_g).all()
            if weight == 0.0:
                assert d["anchor_objective"] == 0 and not d["anchor_gradient"].any()


def test_an_image_in_no_pair_has_no_gradient_and_an_empty_pair_adds_nothing(golden):
    g = golden("orient_chunks.npz")
    pairs = oc.pairs_of(g)
    assert [len(p[2]) for p in pairs][:2] == [2 * rs.CHUNK + 37, 0]
    R, Rprime = rotations(g["points"][0])
    objective, gradient = rs.evaluate(6, pairs, R, Rprime)
    assert not gradient[5].any() and not g["probe_gradient_w0"][:, 5].any()
    without = [p for p in pairs if len(p[2])]
    objective_2, gradient_2 = rs.evaluate(6, without, R, Rprime)
    assert np.array_equal(gradient, gradient_2)
    # (the objective's lanes are dealt by pair number, so dropping a pair may move the others: equal only up to rounding)
    assert abs(objective - objective_2) <= 8 * U * objective


@pytest.mark.parametrize("n_images", oc.SYNTHETIC)
def test_the_synthetic_sequences_meet_the_conditions_of_the_gpu_test(n_images):
    """What tests/test_optimize_gpu.py relies on to reach the paths past one workgroup, asserted without a device: the
    image and pair counts, the pair sizes in a lane's first and second turn, the images in no pair, the image that is only
    ever j, the hub, and the noise condition; and the restatement itself inside the longdouble bound."""
    case = oc.synthetic_case(n_images)
    pairs, details = case["pairs"], case["details"]
    workgroups = {256: 1, 257: 2, 300: 2, 600: 3}[n_images]
    assert len(case["R"]) == n_images and -(-n_images // rs.TB) == workgroups
    assert -(-len(pairs) // rs.TB) >= max(2, workgroups)  # the objective's lanes take that many turns
    order = [(i, j) for i, j, _, _ in pairs]
    assert order == sorted(order) and len(set(order)) == len(order) and all(i != j for i, j in order)
    assert all((i, i + d) in order for i in (0, 1, 50, n_images - 8) for d in (1, 2))  # the chain
    sizes = [len(p[2]) for p in pairs]
    assert all(len(p[3]) == m for p, m in zip(pairs, sizes))
    assert sizes[3:12] == list(oc.PAIR_SIZES) == sizes[260:269] and oc.PAIR_SIZES == (0, 1, 255, 256, 257, 4095, 4096, 4097, 8193)
    xy = np.concatenate([p[2] for p in pairs])
    assert np.abs(xy).max() <= 0.4 and np.abs(xy).max() > 0.39
    members = [set(i for i, _ in order), set(j for _, j in order)]
    isolated = oc.synthetic_isolated(n_images)
    assert isolated[0] < 256 and not (members[0] | members[1]) & set(isolated)
    assert len(isolated) == (2 if n_images > 256 else 1) and all(m >= 256 for m in isolated[1:])  # (256 images: none past 255)
    assert not case["want"][1][isolated].any() and not np.signbit(case["want"][1][isolated]).any()  # exactly +0
    only_j = members[1] - members[0]
    assert only_j and all(np.any(case["want"][1][m] != 0) for m in only_j)
    assert 0 in members[0] - members[1]
    hub_i, hub_j = [j for i, j in order if i == oc.HUB], [i for i, j in order if j == oc.HUB]
    others = n_images - 3 - len(isolated)  # not the hub, not the two end images, not the isolated ones
    assert len(hub_i) >= 150 and len(hub_j) >= 150 and len(hub_i) + len(hub_j) >= 300
    assert len(set(hub_i) | set(hub_j)) >= min(300, others)  # other images as far as there are any
    assert details["min_abs_dxyz"] > 1e-9
    assert details["matches"] == sum(sizes) >= 2 * sum(oc.PAIR_SIZES)
    bound_o, bound_g = oc.longdouble_bounds(details, case["exact"][2])
    (err_o, ratio_o), (err_g, ratio_g) = oc.longdouble_ratios(case["want"], case["exact"], details)
    print(n_images, "images,", len(pairs), "pairs,", details["matches"], "matches, min |dxyz|", details["min_abs_dxyz"],
          "ratio to u sum |addend|: objective", ratio_o, "gradient", ratio_g)
    assert err_o <= bound_o and (err_g <= bound_g).all()
    if n_images == 257:  # the case that goes through ObserverCameras: the same conditions half a degree off the start
        model, same_pairs = oc.synthetic_observer(257)
        assert same_pairs is pairs and list(model.matches) == order and model.anchors == [0, 130]
        assert [(i, j) for _, i, j in optimize.match_pairs(model.matches)] == order
        d = {}
        rs.callback(oc.synthetic_probe(case["viewdirs"]), case["viewdirs"], model.anchors, 1e6, pairs, rotations, d)
        assert d["min_abs_dxyz"] > 1e-9 and d["anchor_objective"] > 0


def test_rotations_equal_the_properties_and_the_reference_bit_for_bit(golden):
    for fixture in oc.FIXTURES:
        g = golden(fixture)
        R, Rprime = rotations(g["viewdirs_start"])
        assert R.shape == (len(R), 3, 3) and Rprime.shape == (len(R), 3, 3, 3)
        assert R.flags.c_contiguous and Rprime.flags.c_contiguous
        assert np.array_equal(R, g["R"])
        assert np.array_equal(Rprime, g["Rprime"])  # the reference's Camera.Rprime
        for n, v in enumerate(g["viewdirs_start"]):
            cam = glimpse_amd.Camera(viewdir=v, **oc.internals(g))
            assert np.array_equal(cam.R, R[n])
            assert np.array_equal(cam.Rprime, Rprime[n])
    rng = np.random.default_rng(5)
    wide = rng.uniform(-180, 180, (257, 3))
    R, Rprime = rotations(wide)
    for n in (0, 1, 63, 64, 255, 256):
        cam = glimpse_amd.Camera(imgsz=(10, 10), f=10, viewdir=wide[n])
        assert np.array_equal(cam.R, R[n]) and np.array_equal(cam.Rprime, Rprime[n])


def _cams(**kwargs):
    kw = dict(imgsz=(100, 80), f=(120, 120), k=(0.1, 0, 0, 0, 0, 0))
    return [glimpse_amd.Camera(viewdir=(1, 2, 0), **kw, **kwargs), glimpse_amd.Camera(viewdir=(2, 1, 0), **kw, **kwargs)]


XYS = [np.array([[0.1, 0.2], [0.0, -0.1], [0.3, 0.1]]), np.array([[0.11, 0.2], [0.01, -0.1], [0.31, 0.1]])]
UVS = [np.array([[10.0, 20.0], [30.0, 40.0], [50.0, 60.0]]), np.array([[11.0, 21.0], [31.0, 41.0], [51.0, 61.0]])]


@pytest.mark.parametrize("make", [
    lambda cams, pts: optimize.Matches(cams=cams, uvs=pts),
    lambda cams, pts: optimize.RotationMatches(cams=cams, uvs=pts, xys=pts),
    lambda cams, pts: optimize.RotationMatchesXY(cams=cams, xys=pts),
    lambda cams, pts: optimize.RotationMatchesXYZ(cams=cams, xys=pts),
], ids=["Matches", "RotationMatches", "RotationMatchesXY", "RotationMatchesXYZ"])
def test_constructor_checks(make):
    cams = _cams()
    assert make(cams, XYS).size == 3
    with pytest.raises(ValueError, match="Both cameras are the same object"):
        make([cams[0], cams[0]], XYS)
    with pytest.raises(ValueError, match="Cameras and point coordinates do not have two elements each"):
        make(cams, [XYS[0], XYS[1], XYS[1]])
    with pytest.raises(ValueError, match="Cameras and point coordinates do not have two elements each"):
        make([cams[0], cams[1], cams[1].copy()], XYS)
    with pytest.raises(ValueError, match="Camera point coordinates do not have the same length"):
        make(cams, [XYS[0], XYS[1][:2]])


def test_position_and_internals_checks():
    cams = _cams()
    apart = [cams[0], glimpse_amd.Camera(imgsz=(100, 80), f=120, xyz=(1, 0, 0))]
    with pytest.raises(ValueError, match="Cameras have different positions"):
        optimize.Matches(cams=apart, uvs=UVS)
    m = optimize.RotationMatchesXYZ(cams=apart, xys=XYS)  # (the rotation classes test the position when they predict)
    with pytest.raises(ValueError, match="Cameras have different positions"):
        m.predicted()
    with pytest.raises(ValueError, match="Both uvs and xys are missing"):
        optimize.RotationMatches(cams=cams)
    for mtype in (optimize.RotationMatchesXY, optimize.RotationMatchesXYZ):
        cams = _cams()
        m = mtype(cams=cams, xys=XYS)
        cams[1].viewdir = (3, 3, 3)  # an external parameter may change
        m.predicted()
        cams[1].f = (121, 120)
        with pytest.raises(ValueError, match=r"Camera internal parameters \(imgsz, f, c, k, p\) have changed"):
            m.predicted()
    m = optimize.Matches(cams=_cams(), uvs=UVS)
    with pytest.raises(IndexError, match="Camera index out of range"):
        m.observed(cam=2)
    assert m._cam_index(m.cams[1]) == 1


def test_xyz_predicted_is_the_unit_ray_and_observed_is_not_there():
    cams = _cams()
    m = optimize.RotationMatchesXYZ(cams=cams, xys=XYS)
    for c in (0, 1):
        d = m.predicted(cam=c)
        assert d.shape == (3, 3)
        expected = rs.rays(cams[c].R, XYS[c])
        assert np.array_equal(d, np.column_stack(expected))
    with pytest.raises(NotImplementedError):
        m.observed()
    with pytest.raises(NotImplementedError):
        m.plot()
    xy = optimize.RotationMatchesXY(cams=cams, xys=XYS)
    assert np.array_equal(xy.observed(cam=1), XYS[1])
    assert np.abs(xy.predicted(cam=0) - XYS[0]).max() < 0.05  # the other camera's points, a degree or two away


def test_to_type_on_the_host():
    cams = _cams()
    weights = np.array([0.5, 0.25, 1.0])
    xy = optimize.RotationMatchesXY(cams=cams, uvs=UVS, xys=XYS, weights=weights)
    assert xy.to_type(optimize.RotationMatchesXY) is xy
    for mtype in (optimize.RotationMatchesXYZ, optimize.RotationMatches):
        other = xy.to_type(mtype)
        assert type(other) is mtype and other.cams is cams and other.weights is weights
        assert all(np.array_equal(a, b) for a, b in zip(other.xys, XYS))
        assert all(np.array_equal(a, b) for a, b in zip(other.uvs, UVS))
    plain = xy.to_type(optimize.Matches)
    assert type(plain) is optimize.Matches and all(np.array_equal(a, b) for a, b in zip(plain.uvs, UVS))
    # without image coordinates they are made from the camera coordinates: distortion, focal length, principal point
    xyz = optimize.RotationMatchesXYZ(cams=cams, xys=XYS)
    assert xyz.uvs is None
    plain = xyz.to_type(optimize.Matches)
    x, y = XYS[0][:, 0], XYS[0][:, 1]
    dr = 1 + 0.1 * (x * x + y * y)
    assert np.allclose(plain.uvs[0], np.column_stack((x * dr * 120 + 50, y * dr * 120 + 40)), rtol=1e-15, atol=0)
    assert plain.to_type(optimize.Matches) is plain
    back = xyz.to_type(optimize.RotationMatchesXY)
    assert type(back) is optimize.RotationMatchesXY and all(np.array_equal(a, b) for a, b in zip(back.xys, XYS))


def test_filter_on_weights_alone():
    weights = np.array([0.5, 0.25, 1.0])
    m = optimize.Matches(cams=_cams(), uvs=UVS, weights=weights.copy())
    m.filter(n_best=2)
    assert m.size == 2 and np.array_equal(m.weights, [0.5, 1.0]) and np.array_equal(m.uvs[1], UVS[1][[0, 2]])
    m = optimize.Matches(cams=_cams(), uvs=UVS, weights=weights.copy())
    m.filter(min_weight=0.5)
    assert np.array_equal(m.uvs[0], UVS[0][[0, 2]])
    m = optimize.Matches(cams=_cams(), uvs=UVS, weights=weights.copy())
    m.filter(n_best=5, min_weight=0.6)
    assert np.array_equal(m.uvs[0], UVS[0][[2]]) and np.array_equal(m.weights, [1.0])
    m = optimize.RotationMatchesXY(cams=_cams(), uvs=UVS, xys=XYS, weights=weights.copy())
    m.filter(n_best=1)
    assert m.size == 1 and np.array_equal(m.xys[0], XYS[0][[2]]) and np.array_equal(m.uvs[0], UVS[0][[2]])
    with pytest.raises(ValueError, match="Filtering on weights failed since these are missing"):
        optimize.Matches(cams=_cams(), uvs=UVS).filter(n_best=1)


def test_resize_scales_the_image_coordinates():
    m = optimize.Matches(cams=_cams(), uvs=[uv.copy() for uv in UVS])
    m.resize(0.5)
    assert np.array_equal(m.cams[0].imgsz, [50, 40]) and np.array_equal(m.uvs[0], UVS[0] * 0.5)
    m.resize()  # nothing has changed since
    assert np.array_equal(m.uvs[1], UVS[1] * 0.5)


def test_the_three_forms_of_matches_give_the_same_coo_order(golden):
    import scipy.sparse

    g = golden("orient_sequence.npz")
    model, _ = oc.observer_of(g)
    as_dict = model.matches
    order = [(i, j) for i, j, _, _ in oc.pairs_of(g)]
    assert [(i, j) for _, i, j in optimize.match_pairs(as_dict)] == order
    assert (3, 1) in order and order.index((1, 3)) < order.index((3, 1))
    # a COO-like object and a dict keep the order they were given (the fixture's: (3, 1) before (2, 4)) ...
    coo = types.SimpleNamespace(data=list(as_dict.values()), row=g["pair_i"], col=g["pair_j"])
    got = optimize.match_pairs(coo)
    assert [(i, j) for _, i, j in got] == order and all(m is as_dict[i, j] for m, i, j in got)
    # ... an (n, n) grid is read row by row, which is the order scipy.sparse.coo_matrix gives a dense array; with the
    # pairs given in that order, the three forms agree
    by_rows = sorted(order)
    assert by_rows != order
    grid = np.full((5, 5), None, dtype=object)
    zeros = np.zeros((5, 5), dtype=object)
    for (i, j), m in as_dict.items():
        grid[i, j] = zeros[i, j] = m
    dense = scipy.sparse.coo_matrix(np.array([[0 if v is None else 1 for v in row] for row in grid]))
    assert list(zip(dense.row.tolist(), dense.col.tolist())) == by_rows
    sorted_dict = {key: as_dict[key] for key in by_rows}
    sorted_coo = types.SimpleNamespace(data=list(sorted_dict.values()), row=[i for i, _ in by_rows], col=[j for _, j in by_rows])
    for form in (grid, zeros, sorted_dict, sorted_coo):
        got = optimize.match_pairs(form)
        assert [(i, j) for _, i, j in got] == by_rows
        assert all(m is as_dict[i, j] for m, i, j in got)
    with pytest.raises(ValueError, match="matches are missing"):
        optimize.match_pairs(None)


def test_observer_cameras_on_the_host(golden):
    g = golden("orient_sequence.npz")
    model, cams = oc.observer_of(g)
    assert np.array_equal(model.viewdirs, g["viewdirs_start"]) and model.anchors == [0, 3]
    assert optimize.ObserverCameras(model.observer).anchors == [0]
    model.set_cameras(g["viewdirs_true"])
    assert np.array_equal(cams[2].viewdir, g["viewdirs_true"][2])
    model.reset_cameras()
    assert all(np.array_equal(cam.viewdir, v) for cam, v in zip(cams, g["viewdirs_start"]))
    for call in (model.build_keypoints, model.build_matches, optimize.KeypointMatcher):
        with pytest.raises(NotImplementedError, match=r"SIFT and FLANN.*cv2.*pass the matches"):
            call()
    # matches between other cameras than the observer's are refused before anything is uploaded
    stranger = optimize.RotationMatchesXYZ(cams=[cams[0], cams[1].copy()], xys=XYS)
    model.matches = {(0, 1): stranger}
    with pytest.raises(ValueError, match="not between the cameras of images 0 and 1"):
        model.fit()
    assert "optimize" in glimpse_amd.__all__ and glimpse_amd.ObserverCameras is optimize.ObserverCameras
