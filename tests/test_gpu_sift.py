"""SIFT on the device (glh_sift_detect, glimpse_amd/csrc/glh_sift.hip) against its NumPy restatement
(tests/sift_restated.py), stage by stage and bit for bit: every Gaussian and DoG layer, the sorted candidate list, the
refined list, the angles and the descriptors, then the public surface with every parameter, the handle's reuse, and
KeypointMatcher from images to matches on the integer path.

The images (tests/sift_cases.py): 61 x 47 and 47 x 61 (odd sides: odd decimation, partial blocks), 256 x 192 (many blocks
of every kernel), a 12 x 40 strip (its second octave is 12 cells wide: two interior columns), 5 x 5 (no octave) and
400 x 300 (more candidates than a fresh handle's list holds: the extrema run twice)."""
import datetime

import numpy as np
import pytest

from tests import sift_cases as sc
from tests import sift_restated as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    _lib.load()
    return _lib


def same_bits(found, expected, what):
    found, expected = np.ascontiguousarray(found), np.ascontiguousarray(expected)  # (column slices are strided)
    assert found.dtype == expected.dtype and found.shape == expected.shape, (what, found.dtype, found.shape, expected.shape)
    assert np.array_equal(found.view(np.uint8), expected.view(np.uint8)), what


def every_stage(lib, sift, name, **params):
    """One detection of image `name` on the handle `sift`: every stage against the restatement's, bit for bit (the number
    of differing bytes of each stage is printed first).  Returns what `detect` gave."""
    st = sc.stages(name, **params)
    layers = params.get("nOctaveLayers", 3)
    kps, desc = sift.detect(sc.image(name), n_layers=layers, sigma=params.get("sigma", 1.6))
    counts = sift.counts()
    assert counts["octaves"] == len(st["gauss"]) and counts["layers"] == layers
    assert all(len(gauss) == layers + 3 and len(dog) == layers + 2 for gauss, dog in zip(st["gauss"], st["dog"]))
    compared = []
    for o, (gauss, dog) in enumerate(zip(st["gauss"], st["dog"])):
        compared += [(sift.layer(lib.SIFT_GAUSS, o, i), layer, f"Gaussian layer {i} of octave {o}") for i, layer in enumerate(gauss)]
        compared += [(sift.layer(lib.SIFT_DOG, o, i), layer, f"DoG layer {i} of octave {o}") for i, layer in enumerate(dog)]
    refined = sift.layer(lib.SIFT_REFINED)
    compared += [(sift.layer(lib.SIFT_CANDIDATES), st["candidates"], "candidates"),
                 (refined[:, 0], st["refined"][:, 0], "which rule rejected which candidate"),
                 (refined[:, 1:5], st["refined"][:, 1:5], "settled cells"),
                 (refined, st["refined"], "refined list: offsets, contrast, size, position"),
                 (sift.layer(lib.SIFT_CELLS), st["cells"], "keypoint cells and orientation bins"),
                 (kps[:, [0, 1, 2, 4, 5]], st["keypoints"][:, [0, 1, 2, 4, 5]], "position, size, response, octave"),
                 (kps[:, 3], st["keypoints"][:, 3], "angles"), (desc, st["descriptors"], "descriptors")]
    differing = {what: (int(np.count_nonzero(np.ascontiguousarray(f).view(np.uint8) != np.ascontiguousarray(e).view(np.uint8)))
                        if f.shape == e.shape and f.dtype == e.dtype else f"shape {f.shape}, not {e.shape}")
                 for f, e, what in compared}
    print(name, params, counts, "differing bytes:", {w: n for w, n in differing.items() if n} or "none in",
          len(compared), "arrays")
    for found, expected, what in compared:
        same_bits(found, expected, what)
    return kps, desc


@pytest.mark.parametrize("name", ["61x47", "47x61", "256x192", "strip"])
def test_every_stage_equals_the_restatement(lib, name):
    st = sc.stages(name)
    trace = st["trace"]
    if name in sc.FULL:  # nothing below passes vacuously
        assert len(st["keypoints"]) >= 30 and len(trace["octaves"]) >= 3
        for what in ("moved", "contrast", "edge", "border", "two_orientations", "clipped"):
            assert trace[what] >= 1, what
    with lib.Sift() as sift:
        every_stage(lib, sift, name)


@pytest.mark.parametrize("name, layers", [("47x61", 8), ("strip", 8), ("strip", 1)])
def test_every_stage_at_the_ends_of_the_layer_range(lib, name, layers):
    """Eleven Gaussian and ten DoG layers per octave with nOctaveLayers = 8, and with 1 the blurs of radius 11, 22 and 45,
    which on the strip's octaves (24 and 12 cells wide) fold the reflection up to four times."""
    with lib.Sift() as sift:
        every_stage(lib, sift, name, nOctaveLayers=layers)


@pytest.fixture(scope="module")
def fresh_300x400(lib):
    """A fresh handle's first detection on "300x400" (4446 candidates for a list of 4096: two attempts), every stage
    compared; the handle and what it gave."""
    assert len(sc.stages("300x400")["candidates"]) > sc.LIST_SLOTS
    with lib.Sift() as sift:
        yield sift, every_stage(lib, sift, "300x400")


def test_candidate_list_overflows_and_the_octaves_run_again(lib, fresh_300x400):
    """The second attempt of the candidate list (glh_sift.hip: "the counter goes on counting past `cap`"): every stage of
    the first detection on a fresh handle (the fixture), then the same handle again, whose list is now long enough for
    one attempt: the same bytes, every stage again."""
    sift, (kps, desc) = fresh_300x400
    assert sift.counts()["candidates"] == len(sc.stages("300x400")["candidates"]) > sc.LIST_SLOTS
    again = every_stage(lib, sift, "300x400")
    same_bits(again[0], kps, "one attempt after two: keypoints")
    same_bits(again[1], desc, "one attempt after two: descriptors")


def test_candidate_list_grows_on_a_used_handle_and_serves_a_small_image_after(lib, fresh_300x400):
    """A handle that has detected on "61x47" (94 candidates), then "300x400": equal to the fresh handle's; then "61x47"
    on the grown handle: equal to a fresh handle's, every stage."""
    _, (kps, desc) = fresh_300x400
    with lib.Sift() as used, lib.Sift() as fresh_small:
        small = every_stage(lib, fresh_small, "61x47")
        used.detect(sc.image("61x47"))
        grown = every_stage(lib, used, "300x400")
        same_bits(grown[0], kps, "grown handle: keypoints")
        same_bits(grown[1], desc, "grown handle: descriptors")
        after = every_stage(lib, used, "61x47")
        same_bits(after[0], small[0], "small image on the grown handle: keypoints")
        same_bits(after[1], small[1], "small image on the grown handle: descriptors")


def _arrays(keypoints, descriptors):
    kps = np.array([[k.pt[0], k.pt[1], k.size, k.angle, k.response, k.octave] for k in keypoints], np.float64).reshape(-1, 6)
    return kps, descriptors


@pytest.mark.parametrize("kwargs", [
    {}, {"nOctaveLayers": 2}, {"contrastThreshold": 0.08}, {"edgeThreshold": 5}, {"sigma": 1.2}, {"mask": True},
    {"nfeatures": 10}, {"root": True}], ids=lambda k: "-".join(k) or "defaults")
@pytest.mark.parametrize("name", ["61x47", "47x61"])
def test_detect_keypoints_equals_the_restatement(lib, name, kwargs):
    detect_keypoints_case(name, kwargs)


@pytest.mark.parametrize("kwargs", [{"nOctaveLayers": 1}, {"nOctaveLayers": 8}, {"nOctaveLayers": 8, "sigma": 2.4}],
                         ids=["1", "8", "8-sigma2.4"])
@pytest.mark.parametrize("name", ["61x47", "47x61"])
def test_detect_keypoints_at_the_ends_of_the_layer_range(lib, name, kwargs):
    """nOctaveLayers 1 and 8, the ends of what is served: the [SF_MAX_LAYERS + 3] tables full, the layer field of the
    sort key and the octave packing up to 8 (tests/test_sift_restated.py asserts that keypoints of layer 8 are there),
    and with one layer a last blur of radius 45 in octaves of 12 to 16 rows."""
    detect_keypoints_case(name, kwargs)


def detect_keypoints_case(name, kwargs):
    from glimpse_amd import optimize

    kwargs = dict(kwargs)
    mask = sc.mask_of(name) if kwargs.pop("mask", None) else None
    root = kwargs.pop("root", False)
    nfeatures = kwargs.pop("nfeatures", 0)
    st = sc.stages(name, **kwargs)
    expected_k, expected_d = sr.finish(st["keypoints"], st["descriptors"], mask, nfeatures)
    assert len(expected_k) >= 5
    if mask is not None or nfeatures:
        assert len(expected_k) < len(st["keypoints"])
    keypoints, descriptors = optimize.detect_keypoints(sc.image(name), mask=mask, method=optimize.SIFT, root=root,
                                                       nfeatures=nfeatures, **kwargs)
    assert all(type(k) is optimize.KeyPoint and k.class_id == -1 and type(k.octave) is int for k in keypoints)
    found_k, found_d = _arrays(keypoints, descriptors)
    print(name, kwargs, len(found_k), "keypoints, expected", len(expected_k), "; differing keypoint values:",
          int(np.count_nonzero(found_k.view(np.uint64) != expected_k.view(np.uint64))) if found_k.shape == expected_k.shape else "-")
    same_bits(found_k, expected_k, "keypoints")
    if root:
        expected_d = sr.root_descriptors(expected_d)
    same_bits(found_d, expected_d, "descriptors")


def test_large_image_through_the_public_surface(lib):
    from glimpse_amd import optimize

    st = sc.stages("256x192")
    keypoints, descriptors = optimize.detect_keypoints(sc.image("256x192"), method=optimize.SIFT)
    expected_k, expected_d = sr.finish(st["keypoints"], st["descriptors"])
    same_bits(_arrays(keypoints, descriptors)[0], expected_k, "keypoints")
    same_bits(descriptors, expected_d, "descriptors")


def test_empty_result_and_arguments(lib):
    from glimpse_amd import optimize

    assert optimize.detect_keypoints(sc.image("5x5"), method=optimize.SIFT) == ([], None)
    with lib.Sift() as sift:
        kps, desc = sift.detect(sc.image("5x5"))
        assert kps.shape == (0, 6) and desc.shape == (0, 128) and sift.counts()["octaves"] == 0
        kps, desc = sift.detect(np.full((40, 40), 7, np.uint8))  # octaves, but nothing in them
        assert kps.shape == (0, 6) and sift.counts()["candidates"] == 0 and sift.counts()["octaves"] == 3
        n = np.zeros(1, np.int32)
        strip = sc.image("strip")
        for params, w, h, message in (([9.0, 0.04, 10.0, 1.6], 12, 40, "nOctaveLayers"),
                                      ([3.0, 0.04, 10.0, 99.0], 12, 40, "sigma"),
                                      ([3.0, 0.04, 10.0, 1.6], 1 << 15, 1 << 15, "2\\^31 cells")):
            with pytest.raises(lib.GlhError, match=message):
                lib.check(lib.load().glh_sift_detect(sift._h, lib._ptr(strip), w, h, lib._ptr(np.array(params)), lib._ptr(n),
                                                     None))
    assert lib.load().glh_sift_destroy(None) == 0 and lib.load().glh_sift_create(0, None) == -1


def test_handle_is_reused_across_calls_and_sizes(lib):
    a, b = sc.image("61x47"), sc.image("256x192")
    with lib.Sift() as fresh_a, lib.Sift() as fresh_b, lib.Sift() as reused:
        first = reused.detect(a)
        second = reused.detect(a)
        same_bits(first[0], second[0], "two calls: keypoints")
        same_bits(first[1], second[1], "two calls: descriptors")
        for img, fresh in ((b, fresh_b), (a, fresh_a)):  # grows, then shrinks
            found, expected = reused.detect(img), fresh.detect(img)
            same_bits(found[0], expected[0], "reused handle: keypoints")
            same_bits(found[1], expected[1], "reused handle: descriptors")


def _images(tmp_path):
    import glimpse_amd

    big = sc.texture(140, 200, seed=5)
    crops = [big[8:128, 16:176], big[0:120, 0:160]]  # the second is the first moved by (16, 8) px
    cam = dict(imgsz=(160, 120), f=(200, 200))
    return [glimpse_amd.Image(str(tmp_path / f"crop_{i}.png"), cam=glimpse_amd.Camera(**cam), array=crop,
                              datetime=datetime.datetime(2020, 1, 1 + i)) for i, crop in enumerate(crops)]


def test_images_to_matches_on_the_integer_path(lib, tmp_path):
    from glimpse_amd import optimize

    model = optimize.KeypointMatcher(_images(tmp_path))
    model.build_keypoints(method=optimize.SIFT, clear_images=False)
    assert all(d.dtype == np.uint8 and len(k) == len(d) >= 30 for k, d in model.keypoints)
    paths = []
    original = lib.Matcher.put

    def put(self, slot, descriptors, path=None):
        paths.append(original(self, slot, descriptors, path))
        return paths[-1]

    lib.Matcher.put = put
    try:
        model.build_matches(cross_check=True, max_ratio=0.7)
    finally:
        lib.Matcher.put = original
    assert paths and set(paths) == {"integer"}
    m = model.matches.data[0]
    assert len(model.matches.data) == 1
    assert len(m.uvs[0]) >= 10
    shift = np.median(m.uvs[1] - m.uvs[0], axis=0)
    print(len(m.uvs[0]), shift)
    assert np.all(np.abs(shift - (16.0, 8.0)) <= 0.5)


def test_build_keypoints_writes_reads_and_clears(lib, tmp_path):
    from glimpse_amd import helpers, optimize

    images = _images(tmp_path)
    model = optimize.KeypointMatcher(images)
    masks = [None, np.ones((120, 160), np.uint8)]
    made, closed = [], []
    create, close = lib.Sift.__init__, lib.Sift.close

    def counted_init(self, *a, **k):
        made.append(self)
        create(self, *a, **k)

    def counted_close(self):
        if self._h:
            closed.append(self)
        close(self)

    lib.Sift.__init__, lib.Sift.close = counted_init, counted_close
    try:
        model.build_keypoints(masks=masks, path=tmp_path / "kp", method=optimize.SIFT, nfeatures=40)
    finally:
        lib.Sift.__init__, lib.Sift.close = create, close
    assert len(made) == 1 and closed == made  # one handle for all the images, freed when the call ends
    assert all(img.array is None for img in images)
    assert sorted(p.name for p in (tmp_path / "kp").iterdir()) == ["crop_0.pkl", "crop_1.pkl"]
    kept = model.keypoints
    assert all(len(k) == 40 and d.shape == (40, 128) for k, d in kept)
    again = optimize.KeypointMatcher(images)
    again.build_keypoints(path=tmp_path / "kp")  # read back: nothing to detect, no method needed
    for (ka, da), (kb, db) in zip(kept, again.keypoints):
        assert ka == kb and np.array_equal(da, db)
    assert helpers.read_pickle(tmp_path / "kp" / "crop_0.pkl")[0][0] == kept[0][0][0]
