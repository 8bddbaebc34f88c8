"""CLAHE on the device (glh_stage_clahe, glimpse_amd/csrc/glh_clahe.hip) against its NumPy restatement
(tests/clahe_restated.py), byte for byte and with no tolerance: every tile's table and the image of every case of the
restatement's table, the channel mean on the device, the arguments the C ABI refuses, and KeypointMatcher from colour frames
through CLAHE to SIFT keypoints.

The cases (tests/clahe_restated.py: CASES) are the smallest that reach each path: a divisible and a padded image, an odd
width (the byte path of the blend), a grid that is not square with every tile clipped and a step of 1, no clipping, one
tile, tiles of 2 x 2, several row slices per tile, one bin holding everything, 393 216 pixels per tile, two bins only, and
a grid as wide as the image."""
import datetime

import numpy as np
import pytest

from tests import clahe_restated as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    _lib.load()
    return _lib


def same_bytes(found, expected, what):
    assert found.dtype == expected.dtype == np.uint8 and found.shape == expected.shape, (what, found.dtype, found.shape)
    print(what, "differing bytes:", int(np.count_nonzero(found != expected)), "of", expected.size)
    assert np.array_equal(found, expected), what


def test_every_case_equals_the_restatement(lib):
    residual = step_one = padded = False
    for name, (h, w, clip, grid, _) in cr.CASES.items():
        dst, L, reach = cr.expected(name)
        found, found_luts = lib.stage_clahe(cr.frame(name), clip, grid, return_luts=True)
        same_bytes(found_luts, L, f"{name}: tables")
        same_bytes(found, dst, f"{name}: image")
        residual |= any(r != 0 for r in reach["residual"])
        step_one |= any(s == 1 for s in reach["step"])
        padded |= reach["padded"]
    assert residual and step_one and padded  # (the table still reaches every branch of the rule)
    assert np.array_equal(cr.expected("constant255")[0], cr.frame("constant255"))


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_channel_mean_on_the_device(lib, c):
    array = cr.colour(47, 61, c)
    gray = array.mean(axis=2).astype(np.uint8)
    expected, L = cr.apply(gray, 3.0, (8, 8))
    found, found_luts = lib.stage_clahe(array, 3.0, (8, 8), return_luts=True)
    same_bytes(found_luts, L, f"{c} channels: tables")
    same_bytes(found, expected, f"{c} channels: image")
    wide = cr.colour(48, 64, c)  # the word path of the blend reads the gray plane the histogram kernel wrote
    same_bytes(lib.stage_clahe(wide, 3.0, (8, 8)), cr.apply(wide.mean(axis=2).astype(np.uint8), 3.0, (8, 8))[0],
               f"{c} channels, width 64: image")


def _matcher(frames, tmp_path, clahe):
    import glimpse_amd
    from glimpse_amd import optimize

    h, w = frames[0].shape[:2]
    images = [glimpse_amd.Image(str(tmp_path / f"frame_{i}.png"), cam=glimpse_amd.Camera(imgsz=(w, h), f=(200, 200)), array=a,
                                datetime=datetime.datetime(2020, 1, 1 + i)) for i, a in enumerate(frames)]
    return optimize.KeypointMatcher(images, clahe=clahe)


def test_float_frames_take_the_host_mean_and_give_the_same(lib, tmp_path):
    from glimpse_amd import optimize

    rgb = cr.colour(47, 61, 3)
    model = _matcher([rgb, rgb], tmp_path, optimize.CLAHE(clipLimit=3.0))
    expected = cr.apply(cr.channel_mean(rgb), 3.0, (8, 8))[0]
    same_bytes(model._prepare_image(rgb), expected, "uint8 frame: one stage call with the channels")
    same_bytes(model._prepare_image(rgb.astype(np.float64)), expected, "float64 frame: host mean, then apply")
    same_bytes(optimize.CLAHE(clipLimit=3.0).apply(cr.channel_mean(rgb)), expected, "apply")


def test_two_calls_give_the_same_bytes_and_the_input_is_not_written(lib):
    for array in (cr.colour(47, 61, 3), np.array(cr.frame("slices-clip3"))):
        before = array.copy()
        first = lib.stage_clahe(array, 3.0, (8, 8), return_luts=True)
        second = lib.stage_clahe(array, 3.0, (8, 8), return_luts=True)
        same_bytes(second[0], first[0], "two calls: image")
        same_bytes(second[1], first[1], "two calls: tables")
        assert np.array_equal(array, before)
    out, times = lib.stage_clahe(before, 3.0, (8, 8), return_times=True)
    same_bytes(out, first[0], "with times: image")
    assert list(times) == list(lib.CLAHE_TIMES) and all(t >= 0.0 for t in times.values())
    out, luts, times = lib.stage_clahe(before, 3.0, (8, 8), return_luts=True, return_times=True)
    same_bytes(luts, first[1], "with times: tables")


def test_invalid_arguments_raise_and_a_valid_call_works_after(lib):
    src = np.array(cr.frame("divisible"))
    h, w = src.shape
    dst = np.empty_like(src)
    fn = lib.load().glh_stage_clahe
    bad = {
        "null src": (None, w, h, 1, 40.0, 8, 8, dst),
        "null dst": (src, w, h, 1, 40.0, 8, 8, None),
        "w 0": (src, 0, h, 1, 40.0, 8, 8, dst),
        "h 0": (src, w, 0, 1, 40.0, 8, 8, dst),
        "2^31 pixels": (src, 1 << 16, 1 << 15, 1, 40.0, 8, 8, dst),
        "0 channels": (src, w, h, 0, 40.0, 8, 8, dst),
        "5 channels": (src, w, h, 5, 40.0, 8, 8, dst),
        "tiles_x 0": (src, w, h, 1, 40.0, 0, 8, dst),
        "tiles_x above w": (src, w, h, 1, 40.0, w + 1, 8, dst),
        "tiles_y 0": (src, w, h, 1, 40.0, 8, 0, dst),
        "tiles_y above h": (src, w, h, 1, 40.0, 8, h + 1, dst),
        "nan clip": (src, w, h, 1, float("nan"), 8, 8, dst),
        "inf clip": (src, w, h, 1, float("inf"), 8, 8, dst),
    }
    for what, (s, ww, hh, c, clip, gx, gy, d) in bad.items():
        rc = fn(0, lib._ptr(s), ww, hh, c, clip, gx, gy, lib._ptr(d), None, None)
        assert rc == -1, (what, rc)  # GLH_E_INVALID
        with pytest.raises(lib.GlhError, match="clahe"):
            lib.check(rc)
    with pytest.raises(lib.GlhError):
        lib.stage_clahe(src, 40.0, (w + 1, 8))
    same_bytes(lib.stage_clahe(src, 40.0, (8, 8)), cr.expected("divisible")[0], "a valid call afterwards")


def test_frames_through_clahe_to_keypoints(lib, tmp_path):
    """Two 96 x 128 x 3 frames of low-contrast texture near white: KeypointMatcher with a CLAHE finds the keypoints the
    restated SIFT finds on the restated CLAHE of the channel mean -- at least 20, and more than without CLAHE (tests/
    test_clahe.py checks the same on the CPU), so a matcher that skipped the stage would fail here."""
    from glimpse_amd import optimize
    from tests import sift_restated as sr

    frames = cr.sequence()
    assert len(frames) == 2 and frames[0].shape == (96, 128, 3) and frames[0].dtype == np.uint8
    model = _matcher(frames, tmp_path, optimize.CLAHE(clipLimit=2.0))
    model.build_keypoints(method=optimize.SIFT)
    for frame, (keypoints, descriptors) in zip(frames, model.keypoints):
        gray = frame.mean(axis=2).astype(np.uint8)
        equalised = cr.apply(gray, 2.0, (8, 8))[0]
        want_k, want_d = optimize.detect_keypoints(equalised, method=optimize.SIFT)
        plain_k, _ = optimize.detect_keypoints(gray, method=optimize.SIFT)
        print(len(keypoints), "keypoints; on the restated CLAHE", len(want_k), "; without CLAHE", len(plain_k))
        assert keypoints == want_k and len(keypoints) >= 20 and len(keypoints) >= len(plain_k) + 1
        same_bytes(descriptors, want_d, "descriptors")
        restated_k, restated_d = sr.detect(equalised)
        found = np.array([[k.pt[0], k.pt[1], k.size, k.angle, k.response, k.octave] for k in keypoints], np.float64)
        assert np.array_equal(found.view(np.uint64), restated_k.view(np.uint64))
        same_bytes(descriptors, restated_d, "descriptors against the restated SIFT")
