"""optimize.CLAHE without a device: the restatement of INPUTS.md's "CLAHE: the rule" (tests/clahe_restated.py) against
itself and against NumPy where NumPy says the same thing, the case table's reach, the object's surface and the C ABI's new
symbol.  The device's results are compared in tests/test_gpu_clahe.py."""
import copy
import datetime
import os
import pickle
import re

import numpy as np
import pytest

from tests import clahe_restated as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [name for name in cr.CASES if name != "large-2x2"]


@pytest.mark.parametrize("name", list(cr.CASES))
def test_closed_form_equals_the_residual_loop(name):
    _, _, clip, grid, _ = cr.CASES[name]
    by_loop = cr.luts(cr.frame(name), clip, grid, redistribute=cr.redistribute_loop)
    assert np.array_equal(by_loop, cr.expected(name)[1])


def test_closed_form_equals_the_residual_loop_on_every_residual():
    """Every residual 0 .. 255 and both sides of step == 1 (residual > 128), on histograms made for it."""
    rng = np.random.default_rng(3)
    for residual in range(256):
        lim = 5
        hist = rng.integers(0, lim + 1, 256)
        hist[int(rng.integers(0, 256))] = lim + 256 * 2 + residual  # clipped = 512 + residual
        a, ra, sa = cr.redistribute_loop(hist, lim)
        b, rb, sb = cr.redistribute_closed(hist, lim)
        assert ra == rb == residual and sa == sb and np.array_equal(a, b)
        assert a.sum() == hist.sum()


def test_the_cases_reach_every_branch():
    """What the issue lists of each case, and that the table as a whole keeps a residual, a step of 1 and padding."""
    reach = {name: cr.expected(name)[2] for name in cr.CASES}
    assert not reach["divisible"]["padded"] and reach["padded-odd"]["padded"]
    t = reach["grid3x5-clip2"]
    assert all(c > 0 for c in t["clipped"]) and len(t["clipped"]) == 15 and sum(s == 1 for s in t["step"]) >= 1
    assert reach["noclip-rows-padded"]["lim"] == 0 and reach["noclip-rows-padded"]["padded"]
    assert cr.geometry(33, 40, (4, 4)) == (36, 44, 9, 11)  # three rows and a whole grid of columns
    assert reach["one-tile-lim1"]["lim"] == 1
    assert cr.geometry(9, 11, (8, 8))[2:] == (2, 2)
    assert all(c > 0 for c in reach["slices-clip3"]["clipped"]) and len(reach["slices-clip3"]["clipped"]) == 64
    assert np.array_equal(cr.expected("constant255")[0], cr.frame("constant255"))
    assert cr.geometry(1024, 1536, (2, 2))[2:] == (512, 768)
    assert set(np.unique(cr.frame("stripes"))) == {0, 255}
    assert any(r != 0 for t in reach.values() for r in t["residual"])
    assert any(s == 1 for t in reach.values() for s in t["step"])
    assert any(t["padded"] for t in reach.values())


def test_reflection_is_np_pad():
    for h, w, grid in [(47, 61, (8, 8)), (33, 40, (4, 4)), (9, 11, (8, 8)), (9, 4, (4, 2)), (5, 7, (7, 4)), (4, 6, (6, 3)),
                       (2, 3, (2, 2)), (3, 1, (1, 2)), (1, 5, (2, 1))]:
        src = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w)).astype(np.uint8)
        ext_h, ext_w, _, _ = cr.geometry(h, w, grid)
        assert (ext_h, ext_w) != (h, w)
        assert np.array_equal(cr.extend(src, grid), np.pad(src, ((0, ext_h - h), (0, ext_w - w)), mode="reflect")), (h, w, grid)
    src = cr.frame("divisible")
    assert cr.extend(src, (8, 8)) is not src and np.array_equal(cr.extend(src, (8, 8)), src)
    for n in (2, 3, 7, 100):  # the closed form, for every index that at most n added cells reach
        i = np.arange(2 * n)
        assert np.array_equal(cr.reflect(i, n), np.pad(np.arange(n), (0, n), mode="reflect"))


def test_channel_mean_is_the_float_mean_truncated():
    for c in (1, 2, 3, 4):
        sums = np.arange(255 * c + 1)  # every sum c channels can have
        a = np.zeros((len(sums), 1, c), np.int64)
        for k in range(c):
            a[:, 0, k] = np.clip(sums - 255 * k, 0, 255)
        a = a.astype(np.uint8)
        assert np.array_equal(a.astype(np.int64).sum(axis=2)[:, 0], sums)
        assert np.array_equal(cr.channel_mean(a), a.mean(axis=2).astype(np.uint8))
        rnd = cr.colour(47, 61, c)
        assert np.array_equal(cr.channel_mean(rnd), rnd.mean(axis=2).astype(np.uint8))


def test_blend_of_equal_tables_is_the_table():
    """With the same table in every tile the weights sum to one in float32 only nearly; the result still rounds to the
    table's value (what makes a constant image come out as it went in)."""
    src = cr.frame("padded-odd")
    L = np.broadcast_to(np.arange(256, dtype=np.uint8)[::-1], (8, 8, 256)).copy()
    assert np.array_equal(cr.blend(src, L, (8, 8)), 255 - src)


def test_object_surface():
    from glimpse_amd import optimize

    c = optimize.CLAHE()
    assert c.getClipLimit() == 40.0 and c.getTilesGridSize() == (8, 8) and c.device_id == 0
    c = optimize.createCLAHE(clipLimit=2, tileGridSize=[3, 5])
    assert type(c) is optimize.CLAHE and c.getClipLimit() == 2.0 and type(c.getClipLimit()) is float
    assert c.getTilesGridSize() == (3, 5)
    c.setClipLimit(3.5)
    c.setTilesGridSize((4, 2))
    assert (c.getClipLimit(), c.getTilesGridSize()) == (3.5, (4, 2))
    assert c.collectGarbage() is None
    for again in (pickle.loads(pickle.dumps(c)), copy.deepcopy(c), copy.copy(c)):
        assert again is not c and vars(again) == vars(c) == dict(clipLimit=3.5, tileGridSize=(4, 2), device_id=0)
    for bad in ((0, 8), (8,), (8, 8, 8), (2.5, 8), (8, -1)):
        with pytest.raises(ValueError, match="tileGridSize"):
            c.setTilesGridSize(bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            c.setClipLimit(bad)
    assert (c.getClipLimit(), c.getTilesGridSize()) == (3.5, (4, 2))


def test_apply_refuses_before_a_device_is_touched(monkeypatch):
    from glimpse_amd import _lib, optimize

    def no_device(*a, **k):
        raise AssertionError("the stage was called")

    monkeypatch.setattr(_lib, "stage_clahe", no_device)
    c = optimize.CLAHE()
    for bad in (np.zeros((16, 16), np.uint16), np.zeros((16, 16), np.float32), [[1, 2], [3, 4]]):
        with pytest.raises(TypeError, match="two-dimensional uint8"):
            c.apply(bad)
    for bad in (np.zeros((16, 16, 3), np.uint8), np.zeros(16, np.uint8), np.zeros((0, 16), np.uint8)):
        with pytest.raises(ValueError, match="two-dimensional uint8"):
            c.apply(bad)
    with pytest.raises(ValueError, match="larger than the image"):
        c.apply(np.zeros((16, 7), np.uint8))
    with pytest.raises(ValueError, match="larger than the image"):
        optimize.CLAHE(tileGridSize=(2, 9)).apply(np.zeros((8, 16), np.uint8))


class _Image:
    def __init__(self, day):
        self.datetime = datetime.datetime(2020, 1, day)
        self.path = f"img_{day}.png"


def test_matcher_stores_a_clahe_and_refuses_cv2s():
    from glimpse_amd import optimize

    images = [_Image(1), _Image(2)]
    assert optimize.KeypointMatcher(images).clahe is None
    assert optimize.KeypointMatcher(images, clahe=False).clahe is None
    c = optimize.CLAHE(clipLimit=2.0)
    assert optimize.KeypointMatcher(images, clahe=c).clahe is c
    for refused in (True, {}, {"clipLimit": 2.0}, 1, None, "clahe"):
        with pytest.raises(NotImplementedError, match="CLAHE") as e:
            optimize.KeypointMatcher(images, clahe=refused)
        assert "optimize.CLAHE" in str(e.value) and "clahe=False" in str(e.value)


def test_prepare_image_routes(monkeypatch):
    """uint8 of up to four channels goes to the stage with its channels; anything else takes the host mean, then apply;
    without a CLAHE nothing changes."""
    from glimpse_amd import _lib, optimize

    calls = []

    def stage(array, clip_limit, tile_grid_size, device_id=0, **kw):
        calls.append((array.shape, array.dtype, clip_limit, tile_grid_size, device_id))
        return np.zeros(array.shape[:2], np.uint8)

    monkeypatch.setattr(_lib, "stage_clahe", stage)
    images = [_Image(1), _Image(2)]
    plain = optimize.KeypointMatcher(images)
    rgb = cr.colour(16, 24, 3)
    assert np.array_equal(plain._prepare_image(rgb), rgb.mean(axis=2).astype(np.uint8)) and not calls
    gray = rgb[:, :, 0]
    assert plain._prepare_image(gray) is gray
    model = optimize.KeypointMatcher(images, clahe=optimize.CLAHE(clipLimit=2.0, tileGridSize=(4, 2), device_id=0))
    for array, seen in ((rgb, (16, 24, 3)), (gray, (16, 24)), (cr.colour(16, 24, 4), (16, 24, 4)),
                        (cr.colour(16, 24, 5), (16, 24)), (rgb.astype(np.float64), (16, 24)), (rgb.astype(np.uint16), (16, 24))):
        del calls[:]
        out = model._prepare_image(array)
        assert out.shape == (16, 24) and out.dtype == np.uint8
        assert calls == [(seen, np.dtype(np.uint8), 2.0, (4, 2), 0)], (array.shape, array.dtype, calls)


def test_header_and_binding_hold_the_symbol():
    from glimpse_amd import _lib, build

    header = open(os.path.join(ROOT, "include", "glimpse_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+glh_stage_clahe\s*\(([^)]*)\)", code)
    assert m, "include/glimpse_hip.h does not declare glh_stage_clahe"
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = _lib.SIGNATURES["glh_stage_clahe"]
    assert len(params) == len(args) == 11
    import ctypes as C
    for p, a in zip(params, args):
        assert a is (C.c_void_p if "*" in p else C.c_double if p.startswith("double") else C.c_int), (p, a)
    assert "glh_clahe.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "glh_clahe.hip"))
    build.build(verbose=False)
    assert hasattr(_lib.load(), "glh_stage_clahe")


def test_library_host_arithmetic_equals_the_restatement():
    """Steps 1 and 2 as the library's host code computes them (glh_clahe.h, compiled for the CPU): every grid on a few
    sizes, and clip limits from none to one no bin can reach (where the library stops at `area`: nothing is clipped either
    way, which the last lines check on the restatement)."""
    import ctypes as C
    import subprocess

    src = os.path.join(ROOT, "tests", "hostcheck", "clahe_hostcheck.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libclahe_hostcheck.so")
    deps = [src, os.path.join(ROOT, "glimpse_amd", "csrc", "glh_clahe.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.cl_geometry.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_void_p]
    got = np.zeros(6, np.int64)
    for h, w in ((1, 1), (9, 11), (33, 40), (47, 61), (48, 64)):
        for tiles_x in range(1, w + 1):
            for tiles_y in range(1, h + 1):
                ext_h, ext_w, th, tw = cr.geometry(h, w, (tiles_x, tiles_y))
                for clip in (-1.0, 0.0, 0.001, 2.0, 3.0, 40.0, 255.9, 256.0, 1e6, 1e300):
                    lib.cl_geometry(w, h, clip, tiles_x, tiles_y, got.ctypes.data_as(C.c_void_p))
                    lim = cr.clip_limit(clip, tw * th)
                    assert got.tolist() == [ext_w, ext_h, tw, th, tw * th, min(lim, tw * th)], (h, w, tiles_x, tiles_y, clip)
    lib.cl_geometry(46340, 46340, 40.0, 1, 1, got.ctypes.data_as(C.c_void_p))  # the largest square below 2^31 pixels
    assert got.tolist() == [46340, 46340, 46340, 46340, 46340 ** 2, cr.clip_limit(40.0, 46340 ** 2)]
    frame = cr.frame("padded-odd")
    area = 6 * 8
    assert np.array_equal(cr.luts(frame, 256.0, (8, 8)), cr.luts(frame, 1e15, (8, 8)))  # lim = area and lim > area
    assert cr.clip_limit(256.0, area) == area and np.array_equal(cr.luts(frame, 256.0, (8, 8)), cr.luts(frame, 0.0, (8, 8)))


def test_sequence_needs_clahe_for_its_keypoints():
    """The end-to-end frames of tests/test_gpu_clahe.py: the restated SIFT finds at least 20 keypoints on the restated
    CLAHE of each and fewer without it, so a matcher that skipped CLAHE could not pass there."""
    from tests import sift_restated as sr

    for frame in cr.sequence():
        gray = cr.channel_mean(frame)
        assert np.array_equal(gray, frame.mean(axis=2).astype(np.uint8))
        with_clahe, _ = sr.detect(cr.apply(gray, 2.0, (8, 8))[0])
        without, _ = sr.detect(gray)
        n_without = 0 if without is None else len(without)
        print(len(with_clahe), "keypoints with CLAHE,", n_without, "without")
        assert len(with_clahe) >= 20 and len(with_clahe) >= n_without + 1
