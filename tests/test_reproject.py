"""`Image.project` / `Observer.project` without a device: the argument checks come before the library is touched, and
the committed g27 fixture is what the reference writes (regenerated when the reference is on this machine)."""
import datetime
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = datetime.datetime(2020, 1, 1)


def _images(n=3, xyz=(1.0, 2.0, 3.0)):
    from glimpse_amd import Camera, Image

    frame = np.arange(6 * 8, dtype=np.uint8).reshape(6, 8)
    return [Image(cam=Camera(imgsz=(8, 6), f=10, xyz=xyz, viewdir=(i, 0, 0)), array=frame,
                  datetime=T0 + datetime.timedelta(days=i)) for i in range(n)]


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so a ValueError below was raised before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def test_image_project_refuses_another_position_before_the_library(no_library):
    img = _images(1)[0]
    cam = img.cam.copy()
    cam.xyz = (1.0, 2.0, 3.5)
    with pytest.raises(ValueError) as e:
        img.project(cam)
    assert str(e.value) == "Source and target cameras have different positions ('xyz')"
    with pytest.raises(ValueError):
        img.project(cam, method="nearest")


def test_image_project_refuses_an_unknown_method_before_the_library(no_library):
    img = _images(1)[0]
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        img.project(img.cam.copy(), method="cubic")


def test_observer_project_refuses_another_position_and_names_the_image(no_library):
    from glimpse_amd import Observer

    images = _images(3)
    images[2].cam.xyz = (1.0, 2.0, 3.5)
    obs = Observer(images)
    with pytest.raises(ValueError) as e:
        obs.project(images[0].cam.copy())
    assert "cameras have different positions ('xyz')" in str(e.value) and "image 2" in str(e.value)
    with pytest.raises(ValueError, match="image 2"):
        obs.project(images[0].cam.copy(), index=[2, 0])
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        obs.project(images[0].cam.copy(), index=slice(0, 2), method="cubic")


def test_stage_reproject_checks_its_arguments_before_the_library(no_library):
    from glimpse_amd import _lib

    cams = np.zeros((1, _lib.CAM_LEN))
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        _lib.stage_reproject(np.zeros((1, 4, 4, 1), np.uint8), cams, cams[0], (4, 4), "cubic")
    with pytest.raises(TypeError, match="int32"):
        _lib.stage_reproject(np.zeros((1, 4, 4, 1), np.int32), cams, cams[0], (4, 4))


def test_g27_is_what_the_reference_writes(tmp_path, golden):
    """tools/make_golden.py --g27 run again (in a process of its own: it installs stub modules) gives the committed arrays
    bit for bit.  Needs the reference; elsewhere the fixture is taken as committed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import refstubs  # (importing installs nothing; it knows where the reference would be)
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(refstubs.REFERENCE_SRC, "glimpse")):
        pytest.skip("the reference is not on this machine")
    out = tmp_path / "g27.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden.py"), "--g27", "--out", str(out)], check=True,
                   capture_output=True, timeout=600)
    want, got = golden("g27_reproject.npz"), dict(np.load(out, allow_pickle=False))
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key].dtype == got[key].dtype and want[key].shape == got[key].shape, key
        assert want[key].tobytes() == got[key].tobytes(), key


def test_g27_covers_what_it_says(golden):
    g = golden("g27_reproject.npz")
    runs = [str(k).split("__") for k in g["runs"]]
    assert {r[1] for r in runs} == {"uint8", "uint16", "float32", "float64"}
    assert {r[2] for r in runs} == {"1", "3"} and {r[3] for r in runs} == {"linear", "nearest"}
    assert {r[0] for r in runs} == {str(c) for c in g["cases"]} and len(g["cases"]) == 6
    for name, dtype, ch, method in runs:
        out, dst = g["__".join((name, dtype, ch, method))], g[name + "__dst_cam"]
        assert out.dtype == np.dtype(dtype) and out.shape == (int(dst[7]), int(dst[6]), int(ch))
        if out.dtype.kind == "u":
            assert g["__".join((name, dtype, ch, method, "fill"))].shape == out.shape[:2]
    fill = {str(c): float(np.isnan(g[str(c) + "__uv"]).any(axis=1).mean()) for c in g["cases"]}
    assert fill["away"] == 1.0
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g27_reproject.npz")) < 1_000_000


def test_the_library_refuses_what_it_does_not_resample():
    """glh_stage_reproject checks its arguments before it touches a device: raster grids as cameras, unknown methods and
    types, cameras at different positions, sizes that contradict the cameras."""
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    cam = np.zeros(_lib.CAM_LEN)
    cam[0:3], cam[6:8], cam[8:10] = (1, 2, 3), (8, 6), (10, 10)
    frame, out = np.zeros((6, 8, 1), np.uint8), np.zeros((6, 8, 1), np.uint8)

    def call(src=cam, dst=cam, bits=8, is_float=0, channels=1, method=0, dst_size=(8, 6)):
        return lib.glh_stage_reproject(0, _lib._ptr(frame), bits, is_float, 8, 6, channels, 1, _lib._ptr(np.ascontiguousarray(src)),
                                       _lib._ptr(np.ascontiguousarray(dst)), dst_size[0], dst_size[1], method, _lib._ptr(out), None)

    UNSUPPORTED, INVALID = -5, -1
    grid = cam.copy()
    grid[23] = 1.0
    assert call(src=grid) == UNSUPPORTED and "raster" in lib.glh_last_error().decode()
    assert call(dst=grid) == UNSUPPORTED
    assert call(method=2) == UNSUPPORTED
    assert call(bits=32, is_float=0) == UNSUPPORTED and call(bits=16, is_float=1) == UNSUPPORTED
    assert call(channels=2) == UNSUPPORTED
    moved = cam.copy()
    moved[2] = 3.5
    assert call(dst=moved) == INVALID and "positions ('xyz')" in lib.glh_last_error().decode()
    assert call(dst_size=(8, 7)) == INVALID
