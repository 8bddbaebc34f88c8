"""`Image.orthorectify` / `Observer.orthorectify` on the device, through the Python API and so through the C ABI
(`glh_stage_orthorectify`, kernel `k_orthorectify`), against the restatement of the rule in tests/ortho_rule.py (NumPy and
scipy's RegularGridInterpolator only).  The scenes and why they are what they are: tests/ortho_scene.py; that the
agreement scene meets the conditions of the exact comparisons is checked without a device in tests/test_orthorectify.py
and again here, on the cells that are compared.

Where the numbers come from (none of them was fitted to the kernel):

* NaN pattern and "nearest" picks: exact.  Both are decided by comparisons of uv with the frame's edges, the
  pixel-centre lines and the pixel boundaries; no restated uv of a seen cell lies within 1e-9 px of one (asserted), and
  the device's uv agree with the restated ones far below that (measured below).
* "linear" values: PROJECTION_DEVIATION is the largest |uv difference| between the existing projection stage
  (`_lib.stage_project`, what `Camera.xyz_to_uv` runs) and the NumPy restatement of `Camera.xyz_to_uv` on this scene's
  cells that land on the pixel centres' grid -- the existing projection stage against NumPy, not the new kernel; the
  cells far outside the frame are left out, which only narrows the bound.  A coordinate error d moves a bilinear value
  by at most d x (the largest difference between neighbouring pixels) per axis; a factor of 4 covers the two axes and
  the two roundings of the blend.  Where the measured deviation is exactly zero the values must equal bit for bit.
"""
import numpy as np
import pytest

from tests import ortho_rule, ortho_scene

pytestmark = pytest.mark.gpu

# (the three-channel cases of the wider types are there for the kernel's instantiations, one per type and channel count)
CASES = [(np.uint8, 1), (np.uint8, 3), (np.uint16, 1), (np.float32, 1), (np.float64, 1), (np.uint16, 3), (np.float32, 3),
         (np.float64, 3)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def neighbour_step(frame):
    f = frame.astype(np.float64)
    return max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())


@pytest.fixture(scope="module")
def scene():
    """The agreement scene with what its cases share, computed once: the viewshed from the existing stage, and the
    deviation of the existing projection stage from the NumPy restatement on the scene's cells."""
    from glimpse_amd import _lib

    cam, dem = ortho_scene.objects()
    visible = dem.viewshed(cam.xyz, correction=cam.correction)
    X, Y = np.meshgrid(dem.x, dem.y)
    xyz = np.column_stack((X.ravel(), Y.ravel(), dem.array.ravel()))
    device_uv, numpy_uv = _lib.stage_project(cam.vector24, xyz), ortho_rule.xyz_to_uv(cam, xyz)
    assert (np.isnan(device_uv) == np.isnan(numpy_uv)).all()
    # over the cells whose restated uv lies on the pixel centres' grid, where a value can come from (masked and hidden
    # ones included): the cells far outside the frame, next to the camera's plane, have uv of 1e4 px and more and
    # deviate accordingly (printed, not used: they would only widen the bound)
    with np.errstate(invalid="ignore"):
        inside = ((numpy_uv >= 0.5) & (numpy_uv <= np.array([ortho_scene.FW, ortho_scene.FH]) - 0.5)).all(axis=1)
    deviation = float(np.abs(device_uv - numpy_uv)[inside].max())
    print(f"projection stage against NumPy: max |uv difference| {deviation:.3e} px on the {int(inside.sum())} cells on the "
          f"pixel centres' grid, {float(np.nanmax(np.abs(device_uv - numpy_uv))):.3e} px on all {len(xyz)} cells")
    return {"cam": cam, "dem": dem, "mask": ortho_scene.mask(), "visible": visible, "deviation": deviation}


def test_closed_form_scene_returns_the_frame():
    """The nadir scene: every cell centre lands on a pixel centre, so the orthophoto is the frame, orientation included
    (ortho_scene.closed_form: why this holds bit for bit under "linear" too)."""
    from glimpse_amd import Camera, Raster

    args, frame, x, y, z = ortho_scene.closed_form()
    img = ortho_scene.image(frame, Camera(**args))
    for method in ("linear", "nearest"):
        got = img.orthorectify(Raster(z, x=x, y=y), method=method)
        assert got.shape == (3, 3, 1) and got.dtype == np.float64
        assert same_bits(np.ascontiguousarray(got[:, :, 0]), frame), method


@pytest.mark.parametrize("method", ["linear", "nearest"])
@pytest.mark.parametrize("dtype,channels", CASES, ids=lambda v: getattr(v, "__name__", str(v)))
def test_agreement_with_the_rule(scene, dtype, channels, method):
    cam, dem = scene["cam"], scene["dem"]
    frame = ortho_scene.frame(dtype, channels)
    want, uv, seen = ortho_rule.orthorectify(cam, frame, dem.x, dem.y, dem.array, mask=scene["mask"],
                                             viewshed=scene["visible"], method=method)
    got = ortho_scene.image(frame, cam).orthorectify(dem, viewshed=True, mask=scene["mask"], method=method)
    assert got.shape == (ortho_scene.NY, ortho_scene.NX, channels) == want.shape
    assert got.dtype == want.dtype == (np.float32 if dtype == np.float32 else np.float64)
    # the scene: the exact comparisons below rest on no seen cell sitting on a decision, and every kind of cell is there
    assert ortho_rule.fragile_cells(uv, seen, (ortho_scene.FW, ortho_scene.FH), method) == 0
    valued = ~np.isnan(want).any(axis=2)
    hidden = ~scene["visible"] & ~np.isnan(uv).any(axis=2) & ortho_rule.inframe(cam, uv.reshape(-1, 2)).reshape(seen.shape)
    assert valued.sum() > 100 and (seen & ~valued).sum() >= 3 and hidden.sum() > 50 and not seen[ortho_scene.MASK_BLOCK].any()
    # NaN pattern: exactly the restatement's, all channels of a cell alike
    assert (np.isnan(got) == np.isnan(want)).all()
    assert (np.isnan(want).all(axis=2) == ~valued).all()
    diff = np.abs(got[valued].astype(np.float64) - want[valued].astype(np.float64))
    bound = 4.0 * scene["deviation"] * neighbour_step(frame)
    print(f"{np.dtype(dtype).name} x {channels} {method}: {int(valued.sum())} valued cells of {valued.size}, "
          f"{int((seen & ~valued).sum())} within half a pixel of the edge, {int(hidden.sum())} hidden; max |diff| "
          f"{diff.max():.3e}, bound {bound:.3e} (projection deviation {scene['deviation']:.3e} px, neighbour step "
          f"{neighbour_step(frame):.6g}), bit-equal {same_bits(got, want)}")
    if method == "nearest" or scene["deviation"] == 0.0:
        assert same_bits(got, want)
    else:
        # Measured on an MI355X: the projection deviates by 1.066e-14 px (not zero, so no bit equality is asked), which
        # makes the bound 1.5e-12 for uint8 (neighbour step 36 / 37), 4.0e-10 for uint16 (step 9304 / 9570) and 6.1e-12
        # for float32 / float64 (step 142 / 146); the differences found were 2.6e-13, 6.5e-11, 0 (float32) and 1.0e-12.
        assert (diff <= bound).all()


def test_ascending_y_gives_the_row_flipped_result(scene):
    """The same DEM stored bottom row first: the cells are the same points, so the result is the other one's rows in
    reverse, bit for bit (viewshed and mask included)."""
    frame = ortho_scene.frame(np.uint8, 3)
    cam, up = ortho_scene.objects(ascending_y=True)
    assert up.y[0] < up.y[-1] and same_bits(np.ascontiguousarray(up.array[::-1]), np.ascontiguousarray(scene["dem"].array))
    for method in ("linear", "nearest"):
        down = ortho_scene.image(frame, scene["cam"]).orthorectify(scene["dem"], viewshed=True, mask=scene["mask"], method=method)
        flipped = ortho_scene.image(frame, cam).orthorectify(up, viewshed=True, mask=scene["mask"][::-1], method=method)
        assert same_bits(np.ascontiguousarray(flipped[::-1]), down), method
        assert not same_bits(flipped, down)


def test_float32_and_integer_elevations_are_widened_exactly(scene):
    """A float32 DEM goes to the device as it is and is widened there, an integer DEM is widened on the host: both give
    what the float64 copy of the same elevations gives, bit for bit (`xyz_to_uv` makes float64 of a cell either way)."""
    from glimpse_amd import Raster

    frame = ortho_scene.frame(np.uint16, 3)
    img, dem = ortho_scene.image(frame, scene["cam"]), scene["dem"]
    with np.errstate(invalid="ignore"):
        coarse = np.where(np.isnan(dem.array), 0.0, np.round(dem.array)).astype(np.int16)
    for array in (dem.array.astype(np.float32), coarse):
        narrow, wide = Raster(array, x=dem.x, y=dem.y), Raster(array.astype(np.float64), x=dem.x, y=dem.y)
        got = img.orthorectify(narrow, viewshed=scene["visible"], mask=scene["mask"])
        assert same_bits(got, img.orthorectify(wide, viewshed=scene["visible"], mask=scene["mask"]))
        assert (~np.isnan(got)).sum() > 300 and not same_bits(got, img.orthorectify(dem, viewshed=scene["visible"], mask=scene["mask"]))


def test_observer_orthorectify_equals_the_per_image_calls_with_one_viewshed(scene, monkeypatch):
    from glimpse_amd import Observer, _lib

    calls = []
    stage_viewshed = _lib.stage_viewshed

    def counted(*args, **kwargs):
        calls.append(1)
        return stage_viewshed(*args, **kwargs)

    for dtype, channels, method in ((np.uint8, 3, "linear"), (np.float32, 1, "nearest")):
        images = [ortho_scene.image(ortho_scene.frame(dtype, channels, seed=i), ortho_scene.objects(viewdir)[0], day=i)
                  for i, viewdir in enumerate(ortho_scene.VIEWDIRS)]
        singles = [img.orthorectify(scene["dem"], viewshed=True, mask=scene["mask"], method=method) for img in images]
        monkeypatch.setattr(_lib, "stage_viewshed", counted)
        del calls[:]
        batch = Observer(images).orthorectify(scene["dem"], viewshed=True, mask=scene["mask"], method=method)
        monkeypatch.setattr(_lib, "stage_viewshed", stage_viewshed)
        assert len(calls) == 1  # (three images, one position: one viewshed)
        assert batch.shape == (3, ortho_scene.NY, ortho_scene.NX, channels)
        for i, one in enumerate(singles):
            assert same_bits(np.ascontiguousarray(batch[i]), one), i
        assert not same_bits(np.ascontiguousarray(batch[0]), np.ascontiguousarray(batch[1]))
        picked = Observer(images).orthorectify(scene["dem"], index=[2, 0], viewshed=scene["visible"], mask=scene["mask"],
                                               method=method)
        assert same_bits(np.ascontiguousarray(picked[0]), singles[2]) and same_bits(np.ascontiguousarray(picked[1]), singles[0])


def test_a_camera_that_sees_no_cell_gives_all_nan(scene):
    cam = ortho_scene.objects(viewdir=(4.0, 60.0, 3.0))[0]  # looking up: every cell is behind it or out of the frame
    for dtype, channels in ((np.uint8, 3), (np.float32, 1)):
        got = ortho_scene.image(ortho_scene.frame(dtype, channels), cam).orthorectify(scene["dem"], viewshed=True)
        assert got.shape == (ortho_scene.NY, ortho_scene.NX, channels) and np.isnan(got).all()
