"""`Image.orthorectify` / `Observer.orthorectify` without a device: the argument checks come before any library call, the
restatement of the rule (tests/ortho_rule.py) returns the frame on the closed-form scene, and the agreement scene of
tests/test_gpu_orthorectify.py meets the conditions its exact comparisons rest on."""
import numpy as np
import pytest

from tests import ortho_rule
from tests import ortho_scene


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Neither the new stage nor the viewshed stage may be reached, and any attempt to load the HIP library fails
    (GlhError): a ValueError below was raised before all of them."""
    from glimpse_amd import _lib

    def reached(*args, **kwargs):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_lib, "stage_orthorectify", reached)
    monkeypatch.setattr(_lib, "stage_viewshed", reached)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def scene_image(day=0):
    cam, dem = ortho_scene.objects()
    return ortho_scene.image(ortho_scene.frame(np.uint8, 3), cam, day), dem


def test_unknown_method_is_refused_before_the_library(no_library):
    img, dem = scene_image()
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        img.orthorectify(dem, method="cubic")
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        img.orthorectify(dem, viewshed=True, method="cubic")


def test_mask_and_viewshed_of_another_shape_are_refused_before_the_library(no_library):
    img, dem = scene_image()
    wrong = np.ones((ortho_scene.NX, ortho_scene.NY), dtype=bool)  # (transposed)
    with pytest.raises(ValueError, match="mask does not have the same 2-d shape as dem"):
        img.orthorectify(dem, mask=wrong)
    with pytest.raises(ValueError, match="viewshed does not have the same 2-d shape as dem"):
        img.orthorectify(dem, viewshed=wrong)
    with pytest.raises(ValueError, match="mask does not have the same 2-d shape as dem"):
        img.orthorectify(dem, viewshed=True, mask=wrong[:, :5])


def test_a_dem_that_is_not_two_dimensional_is_refused_before_the_library(no_library):
    from glimpse_amd import Raster

    img, dem = scene_image()
    layered = Raster(np.zeros((ortho_scene.NY, ortho_scene.NX, 2)), x=dem.x, y=dem.y)
    with pytest.raises(ValueError, match="a DEM is two-dimensional"):
        img.orthorectify(layered)
    with pytest.raises(ValueError, match="a DEM is two-dimensional"):
        img.orthorectify(layered, viewshed=True)


def test_a_raster_grid_as_camera_is_refused_before_the_library(no_library):
    from glimpse_amd import Image, Raster

    _, dem = scene_image()
    grid = Raster(np.zeros((ortho_scene.FH, ortho_scene.FW)), x=(0.0, 48.0), y=(40.0, 0.0))
    img = Image(cam=grid, array=ortho_scene.frame(np.uint8, 1), datetime=ortho_scene.T0)
    with pytest.raises(ValueError, match="raster grid, which has no position to see from"):
        img.orthorectify(dem)


def test_observer_orthorectify_checks_every_image_and_names_it(no_library):
    from glimpse_amd import Observer, Raster

    images = [scene_image(day)[0] for day in range(3)]
    dem = scene_image()[1]
    images[2].cam = Raster(np.zeros((ortho_scene.FH, ortho_scene.FW)), x=(0.0, 48.0), y=(40.0, 0.0))
    obs = Observer(images)
    with pytest.raises(ValueError, match="Image 2's camera is a raster grid"):
        obs.orthorectify(dem)
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        obs.orthorectify(dem, index=[0, 1], method="cubic")
    with pytest.raises(ValueError, match="mask does not have the same 2-d shape as dem"):
        obs.orthorectify(dem, index=slice(0, 2), mask=np.ones((3, 3), dtype=bool))
    with pytest.raises(ValueError, match="No images selected"):
        obs.orthorectify(dem, index=[])


def test_stage_orthorectify_checks_its_arguments_before_the_library(monkeypatch, tmp_path):
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    cams = np.zeros((1, _lib.CAM_LEN))
    z, x, y = np.zeros((3, 4)), np.arange(4.0), np.arange(3.0)
    frames = np.zeros((1, 4, 4, 1), np.uint8)
    with pytest.raises(ValueError, match="Method 'cubic' is not defined"):
        _lib.stage_orthorectify(frames, cams, z, x, y, method="cubic")
    with pytest.raises(TypeError):
        _lib.stage_orthorectify(frames.astype(np.int32), cams, z, x, y)
    with pytest.raises(ValueError):
        _lib.stage_orthorectify(frames, cams, z, x, y, seen=np.ones((1, 4, 3), np.uint8))
    with pytest.raises(ValueError):
        _lib.stage_orthorectify(frames, cams, z, x[:3], y)
    with pytest.raises(_lib.GlhError):  # (every argument in order: only now is the library asked for)
        _lib.stage_orthorectify(frames, cams, z, x, y)


def test_the_c_abi_checks_its_arguments_before_a_device():
    """glh_stage_orthorectify refuses raster grids as cameras, unknown methods, types and channel counts, and sizes
    that do not fit, without touching a device (this machine has none)."""
    from glimpse_amd import _lib

    lib = _lib.load()
    cam, dem = ortho_scene.objects()
    frame = np.ascontiguousarray(ortho_scene.frame(np.uint8, 3))
    z, x, y = np.ascontiguousarray(dem.array), np.ascontiguousarray(dem.x), np.ascontiguousarray(dem.y)
    out = np.empty((ortho_scene.NY, ortho_scene.NX, 3))

    def call(cams=cam.vector24, bits=8, is_float=0, w=ortho_scene.FW, h=ortho_scene.FH, channels=3, method=0, z_dtype=0,
             nx=ortho_scene.NX, seen=None, n_seen=0, seen_of=None):
        cams = np.ascontiguousarray(cams)
        return lib.glh_stage_orthorectify(0, _lib._ptr(frame), bits, is_float, w, h, channels, 1, _lib._ptr(cams), _lib._ptr(z),
                                          z_dtype, nx, ortho_scene.NY, _lib._ptr(x), _lib._ptr(y), _lib._ptr(seen), n_seen,
                                          _lib._ptr(seen_of), method, _lib._ptr(out), None)

    grid = cam.vector24.copy()
    grid[23] = 1.0
    one = np.ones((1, ortho_scene.NY, ortho_scene.NX), np.uint8)
    for rc in (call(cams=grid), call(method=2), call(bits=32, is_float=0), call(channels=2), call(z_dtype=2)):
        assert rc == -5, rc  # GLH_E_UNSUPPORTED
    for rc in (call(w=ortho_scene.FW + 1), call(w=1), call(nx=0), call(seen=one, n_seen=0),
               call(seen_of=np.zeros(1, np.int32)), call(seen=one, n_seen=1, seen_of=np.ones(1, np.int32))):
        assert rc == -1, rc  # GLH_E_INVALID
    assert b"orthorectify" in lib.glh_last_error()


def test_the_restatement_returns_the_frame_on_the_closed_form_scene():
    """Every cell centre of the nadir scene lands on a pixel centre, so the rule returns the frame itself, orientation
    included: top row of the DEM (y = 1) is the top row of the frame, first column (x = -1) its first column."""
    from glimpse_amd import Camera

    args, frame, x, y, z = ortho_scene.closed_form()
    cam = Camera(**args)
    assert len(set(frame.ravel())) == 9 and 8.0 < frame.min() and frame.max() < 12.0  # (ortho_scene: why this range)
    for method in ("linear", "nearest"):
        got, uv, seen = ortho_rule.orthorectify(cam, frame, x, y, z, method=method)
        assert seen.all() and got.shape == (3, 3, 1) and got.dtype == np.float64
        assert np.abs(uv - np.stack(np.meshgrid([0.5, 1.5, 2.5], [0.5, 1.5, 2.5]), axis=2)).max() <= 2.0 ** -52
        assert got[:, :, 0].tobytes() == frame.tobytes(), method
    # the orientation is not an accident of a symmetric frame: a transposed or flipped frame is another answer
    assert not (frame == frame.T).all() and not (frame == frame[::-1]).all() and not (frame == frame[:, ::-1]).all()


def test_the_restatement_keeps_the_rule_of_unseen_cells():
    """NaN elevation, a masked cell, a cell the viewshed hides, a cell behind the camera: NaN; float32 frames give float32."""
    from glimpse_amd import Camera

    args, frame, x, y, z = ortho_scene.closed_form()
    z = z.copy()
    z[0, 1] = np.nan
    mask, visible = np.ones((3, 3), bool), np.ones((3, 3), bool)
    mask[1, 1], visible[2, 0] = False, False
    got, _, seen = ortho_rule.orthorectify(Camera(**args), frame.astype(np.float32), x, y, z, mask=mask, viewshed=visible)
    assert got.dtype == np.float32
    assert (np.isnan(got[:, :, 0]) == ~seen).all() and (~seen == np.array([[0, 1, 0], [0, 1, 0], [1, 0, 0]], bool)).all()
    up = Camera(**{**args, "viewdir": (0, 90, 0)})
    got, uv, seen = ortho_rule.orthorectify(up, frame, x, y, z)
    assert np.isnan(uv).all() and not seen.any() and np.isnan(got).all()


@pytest.mark.parametrize("viewdir", ortho_scene.VIEWDIRS)
def test_the_agreement_scene_meets_its_conditions(viewdir):
    """What the exact comparisons of tests/test_gpu_orthorectify.py rest on, checked here without a device and without
    the viewshed (so over more cells than the device test compares): no cell's restated uv lies within 1e-9 px of a
    frame edge, of a pixel-centre line or of a pixel boundary; and the scene has every kind of cell it is meant to."""
    cam, dem = ortho_scene.objects(viewdir)
    frame = ortho_scene.frame(np.float64, 1)
    got, uv, seen = ortho_rule.orthorectify(cam, frame, dem.x, dem.y, dem.array)
    everywhere = ~np.isnan(uv).any(axis=2)
    for method in ("linear", "nearest"):
        assert ortho_rule.fragile_cells(uv, everywhere, (ortho_scene.FW, ortho_scene.FH), method) == 0
    assert dem.shape == (ortho_scene.NY, ortho_scene.NX) and dem.y[0] > dem.y[-1]
    assert ortho_scene.NX % 32 and ortho_scene.NY % 8 and ortho_scene.NX > 32 and ortho_scene.NY > 8
    assert cam.k.all() and cam.p.all() and isinstance(cam.correction, dict)
    behind = np.isnan(uv).any(axis=2) & ~np.isnan(dem.array)
    outside = everywhere & ~seen
    edge = seen & np.isnan(got[:, :, 0])  # in the frame, within half a pixel of its edge
    valued = ~np.isnan(got[:, :, 0])
    print(f"{viewdir}: behind {behind.sum()}, outside {outside.sum()}, edge {edge.sum()}, valued {valued.sum()}")
    assert behind.sum() > 50 and outside.sum() > 50 and edge.sum() >= 3 and valued.sum() > 300
    if viewdir == ortho_scene.VIEWDIRS[0]:
        assert valued[ortho_scene.MASK_BLOCK].all()  # (the mask takes away cells that would have a value)
        for r, c in ortho_scene.NAN_CELLS:  # (so do the NaN elevations: each has valued neighbours left and right)
            assert np.isnan(dem.array[r, c]) and valued[r, c - 1] and valued[r, c + 1]

