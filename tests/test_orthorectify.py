"""`Image.orthorectify` / `Observer.orthorectify` without a device: the argument checks come before any library call, the
restatement of the rule (tests/ortho_rule.py) returns the frame on the closed-form scene, and the agreement scene of
tests/test_gpu_orthorectify.py meets the conditions its exact comparisons rest on -- as does every station of the batch
of tests/test_gpu_orthorectify_batches.py, whose masks moreover tell the stations apart -- and `orthorectify()` hands the
library one mask per distinct (position, correction) with each frame's mask named (recorders in the library's place)."""
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


def scene_conditions(cam, dem, name):
    """The conditions of the agreement scene for one camera, without the viewshed: no cell's restated uv lies within
    1e-9 px of a frame edge, of a pixel-centre line or of a pixel boundary, and every kind of cell is there.  Returns
    (uv, the cells with a value)."""
    size = tuple(int(v) for v in cam.imgsz)
    frame = ortho_scene.frame(np.float64, 1, size=size)
    got, uv, seen = ortho_rule.orthorectify(cam, frame, dem.x, dem.y, dem.array)
    everywhere = ~np.isnan(uv).any(axis=2)
    for method in ("linear", "nearest"):
        assert ortho_rule.fragile_cells(uv, everywhere, size, method) == 0
    assert dem.shape == (ortho_scene.NY, ortho_scene.NX) and dem.y[0] > dem.y[-1]
    assert ortho_scene.NX % 32 and ortho_scene.NY % 8 and ortho_scene.NX > 32 and ortho_scene.NY > 8
    assert cam.k.all() and cam.p.all()
    behind = np.isnan(uv).any(axis=2) & ~np.isnan(dem.array)
    outside = everywhere & ~seen
    edge = seen & np.isnan(got[:, :, 0])  # in the frame, within half a pixel of its edge
    valued = ~np.isnan(got[:, :, 0])
    print(f"{name}: behind {behind.sum()}, outside {outside.sum()}, edge {edge.sum()}, valued {valued.sum()}")
    assert behind.sum() > 50 and outside.sum() > 50 and edge.sum() >= 3 and valued.sum() > 300
    return uv, valued


@pytest.mark.parametrize("viewdir", ortho_scene.VIEWDIRS)
def test_the_agreement_scene_meets_its_conditions(viewdir):
    """What the exact comparisons of tests/test_gpu_orthorectify.py rest on, checked here without a device and without
    the viewshed (so over more cells than the device test compares): no cell's restated uv lies within 1e-9 px of a
    frame edge, of a pixel-centre line or of a pixel boundary; and the scene has every kind of cell it is meant to."""
    cam, dem = ortho_scene.objects(viewdir)
    _, valued = scene_conditions(cam, dem, viewdir)
    assert isinstance(cam.correction, dict)
    if viewdir == ortho_scene.VIEWDIRS[0]:
        assert valued[ortho_scene.MASK_BLOCK].all()  # (the mask takes away cells that would have a value)
        for r, c in ortho_scene.NAN_CELLS:  # (so do the NaN elevations: each has valued neighbours left and right)
            assert np.isnan(dem.array[r, c]) and valued[r, c - 1] and valued[r, c + 1]


def test_the_odd_frame_shape_is_odd_in_every_byte_count():
    w, h = ortho_scene.ODD_SIZE
    assert (w, h) == (47, 39) and (w * h * 3) % 4
    for itemsize in (1, 2, 4, 8):
        for channels in (1, 3):
            assert (w * h * channels * itemsize) % 16


@pytest.fixture(scope="module")
def restated_viewsheds():
    """The viewshed of every station from the restatement (tests/viewshed_restatement.py), one per mask key, ANDed with
    the scene's mask: what `viewshed=True, mask=mask` makes of the batch."""
    from tests import viewshed_restatement

    dem = ortho_scene.objects()[1]
    masks = {}
    for (position, _, correction), k in zip(ortho_scene.stations(), ortho_scene.STATION_MASKS):
        if k not in masks:
            assert k == len(masks)  # (numbered by first appearance)
            masks[k] = viewshed_restatement.of_raster(dem, ortho_scene.POSITIONS[position], correction)
    return dem, [masks[k] for k in range(len(masks))]


@pytest.mark.parametrize("size", [(ortho_scene.FW, ortho_scene.FH), ortho_scene.ODD_SIZE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_station_meets_the_scene_conditions_and_the_masks_discriminate(restated_viewsheds, size):
    """The agreement scene's conditions for each of the eight stations and both frame shapes -- with the counts
    tests/test_gpu_orthorectify.py asserts under the viewshed and the mask: valued cells, seen cells within half a pixel
    of the edge, cells the ridge hides -- and what the batch tests rest on beyond them: the four masks are pairwise
    different where it shows.  Every frame has at least 10 cells that have a value under its own mask and none under
    another one, or the reverse, for each other mask: a frame shown through a wrong mask cannot pass."""
    dem, viewsheds = restated_viewsheds
    stations, mask = ortho_scene.stations(), ortho_scene.mask()
    assert len(stations) == 8 and [s[0] for s in stations] == [0, 1, 0, 2, 1, 0, 2, 1]
    assert ortho_scene.POSITIONS[0] == (17.83, 4.29, 3.37) and len(set(ortho_scene.POSITIONS)) == 3
    keys = [(p, tuple(sorted(c.items())) if isinstance(c, dict) else c) for p, _, c in stations]
    first = sorted(set(keys), key=keys.index)
    assert tuple(first.index(k) for k in keys) == ortho_scene.STATION_MASKS and len(first) == 4
    assert stations[2][2] is False and keys[2][0] == keys[0][0] == keys[5][0] and keys[0] == keys[5] != keys[2]
    valued_unmasked = []
    for i, station in enumerate(stations):
        cam = ortho_scene.station_camera(station, size)
        uv, valued = scene_conditions(cam, dem, f"station {i} at {size}")
        visible = viewsheds[ortho_scene.STATION_MASKS[i]]
        frame = ortho_scene.frame(np.float64, 1, size=size)
        got, _, seen = ortho_rule.orthorectify(cam, frame, dem.x, dem.y, dem.array, mask=mask, viewshed=visible)
        shown = ~np.isnan(got[:, :, 0])
        hidden = ~visible & ~np.isnan(uv).any(axis=2) & ortho_rule.inframe(cam, uv.reshape(-1, 2)).reshape(seen.shape)
        print(f"station {i} at {size}: valued {shown.sum()}, edge {(seen & ~shown).sum()}, hidden {hidden.sum()}")
        assert shown.sum() > 100 and (seen & ~shown).sum() >= 3 and hidden.sum() > 50
        valued_unmasked.append(valued)
    masks = [v & mask for v in viewsheds]
    least = ortho_scene.discrimination(valued_unmasked, masks, ortho_scene.STATION_MASKS)
    print(f"{size}: the least number of cells that tell two masks apart in a frame: {least}")
    assert least >= 10


def station_images(dtype=np.uint8, channels=3):
    return [ortho_scene.image(ortho_scene.frame(dtype, channels, seed=i), ortho_scene.station_camera(station), day=i)
            for i, station in enumerate(ortho_scene.stations())]


@pytest.fixture
def recorded(monkeypatch):
    """`Raster.viewshed` and `_lib.stage_orthorectify` replaced by recorders: what `orthorectify()` asks for and what it
    hands the library, without a device.  Viewshed call k returns its own pseudo-random booleans, kept in "returned"."""
    from glimpse_amd import Raster, _lib

    calls = {"viewshed": [], "returned": [], "stage": []}

    def viewshed(self, origin, correction=False):
        calls["viewshed"].append((tuple(float(v) for v in origin), correction))
        calls["returned"].append(np.random.default_rng(len(calls["returned"])).random((ortho_scene.NY, ortho_scene.NX)) < 0.5)
        return calls["returned"][-1].copy()

    def stage_orthorectify(frames, cams, z, x, y, seen=None, seen_of=None, method="linear"):
        calls["stage"].append({"frames": frames, "cams": cams, "seen": seen, "seen_of": seen_of, "method": method})
        return np.zeros((len(frames), len(y), len(x), frames.shape[3]))

    monkeypatch.setattr(Raster, "viewshed", viewshed)
    monkeypatch.setattr(_lib, "stage_orthorectify", stage_orthorectify)
    monkeypatch.setattr(_lib, "stage_viewshed", None)
    return calls


def same_correction(a, b):
    return type(a) is type(b) and a == b


def test_viewshed_true_asks_for_one_viewshed_per_position_and_correction(recorded):
    """Eight stations, four keys: `dem.viewshed` is called once per distinct (xyz, correction) in order of first
    appearance, with that station's own arguments; the masks are those viewsheds in that order, ANDed with the caller's
    mask; `seen_of` names each frame's."""
    from glimpse_amd import Observer
    from glimpse_amd.image import orthorectify

    images, dem = station_images(), ortho_scene.objects()[1]
    # the same correction with its items in another order is the same key
    images[5].cam.correction = dict(reversed(list(images[0].cam.correction.items())))
    assert list(images[5].cam.correction) != list(images[0].cam.correction) and images[5].cam.correction == images[0].cam.correction
    assert images[0].cam.correction["radius"] == 400.0 and images[2].cam.correction is False
    for mask in (ortho_scene.mask(), None):
        for calls in recorded.values():
            del calls[:]
        out = Observer(images).orthorectify(dem, viewshed=True, mask=mask, method="nearest")
        assert out.shape == (8, ortho_scene.NY, ortho_scene.NX, 3) and len(recorded["stage"]) == 1
        firsts = [0, 1, 2, 3]  # (the stations at which a key first appears)
        assert len(recorded["viewshed"]) == 4
        for (origin, correction), i in zip(recorded["viewshed"], firsts):
            assert origin == tuple(images[i].cam.xyz) == ortho_scene.POSITIONS[ortho_scene.stations()[i][0]]
            assert same_correction(correction, images[i].cam.correction)
        got = recorded["stage"][0]
        assert got["seen"].shape == (4, ortho_scene.NY, ortho_scene.NX) and got["seen"].dtype == bool
        for k, visible in enumerate(recorded["returned"]):
            assert (got["seen"][k] == (visible if mask is None else visible & mask)).all()
        assert len({m.tobytes() for m in got["seen"]}) == 4
        assert [int(k) for k in got["seen_of"]] == list(ortho_scene.STATION_MASKS)
        assert got["method"] == "nearest"
        assert (got["cams"] == np.stack([img.cam.vector24 for img in images])).all()
        assert got["frames"].tobytes() == np.stack([img.read() for img in images]).tobytes()
    # at one position, correction=True and correction=False are two keys; twice the same is one
    pair = [ortho_scene.image(ortho_scene.frame(np.uint8, 1), ortho_scene.objects(correction=c)[0], day=i)
            for i, c in enumerate((True, False, True))]
    for calls in recorded.values():
        del calls[:]
    orthorectify(pair, dem, True, None, "linear")
    assert [c for _, c in recorded["viewshed"]] == [pair[0].cam.correction, False]
    assert all(origin == ortho_scene.POSITIONS[0] for origin, _ in recorded["viewshed"])
    assert list(recorded["stage"][0]["seen_of"]) == [0, 1, 0] and recorded["stage"][0]["seen"].shape[0] == 2


def test_the_other_forms_of_viewshed_give_one_mask_or_none(recorded):
    from glimpse_amd import Observer

    images, dem, mask = station_images(np.float32, 1), ortho_scene.objects()[1], ortho_scene.mask()
    visible = np.random.default_rng(9).random((ortho_scene.NY, ortho_scene.NX)) < 0.6
    obs = Observer(images)
    for viewshed in (False, None, np.False_):
        obs.orthorectify(dem, viewshed=viewshed, mask=mask)
        obs.orthorectify(dem, viewshed=viewshed)
        with_mask, without = recorded["stage"][-2:]
        assert with_mask["seen"].shape == (1, ortho_scene.NY, ortho_scene.NX) and (with_mask["seen"][0] == mask).all()
        assert without["seen"] is None and with_mask["seen_of"] is None and without["seen_of"] is None
    obs.orthorectify(dem, viewshed=visible, mask=mask)
    obs.orthorectify(dem, viewshed=visible.astype(np.uint8))
    with_mask, without = recorded["stage"][-2:]
    assert with_mask["seen"].shape == (1, ortho_scene.NY, ortho_scene.NX) and (with_mask["seen"][0] == (visible & mask)).all()
    assert without["seen"].shape == (1, ortho_scene.NY, ortho_scene.NX) and (without["seen"][0] == visible).all()
    assert with_mask["seen_of"] is None and without["seen_of"] is None
    assert not recorded["viewshed"] and all(len(call["frames"]) == 8 for call in recorded["stage"])


def test_observer_orthorectify_numbers_the_masks_among_the_chosen_images(recorded):
    from glimpse_amd import Observer

    images, dem, mask = station_images(np.uint16, 1), ortho_scene.objects()[1], ortho_scene.mask()
    chosen = [5, 1, 6]
    out = Observer(images).orthorectify(dem, index=chosen, viewshed=True, mask=mask)
    assert out.shape == (3, ortho_scene.NY, ortho_scene.NX, 1)
    got, = recorded["stage"]
    assert (got["cams"] == np.stack([images[i].cam.vector24 for i in chosen])).all()
    assert got["frames"].tobytes() == np.stack([images[i].read()[:, :, None] for i in chosen]).tobytes()
    # stations 5, 1 and 6 stand at positions 0, 1 and 2: three masks, numbered in that order (in the whole batch they
    # are masks 0, 1 and 3)
    assert [int(k) for k in got["seen_of"]] == [0, 1, 2] and [ortho_scene.STATION_MASKS[i] for i in chosen] == [0, 1, 3]
    assert [origin for origin, _ in recorded["viewshed"]] == [ortho_scene.POSITIONS[p] for p in (0, 1, 2)]
    assert all(same_correction(c, images[i].cam.correction) for (_, c), i in zip(recorded["viewshed"], chosen))
    assert got["seen"].shape == (3, ortho_scene.NY, ortho_scene.NX)
    for k, visible in enumerate(recorded["returned"]):
        assert (got["seen"][k] == (visible & mask)).all()

