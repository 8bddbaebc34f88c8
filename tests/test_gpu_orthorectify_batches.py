"""The batch machinery around `k_orthorectify` on the device: several masks in one call (`seen`, `seen_of`, the mask
pointer's offset in glh_ortho.hip), the staging ring of glh_frame_ring.h below, at and beyond its NSLOT = 3 slots, the
timed ring, rasters stored in the other directions, and frames whose byte count is a multiple of nothing.

The single-frame kernel is pinned to the rule by tests/test_gpu_orthorectify.py; what is new here is compared bit for bit
with that single-frame path, and with the restatement of the rule (tests/ortho_rule.py) by the same comparison and the
same bound as there -- no new tolerance:

* NaN pattern and "nearest" picks: exact (no restated uv of a seen cell lies within 1e-9 px of a decision: asserted here
  on the compared cells, and in tests/test_orthorectify.py on all of them).
* "linear" values: within 4 x (the deviation of the existing projection stage `_lib.stage_project` from the NumPy
  restatement of `Camera.xyz_to_uv`, measured here per camera on the cells that land on the pixel centres' grid) x (the
  frame's largest difference between neighbouring pixels); bit for bit where that deviation is zero.

The scenes and why they are what they are: tests/ortho_scene.py.  That a frame shown through another frame's mask would
differ is asserted on the device's own viewsheds before any comparison leans on it.
"""
import numpy as np
import pytest

from tests import ortho_rule, ortho_scene
from tests.test_gpu_orthorectify import neighbour_step, same_bits

pytestmark = pytest.mark.gpu

NY, NX = ortho_scene.NY, ortho_scene.NX
FILLS = (1, 2, 3, 4, 7)  # frames in a call: a ring shorter than NSLOT = 3, exactly full, one past it, two wraps plus one
CHANGING = [2, 0, 1, 1, 2, 0, 2]  # a mask index that changes at every frame but one, and across both slot boundaries


def projection_deviation(cam, dem, _cache={}):
    """The largest |uv difference| between `_lib.stage_project` and the NumPy restatement of `Camera.xyz_to_uv` for `cam`
    over the DEM's cells whose restated uv lies on the pixel centres' grid: as the fixture of
    tests/test_gpu_orthorectify.py measures it, per camera."""
    from glimpse_amd import _lib

    key = cam.vector24.tobytes()
    if key not in _cache:
        X, Y = np.meshgrid(dem.x, dem.y)
        xyz = np.column_stack((X.ravel(), Y.ravel(), dem.array.ravel()))
        device_uv, numpy_uv = _lib.stage_project(cam.vector24, xyz), ortho_rule.xyz_to_uv(cam, xyz)
        assert (np.isnan(device_uv) == np.isnan(numpy_uv)).all()
        with np.errstate(invalid="ignore"):
            inside = ((numpy_uv >= 0.5) & (numpy_uv <= np.asarray(cam.imgsz) - 0.5)).all(axis=1)
        _cache[key] = float(np.abs(device_uv - numpy_uv)[inside].max())
    return _cache[key]


def agrees_with_the_rule(got, cam, frame, dem, seen_mask, method, label):
    """`got` (NY, NX, channels) against the rule for `frame` seen by `cam` under `seen_mask` (mask and viewshed of a
    cell, one boolean): the comparison of tests/test_gpu_orthorectify.py."""
    want, uv, seen = ortho_rule.orthorectify(cam, frame, dem.x, dem.y, dem.array, mask=seen_mask, method=method)
    assert got.shape == want.shape and got.dtype == want.dtype == (np.float32 if frame.dtype == np.float32 else np.float64)
    assert ortho_rule.fragile_cells(uv, seen, tuple(int(v) for v in cam.imgsz), method) == 0
    valued = ~np.isnan(want).any(axis=2)
    assert valued.sum() > 30
    assert (np.isnan(got) == np.isnan(want)).all()
    assert (np.isnan(want).all(axis=2) == ~valued).all()
    deviation = projection_deviation(cam, dem)
    diff = np.abs(got[valued].astype(np.float64) - want[valued].astype(np.float64))
    bound = 4.0 * deviation * neighbour_step(frame)
    print(f"{label} {frame.dtype.name} x {want.shape[2]} {method}: {int(valued.sum())} valued cells, max |diff| "
          f"{diff.max():.3e}, bound {bound:.3e} (projection deviation {deviation:.3e} px, neighbour step "
          f"{neighbour_step(frame):.6g}), bit-equal {same_bits(got, want)}")
    if method == "nearest" or deviation == 0.0:
        assert same_bits(got, want), label
    else:
        assert (diff <= bound).all(), label


def valued_without_a_mask(cam, dem):
    size = tuple(int(v) for v in cam.imgsz)
    got = ortho_rule.orthorectify(cam, ortho_scene.frame(np.float64, 1, size=size), dem.x, dem.y, dem.array)[0]
    return ~np.isnan(got[:, :, 0])


@pytest.fixture(scope="module")
def scene():
    """What the cases share, computed once: the DEM, the mask, the eight stations' cameras in both frame shapes, and the
    device's own viewshed of every mask key (the existing stage), numbered as `ortho_scene.STATION_MASKS` numbers them."""
    dem = ortho_scene.objects()[1]
    stations = ortho_scene.stations()
    cams = [ortho_scene.station_camera(s) for s in stations]
    viewsheds = {}
    for cam, k in zip(cams, ortho_scene.STATION_MASKS):
        if k not in viewsheds:
            viewsheds[k] = dem.viewshed(cam.xyz, correction=cam.correction)
    viewsheds = [viewsheds[k] for k in range(len(viewsheds))]
    assert len(viewsheds) == 4 and viewsheds[0].shape == (NY, NX) and viewsheds[0].dtype == bool
    return {"dem": dem, "mask": ortho_scene.mask(), "cams": cams, "viewsheds": viewsheds,
            "odd_cams": [ortho_scene.station_camera(s, ortho_scene.ODD_SIZE) for s in stations]}


def assert_the_masks_discriminate(scene, cams, mask_of):
    """Every frame has at least 10 cells with a value under its own mask and none under each other mask, or the reverse,
    on the device's own viewsheds: a frame shown through another station's mask cannot equal the right answer."""
    masks = [v & scene["mask"] for v in scene["viewsheds"]]
    least = ortho_scene.discrimination([valued_without_a_mask(cam, scene["dem"]) for cam in cams], masks, mask_of)
    print(f"the least number of cells that tell two masks apart in a frame: {least}")
    assert least >= 10


# ---- a. eight stations, four masks, one call -------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,channels,method", [(np.uint8, 3, "linear"), (np.float32, 1, "nearest"), (np.uint16, 1, "linear")],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_eight_stations_through_four_viewsheds_in_one_call(scene, monkeypatch, dtype, channels, method):
    from glimpse_amd import Observer, _lib

    dem, mask, cams = scene["dem"], scene["mask"], scene["cams"]
    assert_the_masks_discriminate(scene, cams, ortho_scene.STATION_MASKS)
    frames = [ortho_scene.frame(dtype, channels, seed=i) for i in range(8)]
    images = [ortho_scene.image(frame, cam, day=i) for i, (frame, cam) in enumerate(zip(frames, cams))]
    singles = [img.orthorectify(dem, viewshed=True, mask=mask, method=method) for img in images]
    calls = []
    stage_viewshed = _lib.stage_viewshed

    def counted(*args, **kwargs):
        calls.append(1)
        return stage_viewshed(*args, **kwargs)

    monkeypatch.setattr(_lib, "stage_viewshed", counted)
    batch = Observer(images).orthorectify(dem, viewshed=True, mask=mask, method=method)
    monkeypatch.setattr(_lib, "stage_viewshed", stage_viewshed)
    assert len(calls) == 4  # (eight images, three positions, one of them with and without the correction)
    assert batch.shape == (8, NY, NX, channels)
    for i, one in enumerate(singles):
        assert same_bits(np.ascontiguousarray(batch[i]), one), i
    for i, (cam, frame) in enumerate(zip(cams, frames)):
        visible = scene["viewsheds"][ortho_scene.STATION_MASKS[i]]
        assert same_bits(visible, dem.viewshed(cam.xyz, correction=cam.correction))
        agrees_with_the_rule(np.ascontiguousarray(batch[i]), cam, frame, dem, visible & mask, method, f"station {i}")


# ---- b. the ring at every fill level, explicit masks -----------------------------------------------------------------

RING_CASES = [(np.uint8, 3, "linear"), (np.float32, 1, "nearest")]


@pytest.fixture(scope="module")
def ring(scene):
    """Seven frames per pixel type with the first seven stations' cameras, three masks -- the viewshed of the agreement
    scene, its complement among the cells that lie in some camera's frame, a checkerboard -- and the one-frame results
    (frame i under mask k, through the path tests/test_gpu_orthorectify.py pins to the rule), computed when first asked
    for and left unchanged."""
    from glimpse_amd import _lib

    dem, cams = scene["dem"], scene["cams"][:7]
    X, Y = np.meshgrid(dem.x, dem.y)
    xyz = np.column_stack((X.ravel(), Y.ravel(), dem.array.ravel()))
    in_some_frame = np.zeros((NY, NX), bool)
    for cam in cams:
        in_some_frame |= ortho_rule.inframe(cam, ortho_rule.xyz_to_uv(cam, xyz)).reshape(NY, NX)
    visible = dem.viewshed(ortho_scene.POSITIONS[0], correction=True)
    rows, cols = np.mgrid[0:NY, 0:NX]
    masks = np.stack([visible, ~visible & in_some_frame, (rows + cols) % 2 == 0])
    assert all(m.sum() > 100 for m in masks) and (masks[0] & masks[1]).sum() == 0
    vectors = np.stack([cam.vector24 for cam in cams])
    frames = {case: np.stack([ortho_scene.frame(case[0], case[1], seed=20 + i).reshape(ortho_scene.FH, ortho_scene.FW, case[1])
                              for i in range(7)]) for case in RING_CASES}
    ones = {}

    def one(case, i, k):
        if (case, i, k) not in ones:
            got = _lib.stage_orthorectify(frames[case][i:i + 1], vectors[i:i + 1], dem.array, dem.x, dem.y,
                                          seen=masks[k:k + 1], method=case[2])
            assert got.shape == (1, NY, NX, case[1])
            ones[case, i, k] = got[0].copy()
            ones[case, i, k].flags.writeable = False
        return ones[case, i, k]

    return {"cams": cams, "vectors": vectors, "masks": masks, "frames": frames, "one": one}


@pytest.mark.parametrize("n", FILLS)
@pytest.mark.parametrize("case", RING_CASES, ids=lambda c: f"{np.dtype(c[0]).name}x{c[1]}-{c[2]}")
def test_every_fill_level_of_the_ring_equals_the_one_frame_calls(scene, ring, case, n):
    from glimpse_amd import _lib

    dem, masks, frames, vectors = scene["dem"], ring["masks"], ring["frames"][case], ring["vectors"]
    # the three masks give three different answers for every frame: a wrong mask cannot pass
    for i in range(n):
        assert len({ring["one"](case, i, k).tobytes() for k in range(3)}) == 3
    for name, seen_of in (("none", None), ("last", [2] * n), ("changing", CHANGING[:n])):
        def call():
            return _lib.stage_orthorectify(frames[:n], vectors[:n], dem.array, dem.x, dem.y, seen=masks,
                                           seen_of=None if seen_of is None else np.array(seen_of), method=case[2])
        got = call()
        assert got.shape == (n, NY, NX, case[1])
        for i in range(n):
            k = 0 if seen_of is None else seen_of[i]
            assert same_bits(np.ascontiguousarray(got[i]), ring["one"](case, i, k)), (name, n, i, k)
        assert same_bits(call(), got), name  # (a second identical call: identical bytes)
        if n == 7:
            for i in range(n):
                k = 0 if seen_of is None else seen_of[i]
                frame = frames[i] if case[1] == 3 else frames[i][:, :, 0]
                agrees_with_the_rule(np.ascontiguousarray(got[i]), ring["cams"][i], frame, dem, masks[k], case[2],
                                     f"ring of 7, seen_of {name}, frame {i} under mask {k}:")
    if n >= 2:
        assert not same_bits(np.ascontiguousarray(got[0]), np.ascontiguousarray(got[1]))


# ---- c. the timed ring -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", RING_CASES, ids=lambda c: f"{np.dtype(c[0]).name}x{c[1]}-{c[2]}")
def test_the_timed_ring_returns_the_same_bytes_and_a_kernel_time(scene, ring, case):
    from glimpse_amd import _lib

    dem = scene["dem"]
    args = (ring["frames"][case], ring["vectors"], dem.array, dem.x, dem.y)
    kwargs = dict(seen=ring["masks"], seen_of=np.array(CHANGING), method=case[2])
    plain = _lib.stage_orthorectify(*args, **kwargs)
    timed, kernel_ms = _lib.stage_orthorectify(*args, return_kernel_ms=True, **kwargs)
    print(f"seven frames, timed ring: kernel_ms {kernel_ms:.4f}")
    assert same_bits(timed, plain)
    assert np.isfinite(kernel_ms) and kernel_ms > 0.0
    for i, k in enumerate(CHANGING):
        assert same_bits(np.ascontiguousarray(timed[i]), ring["one"](case, i, k)), i


# ---- d. orientation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ascending_y", [False, True], ids=["descending_x", "descending_x-ascending_y"])
def test_a_raster_stored_in_another_direction_gives_the_flipped_result(scene, ascending_y):
    """The same DEM stored last column first (and bottom row first): the cells are the same points, so the result is the
    other one's columns (and rows) in reverse, bit for bit.  The viewshed and the mask are given, flipped the same way:
    how the viewshed's sort breaks ties follows the cell order and is not what this is about."""
    def flip(a):
        a = a[:, ::-1]
        return np.ascontiguousarray(a[::-1] if ascending_y else a)

    frame = ortho_scene.frame(np.uint8, 3)
    cam, dem = ortho_scene.objects()
    visible = dem.viewshed(cam.xyz, correction=cam.correction)
    other_cam, other = ortho_scene.objects(descending_x=True, ascending_y=ascending_y)
    assert other.x[0] > other.x[-1] and (other.y[0] < other.y[-1]) == ascending_y
    assert same_bits(flip(other.array), np.ascontiguousarray(dem.array))
    for method in ("linear", "nearest"):
        base = ortho_scene.image(frame, cam).orthorectify(dem, viewshed=visible, mask=scene["mask"], method=method)
        got = ortho_scene.image(frame, other_cam).orthorectify(other, viewshed=flip(visible), mask=flip(scene["mask"]),
                                                               method=method)
        assert (~np.isnan(base)).sum() > 300
        assert same_bits(flip(got), base), method
        assert not same_bits(got, base)


# ---- e. the 47 x 39 frame --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,channels", [(np.uint8, 3), (np.float32, 1)], ids=lambda v: getattr(v, "__name__", str(v)))
def test_frames_of_47_by_39_pixels_alone_and_in_a_batch_of_four(scene, dtype, channels):
    """A frame's byte count is odd (uint8) or no multiple of 16 (float32): the staging buffers and the sampler's loads
    have nothing aligned to lean on.  The first four stations are the four masks."""
    from glimpse_amd import Observer

    dem, mask, cams = scene["dem"], scene["mask"], scene["odd_cams"][:4]
    assert ortho_scene.STATION_MASKS[:4] == (0, 1, 2, 3)
    assert_the_masks_discriminate(scene, cams, ortho_scene.STATION_MASKS[:4])
    frames = [ortho_scene.frame(dtype, channels, seed=40 + i, size=ortho_scene.ODD_SIZE) for i in range(4)]
    assert frames[0].shape[:2] == (39, 47) and frames[0].nbytes % 16
    images = [ortho_scene.image(frame, cam, day=i) for i, (frame, cam) in enumerate(zip(frames, cams))]
    for method in ("linear", "nearest"):
        batch = Observer(images).orthorectify(dem, viewshed=True, mask=mask, method=method)
        assert batch.shape == (4, NY, NX, channels)
        for i, (cam, frame) in enumerate(zip(cams, frames)):
            single = images[i].orthorectify(dem, viewshed=True, mask=mask, method=method)
            seen_mask = scene["viewsheds"][i] & mask
            agrees_with_the_rule(single, cam, frame, dem, seen_mask, method, f"47 x 39 alone, station {i}:")
            agrees_with_the_rule(np.ascontiguousarray(batch[i]), cam, frame, dem, seen_mask, method,
                                 f"47 x 39 in a batch of four, station {i}:")
            assert same_bits(np.ascontiguousarray(batch[i]), single), (method, i)
