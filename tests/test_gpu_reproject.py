"""`Image.project` / `Observer.project` on the device, through the Python API and so through the C ABI
(`glh_stage_reproject`, kernel `k_reproject`).

Where the numbers come from (none of them was fitted to the kernel):

* delta = 1e-10 px: the coordinate agreement granted to the device -- its projections are pinned to the reference at
  1e-12 px (g1, g14); two orders above that absorb the 20-iteration undistortion.
* float frames against g27: a coordinate error delta moves a bilinear value by at most delta x (the largest difference
  between horizontally or vertically adjacent source pixels); the corner sum adds 4 ulp of the frame's dtype at the
  frame's largest magnitude; a float32 frame adds one float32 rounding, which can land on the neighbouring float32:
  1 ulp of float32 there.
* integer frames against g27: truncation flips a value by one level when the interpolated value lies within
  delta x gradient of an integer: at most 1e-4 of a case's non-fill values may differ, each by exactly one level
  (tools/make_golden.py keeps only textures on which the reference against itself turned by 1e-11 degrees stays below
  1e-5).  "nearest" picks flip only where the normalised distance is 0.5 +- delta: the same cap on the share, for float
  frames too; a flipped pick of a float frame differs by at most the largest neighbour difference.
* fill boundary: a target pixel whose reference source coordinate lies within delta of 0.5 or n - 0.5 may be fill on
  one side and a value on the other; exactly those pixels (from the uv stored in g27) are left out, and they must be
  fewer than 1e-4 of the frame.  Every other fill pixel must match.
* against SciPy on the device's own coordinates (`stage_unproject` -> `stage_project_directions`, the uv the kernel
  computes bit for bit): integer frames and fill masks equal everywhere; float32 values within the corner-sum and
  rounding terms above (no coordinate term).
"""
import datetime
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DELTA = 1e-10
CAP = 1e-4
T0 = datetime.datetime(2020, 1, 1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_reproject.npz")
RUNS = [str(k) for k in np.load(GOLDEN, allow_pickle=False)["runs"]]


def camera(v):
    from glimpse_amd import Camera

    return Camera(imgsz=v[6:8], f=v[8:10], c=v[10:12], k=v[12:18], p=v[18:20], xyz=v[0:3], viewdir=v[3:6])


def image(frame, cam, day=0):
    from glimpse_amd import Image

    return Image(cam=cam, array=frame, datetime=T0 + datetime.timedelta(days=day))


def neighbour_step(frame):
    f = frame.astype(np.float64)
    return max(np.abs(np.diff(f, axis=0)).max(), np.abs(np.diff(f, axis=1)).max())


def value_tolerance(frame, delta=DELTA):
    top = np.abs(frame.astype(np.float64)).max()
    tol = delta * neighbour_step(frame) + 4 * float(np.spacing(frame.dtype.type(top)))
    if frame.dtype == np.float32:
        tol += float(np.spacing(np.float32(top)))
    return tol


def near_boundary(uv, w, h):
    with np.errstate(invalid="ignore"):
        return ((np.abs(uv[:, 0] - 0.5) < DELTA) | (np.abs(uv[:, 0] - (w - 0.5)) < DELTA)
                | (np.abs(uv[:, 1] - 0.5) < DELTA) | (np.abs(uv[:, 1] - (h - 0.5)) < DELTA))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("key", RUNS)
def test_against_the_reference(golden, key):
    g = golden("g27_reproject.npz")
    name, dtype, ch, method = key.split("__")
    frame = np.ascontiguousarray(g["frame__" + dtype][:, :, :int(ch)])
    src, dst, want, uv = camera(g[name + "__src_cam"]), camera(g[name + "__dst_cam"]), g[key], g[name + "__uv"]
    got = image(frame if int(ch) == 3 else frame[:, :, 0], src).project(dst, method=method)
    assert got.dtype == want.dtype == frame.dtype and got.shape == want.shape
    h, w = frame.shape[:2]
    edge = near_boundary(uv, w, h).reshape(want.shape[:2])
    assert edge.mean() < CAP
    if want.dtype.kind == "f":
        filled = np.isnan(want).all(axis=2)
        assert (np.isnan(want).any(axis=2) == filled).all()
        got_filled = np.isnan(got).any(axis=2)
        assert (got_filled == filled)[~edge].all(), f"{((got_filled != filled) & ~edge).sum()} fill pixels differ"
        live = ~filled & ~got_filled & ~edge
        diff = np.abs(got[live].astype(np.float64) - want[live].astype(np.float64))
        tol = value_tolerance(frame)
        print(f"{key}: max |diff| {diff.max() if diff.size else 0.0:.3e} (tolerance {tol:.3e}), bit-equal "
              f"{same_bits(got, want)}, fill {filled.mean():.3f}, boundary pixels {int(edge.sum())}")
        if method == "linear":
            assert (diff <= tol).all()
        elif diff.size:
            assert (diff > tol).mean() <= CAP and diff.max() <= neighbour_step(frame)
    else:
        filled = g[key + "__fill"]
        assert (got[filled & ~edge] == 0).all()
        live = ~filled & ~edge
        diff = np.abs(got[live].astype(np.int64) - want[live].astype(np.int64))
        print(f"{key}: {int((diff != 0).sum())} of {diff.size} values differ, max {diff.max() if diff.size else 0}, "
              f"fill {filled.mean():.3f}, boundary pixels {int(edge.sum())}")
        if method == "linear":
            assert diff.size == 0 or diff.max() <= 1
        if diff.size:
            assert (diff != 0).mean() <= CAP


def texture(h, w, channels, seed):
    """Smooth waves plus noise in [0, 1): gradients everywhere, no constant areas."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    planes = []
    for c in range(channels):
        a, b, p = rng.uniform(0.01, 0.05, 3)
        z = 0.3 * np.sin(a * x + c) + 0.3 * np.cos(b * y - c) + 0.2 * np.sin(p * (x + y)) + 0.2 * rng.random((h, w), dtype=np.float32)
        planes.append((z + 0.8) / 1.81)
    return np.stack(planes, axis=2)


FULL = dict(f=(2600.0, 2650.0), c=(12.5, -8.0), k=(0.1, -0.05, 0.01, 0.02, -0.01, 0.005), p=(0.001, -0.002),
            xyz=(1.0, 2.0, 3.0), viewdir=(10.0, 5.0, 2.0))


def device_uv(src, dst):
    """The source coordinates of every target pixel centre from the device's own stage hooks."""
    from glimpse_amd import _lib

    dw, dh = (int(v) for v in dst.imgsz)
    U, V = np.meshgrid(np.linspace(0.5, dw - 0.5, dw), np.linspace(0.5, dh - 0.5, dh))
    rays = _lib.stage_unproject(dst.vector24, np.column_stack((U.ravel(), V.ravel())), directions=True)
    return _lib.stage_project(src.vector24, rays, directions=True)


def scipy_sample(frame, uv, dst, method):
    """RegularGridInterpolator on the host at those coordinates, as image.py:345-360 calls it."""
    import scipy.interpolate

    dw, dh = (int(v) for v in dst.imgsz)
    h, w = frame.shape[:2]
    pu, pv = np.linspace(0.5, w - 0.5, w), np.linspace(0.5, h - 0.5, h)
    want = np.full((dh, dw, frame.shape[2]), np.nan, dtype=np.float64)
    for i in range(frame.shape[2]):
        f = scipy.interpolate.RegularGridInterpolator((pv, pu), frame[:, :, i], method=method, bounds_error=False)
        want[:, :, i] = f(np.fliplr(uv)).reshape(dh, dw)
    return want


def test_full_size_uint8_equals_scipy_on_the_device_coordinates():
    from glimpse_amd import Camera

    frame = np.floor(texture(2048, 2048, 3, seed=1) * 256.0).astype(np.uint8)
    src = Camera(imgsz=(2048, 2048), **FULL)
    dst = Camera(imgsz=(2048, 2048), f=(2600.0, 2650.0), xyz=FULL["xyz"], viewdir=(11.5, 5.7, 1.0))
    uv = device_uv(src, dst)
    for method in ("linear", "nearest"):
        want = scipy_sample(frame, uv, dst, method)
        got = image(frame, src).project(dst, method=method)
        assert got.dtype == np.uint8 and got.shape == (2048, 2048, 3)
        filled = np.isnan(want).all(axis=2)
        assert 0.0 < filled.mean() < 0.5
        with np.errstate(invalid="ignore"):
            expect = np.where(np.isnan(want), 0.0, want).astype(np.uint8)  # (truncation; the fill written as 0)
        differ = int((got != expect).sum())
        print(f"2048 x 2048 x 3 uint8 {method}: {differ} values differ, fill {filled.mean():.4f}")
        assert differ == 0


def test_full_size_float32_equals_scipy_on_the_device_coordinates():
    from glimpse_amd import Camera

    frame = (texture(2048, 2048, 1, seed=2) * 1000.0 - 300.0).astype(np.float32)
    src = Camera(imgsz=(2048, 2048), **FULL)
    dst = Camera(imgsz=(1536, 1024), f=(1800.0, 1800.0), xyz=FULL["xyz"], viewdir=(8.0, 3.0, 2.5))  # another size and f
    want = scipy_sample(frame, device_uv(src, dst), dst, "linear")
    got = image(frame[:, :, 0], src).project(dst)
    assert got.dtype == np.float32 and got.shape == (1024, 1536, 1)
    filled = np.isnan(want)
    assert (np.isnan(got) == filled).all() and 0.0 < filled.mean() < 0.5
    diff = np.abs(got[~filled].astype(np.float64) - want[~filled].astype(np.float32).astype(np.float64))
    tol = value_tolerance(frame, delta=0.0)
    print(f"2048 x 2048 float32 -> 1536 x 1024 linear: max |diff| {diff.max():.3e} (tolerance {tol:.3e}), "
          f"bit-equal values {int((diff == 0).sum())} of {diff.size}")
    assert (diff <= tol).all()


def test_identity_nearest_returns_the_frame():
    from glimpse_amd import Camera

    rng = np.random.default_rng(3)
    cam = Camera(imgsz=(160, 120), f=(200.0, 210.0), xyz=(5.0, -2.0, 9.0), viewdir=(33.0, -7.0, 4.0))
    for dtype, channels in ((np.uint8, 3), (np.uint16, 1), (np.float32, 3), (np.float64, 1)):
        frame = (rng.random((120, 160, channels)) * 250.0).astype(dtype)
        got = image(frame, cam).project(cam.copy(), method="nearest")
        assert got.dtype == frame.dtype and got.shape == frame.shape
        # (a border pixel's centre comes back within rounding of the half-pixel limit: value or fill)
        assert same_bits(np.ascontiguousarray(got[1:-1, 1:-1]), np.ascontiguousarray(frame[1:-1, 1:-1]))


def wandering_images(dtype, channels):
    """(target camera, nine images at its position whose view direction wanders)."""
    from glimpse_amd import Camera

    target = Camera(imgsz=(96, 80), f=(150.0, 150.0), xyz=(1.0, 2.0, 3.0), viewdir=(10.0, 5.0, 0.0))
    images = []
    for i in range(9):
        cam = Camera(imgsz=(128, 96), f=(160.0, 165.0), c=(2.5, -1.5), k=(0.1, -0.05, 0.01, 0.0, 0.0, 0.0),
                     xyz=(1.0, 2.0, 3.0), viewdir=(10.0 + 0.8 * np.sin(i), 5.0 + 0.5 * np.cos(2 * i), 0.3 * i - 1.0))
        frame = (texture(96, 128, channels, seed=10 + i) * 250.0).astype(dtype)
        images.append(image(frame if channels == 3 else frame[:, :, 0], cam, day=i))
    return target, images


def test_the_timed_ring_of_reproject_returns_the_same_bytes_and_a_kernel_time():
    """`return_kernel_ms=True` adds a pair of events around every frame's kernel (glh_frame_ring.h); seven frames go
    twice round the ring's three slots and one further.  No bound on the time itself."""
    from glimpse_amd import _lib

    for dtype, channels, method in ((np.uint8, 3, "linear"), (np.float32, 1, "nearest")):
        target, images = wandering_images(dtype, channels)
        frames = np.stack([img._project_frame() for img in images[1:8]])
        cams = np.stack([img.cam.vector24 for img in images[1:8]])
        plain = _lib.stage_reproject(frames, cams, target.vector24, target.imgsz, method)
        timed, kernel_ms = _lib.stage_reproject(frames, cams, target.vector24, target.imgsz, method, return_kernel_ms=True)
        print(f"reproject, seven frames, timed ring: kernel_ms {kernel_ms:.4f}")
        assert plain.shape == (7, 80, 96, channels) and same_bits(timed, plain)
        assert np.isfinite(kernel_ms) and kernel_ms > 0.0
        for i, img in enumerate(images[1:8]):
            assert same_bits(np.ascontiguousarray(timed[i]), img.project(target, method=method)), i


def test_observer_project_equals_the_per_image_calls():
    from glimpse_amd import Observer

    for dtype, channels, method in ((np.uint8, 3, "linear"), (np.float32, 1, "linear"), (np.uint16, 3, "nearest")):
        target, images = wandering_images(dtype, channels)
        obs = Observer(images)
        batch = obs.project(target, method=method)
        assert batch.shape == (9, 80, 96, channels) and batch.dtype == np.dtype(dtype)
        singles = [img.project(target, method=method) for img in images]
        for i, one in enumerate(singles):
            assert same_bits(np.ascontiguousarray(batch[i]), one), i
        assert not same_bits(np.ascontiguousarray(batch[0]), np.ascontiguousarray(batch[1]))
        picked = obs.project(target, index=[7, 2], method=method)
        assert same_bits(np.ascontiguousarray(picked[0]), singles[7]) and same_bits(np.ascontiguousarray(picked[1]), singles[2])
        assert same_bits(obs.project(target, index=slice(3, 6), method=method), np.stack(singles[3:6]))
