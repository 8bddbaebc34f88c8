"""Ray casting without a device: the restatement of the rule (tests/raycast_rule.py) against two independent answers, the
package's host logic with the library call answered by the restatement, the refusals, the stage's argument checks and
`helpers.intersect_rays_plane`.  tests/test_gpu_raycast.py then holds the kernel to the restatement bit for bit."""
import datetime
import re

import numpy as np
import pytest

from tests import raycast_rule as rr
from tests import raycast_scene as sc

# |z_hit - bilinear surface at xy_hit| of the restatement's hits on the base scene, the largest of 2686 (metres), with
# scipy's RegularGridInterpolator over the cell centres as the surface: tests/test_gpu_raycast.py allows the device's
# hits 4 x this against Raster.sample(order=1) (INPUTS.md, "Ray casting: the rule").
HIT_RESIDUAL = 1.7053025658242404e-13
# the largest |t - t_plane| / t of test_the_restatement_on_a_tilted_plane, as measured
PLANE_DEVIATION = 6.325274735242972e-16
WHEN = datetime.datetime(2020, 6, 1, 12)


def base_rays():
    return rr.camera_rays(sc.camera(False), sc.pixel_centres())


def surface(dem):
    """The bilinear surface between the cell centres of a Raster, by scipy: f(xy) -> z."""
    from scipy.interpolate import RegularGridInterpolator

    x, y, z = dem.x, dem.y, np.asarray(dem.array, dtype=np.float64)
    if x[0] > x[-1]:
        x, z = x[::-1], z[:, ::-1]
    if y[0] > y[-1]:
        y, z = y[::-1], z[::-1]
    f = RegularGridInterpolator((y, x), z, bounds_error=False)
    return lambda xy: f(np.column_stack((xy[:, 1], xy[:, 0])))


def hit_residual(dem, t, xyz, d, hit, correction=None):
    """|z_hit - surface(xy_hit) - correction| of the hits."""
    K = 0.0 if correction is None else (correction[1] - 1.0) / (2.0 * correction[0])
    corr = K * t[hit] ** 2 * (d[hit, 0] ** 2 + d[hit, 1] ** 2)
    return np.abs(xyz[hit, 2] - surface(dem)(xyz[hit, 0:2]) - corr)


def test_the_restatement_against_dense_sampling():
    """An independent pin: g = ray height - scipy's bilinear surface sampled along every ray at 1/64 of a cell.  The
    first sign change must bracket the rule's t to within one sampling step.  Rays on which the sampling finds g < 0
    before the rule's hit -- dips within one patch, which the rule states it misses -- are counted: at most 0.5 %.  On
    the terrain of tests/raycast_scene.py (seed 7, the first tried) there are none among 3072 rays."""
    dem = sc.dem()
    o, d = base_rays()
    z, x0, y0, d0, d1 = sc.grid_args(dem)
    t, xyz, patch, status = rr.cast(o, d, z, x0, y0, d0, d1)
    assert set(status) == {rr.HIT, rr.LEAVES} and (status == rr.HIT).sum() > 2000
    f = surface(dem)
    # the domain in world coordinates, by the slab test on the outer cell centres
    lo = np.array([min(dem.x[0], dem.x[-1]), min(dem.y[0], dem.y[-1])])
    hi = np.array([max(dem.x[0], dem.x[-1]), max(dem.y[0], dem.y[-1])])
    with np.errstate(divide="ignore"):
        ta, tb = (lo - o[0:2]) / d[:, 0:2], (hi - o[0:2]) / d[:, 0:2]
    t_in = np.maximum(np.minimum(ta, tb).max(axis=1), 0.0)
    t_out = np.maximum(ta, tb).min(axis=1)
    dt = (1.0 / 64.0) / np.hypot(d[:, 0] / d0, d[:, 1] / d1)
    count = int(np.ceil((t_out - t_in) / dt).max()) + 1
    grazes = compared = 0
    for k in range(len(d)):
        ts = np.minimum(t_in[k] + dt[k] * np.arange(count), t_out[k])
        pts = o + ts[:, None] * d[k]
        # (a sample a rounding outside the rectangle is pulled onto its edge)
        g = pts[:, 2] - f(np.clip(pts[:, 0:2], lo, hi))
        under = np.nonzero(g <= 0)[0]
        if status[k] == rr.LEAVES:
            grazes += len(under) > 0
            continue
        assert len(under) and under[0] > 0, k
        first = under[0]
        if ts[first] < t[k] - dt[k]:
            grazes += 1
            continue
        compared += 1
        assert ts[first - 1] - dt[k] <= t[k] <= ts[first] + dt[k], (k, ts[first - 1], t[k], ts[first])
    print(f"{compared} hits bracketed by the dense sampling, {grazes} grazes of {len(d)} rays")
    assert grazes <= 0.005 * len(d)
    assert compared + grazes >= (status == rr.HIT).sum()


def test_the_restatement_on_a_tilted_plane():
    """z = a x + b y + c, which bilinear patches reproduce: the rule's t against the closed-form ray-plane t.  The bound
    is measured, not guessed: the largest |t - t_plane| / t the restatement shows here is 6.33e-16 (PLANE_DEVIATION, over
    2748 hits), times 8 for the chain of roundings in the patch coordinates: 5.06e-15."""
    dem = sc.dem()
    a, b, c = 0.31, -0.17, 95.0
    X, Y = np.meshgrid(dem.x, dem.y)
    o, d = base_rays()
    _, x0, y0, d0, d1 = sc.grid_args(dem)
    t, xyz, patch, status = rr.cast(o, d, a * X + b * Y + c, x0, y0, d0, d1)
    t_plane = (a * o[0] + b * o[1] + c - o[2]) / (d[:, 2] - a * d[:, 0] - b * d[:, 1])
    hit = status == rr.HIT
    assert hit.sum() > 2000
    deviation = np.max(np.abs(t[hit] - t_plane[hit]) / t[hit])
    print(f"tilted plane: {hit.sum()} hits, largest |t - t_plane| / t = {deviation!r}")
    assert deviation <= 8 * PLANE_DEVIATION
    # rays that leave do so because the plane lies beyond the domain or behind them
    leaves = status == rr.LEAVES
    xy_plane = o[0:2] + t_plane[leaves, None] * d[leaves, 0:2]
    outside = (xy_plane[:, 0] < dem.x.min()) | (xy_plane[:, 0] > dem.x.max()) | (xy_plane[:, 1] < dem.y.min()) \
        | (xy_plane[:, 1] > dem.y.max())
    assert (outside | (t_plane[leaves] < 0)).all()


def test_the_hits_of_the_restatement_lie_on_the_surface():
    """The residual the GPU test's bound is made of (HIT_RESIDUAL), measured here."""
    dem = sc.dem()
    o, d = base_rays()
    t, xyz, patch, status = rr.cast(o, d, *sc.grid_args(dem))
    hit = status == rr.HIT
    residual = hit_residual(dem, t, xyz, d, hit).max()
    print(f"largest residual of {hit.sum()} hits: {residual!r} m")
    assert residual == HIT_RESIDUAL


def same(a, b):
    """Bit for bit, NaN for NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and a[~nan].tobytes() == b[~nan].tobytes()


def scenes():
    """(name, origins, directions, grid arguments, correction): the cases of tests/test_gpu_raycast.py that the
    restatement's own two paths are compared on."""
    dem = sc.dem()
    o, d = base_rays()
    yield "base", o, d, sc.grid_args(dem), None
    yield "x descending", o, d, sc.grid_args(sc.dem(x_descending=True)), None
    oo, dd = rr.camera_rays(sc.camera(False, xyz=(-150.0, 60.0, 140.0), viewdir=(80.0, -8.0, 0.0)), sc.pixel_centres())
    yield "outside", oo, dd, sc.grid_args(dem), None
    lo, ld = rr.camera_rays(sc.long_camera(), sc.pixel_centres())
    yield "long, corrected", lo, ld, sc.grid_args(sc.long_dem()), (6.3781e6, 0.13)


@pytest.mark.parametrize("scene", list(scenes()), ids=lambda s: s[0])
def test_the_path_does_not_matter(scene):
    """The restatement with blocks of 16, 4 and 1 patches equals its plain march bit for bit, and skips work."""
    name, o, d, grid, correction = scene
    plain = rr.cast(o, d, *grid, correction=correction, block=0, return_steps=True)
    for block in (16, 4, 1):
        skipped = rr.cast(o, d, *grid, correction=correction, block=block, return_steps=True)
        assert all(same(a, b) for a, b in zip(plain[:4], skipped[:4])), (name, block)
        assert (skipped[4] <= plain[4]).all()
    print(name, "patches evaluated per ray:", plain[4].mean(), "plain,", skipped[4].mean(), "with blocks of 1")


def test_the_correction_moves_hits_to_other_patches():
    """What the corrected case of tests/test_gpu_raycast.py rests on."""
    o, d = rr.camera_rays(sc.long_camera(), sc.pixel_centres())
    grid = sc.grid_args(sc.long_dem())
    with_c, without = rr.cast(o, d, *grid, correction=(6.3781e6, 0.13)), rr.cast(o, d, *grid)
    both = (with_c[3] == rr.HIT) & (without[3] == rr.HIT)
    assert (with_c[2][both] != without[2][both]).sum() >= 1


# ---- the package's host logic, the library call answered by the restatement ---------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    """glimpse_amd with `_lib.stage_raycast` answered by the restatement (undistorted cameras: the unprojection is
    restated on the host): the host logic runs, no device.  Yields the list of the calls' keyword arguments."""
    from glimpse_amd import Camera, _lib

    calls = []

    def stage_raycast(z, x, y, d, origins=None, directions=None, cam=None, uv=None, step=None, correction=None, block=16,
                      device_id=0, return_times=False):
        calls.append(dict(correction=correction, block=block, step=step, z_dtype=np.asarray(z).dtype))
        on, radius, refraction = _lib.viewshed_correction(correction)
        if directions is None:
            v = np.asarray(cam)
            camera = Camera(imgsz=v[6:8], f=v[8:10], c=v[10:12], xyz=v[0:3], viewdir=v[3:6])
            if uv is None:
                uv = rr.grid_uv(camera.imgsz, step).reshape(-1, 2)
            origins, directions = rr.camera_rays(camera, uv)
        return rr.cast(origins, directions, z, float(x[0]), float(y[0]), float(d[0]), float(d[1]),
                       correction=(radius, refraction) if on else None, block=block)

    monkeypatch.setattr(_lib, "stage_raycast", stage_raycast)
    monkeypatch.setattr(_lib, "_lib", None)
    return calls


def test_the_host_logic_returns_the_restatements_results(restated):
    from glimpse_amd import Image

    dem, cam = sc.dem(), sc.camera(False)
    uv = sc.pixel_centres()
    o, d = rr.camera_rays(cam, uv)
    t, xyz, patch, status = rr.cast(o, d, *sc.grid_args(dem))
    got = dem.intersect_rays(o, d)
    assert same(got, xyz) and got.shape == (len(d), 3)
    got = dem.intersect_rays(o, d, return_depth=True, return_status=True, block=0)
    assert same(got[0], xyz) and same(got[1], t) and same(got[2], status) and restated[-1]["block"] == 0
    per_ray = dem.intersect_rays(np.broadcast_to(o, d.shape), d)
    assert same(per_ray, xyz)
    assert same(dem.intersect_rays(o, d[5]), xyz[5:6])  # (one direction (3,) is one ray)
    assert dem.intersect_rays(o, np.empty((0, 3))).shape == (0, 3)
    got = cam.uv_to_dem(uv, dem, return_depth=True, return_status=True)
    assert same(got[0], xyz) and same(got[1], t) and same(got[2], status)
    assert same(cam.uv_to_dem(uv[7], dem), xyz[7:8])
    image = Image(cam=cam, array=np.zeros((sc.IMGSZ[1], sc.IMGSZ[0]), np.uint8), datetime=WHEN)
    assert same(image.uv_to_dem(uv, dem), xyz)
    for step in (1, 4, 5):
        grid_xyz, depth = cam.xyz_map(dem, step=step, return_depth=True)
        rows, cols = sc.IMGSZ[1] // step, sc.IMGSZ[0] // step
        assert grid_xyz.shape == (rows, cols, 3) and depth.shape == (rows, cols) and restated[-1]["step"] == step
        centres = rr.grid_uv(sc.IMGSZ, step)
        assert (centres[0, 0] == step / 2).all() and (centres[1, 2] == (2.5 * step, 1.5 * step)).all()
        want = rr.cast(*rr.camera_rays(cam, centres.reshape(-1, 2)), *sc.grid_args(dem))
        assert same(grid_xyz.reshape(-1, 3), want[1]) and same(depth.ravel(), want[0])
    assert same(cam.xyz_map(dem), xyz.reshape(sc.IMGSZ[1], sc.IMGSZ[0], 3))
    # a float32 DEM travels as float32, any other as float64
    assert restated[-1]["z_dtype"] == np.float64
    sc.dem(np.float32).intersect_rays(o, d)
    assert restated[-1]["z_dtype"] == np.float32
    from glimpse_amd import Raster

    Raster(sc.terrain().astype(np.int32), x=dem.xlim, y=dem.ylim).intersect_rays(o, d)
    assert restated[-1]["z_dtype"] == np.float64


def test_the_host_logic_applies_the_cameras_correction(restated):
    dem = sc.long_dem()
    cam, plain = sc.long_camera(True), sc.long_camera(False)
    uv = sc.pixel_centres()
    o, d = rr.camera_rays(cam, uv)
    with_c = rr.cast(o, d, *sc.grid_args(dem), correction=(6.3781e6, 0.13))
    without = rr.cast(o, d, *sc.grid_args(dem))
    assert not same(with_c[1], without[1])
    assert same(cam.uv_to_dem(uv, dem), with_c[1]) and restated[-1]["correction"] == cam.correction
    assert same(plain.uv_to_dem(uv, dem), without[1])
    assert same(cam.xyz_map(dem).reshape(-1, 3), with_c[1])
    assert same(dem.intersect_rays(o, d, correction=True), with_c[1])
    assert same(dem.intersect_rays(o, d, correction={"radius": 6.3781e6, "refraction": 0.13}), with_c[1])
    other = Camera_with(cam, {"refraction": 0.2})
    got = other.uv_to_dem(uv, dem)
    assert same(got, rr.cast(o, d, *sc.grid_args(dem), correction=(6.3781e6, 0.2))[1]) and not same(got, with_c[1])


def Camera_with(cam, correction):
    other = cam.copy()
    other.correction = {**cam.correction, **correction}
    return other


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """The stage may not be reached, and any attempt to load the HIP library fails (GlhError): an error below was raised
    before both."""
    from glimpse_amd import _lib

    def reached(*args, **kwargs):
        raise AssertionError("the library was called before the arguments were checked")

    monkeypatch.setattr(_lib, "stage_raycast", reached)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def test_every_refusal_comes_before_a_library_call(no_library):
    from glimpse_amd import Image, Raster

    dem, cam = sc.dem(), sc.camera()
    o, d = np.array(sc.XYZ), np.array([[1.0, 1.0, -0.5]])
    uv = sc.pixel_centres()[:4]
    with pytest.raises(NotImplementedError, match="raster grid"):
        Image(cam=Raster(np.zeros((48, 64)), x=(0.0, 64.0), y=(48.0, 0.0)), array=np.zeros((48, 64), np.uint8),
              datetime=WHEN).uv_to_dem(uv, dem)
    for flat in (Raster(np.zeros((1, 9)), x=(0.0, 9.0), y=(1.0, 0.0)), Raster(np.zeros((9, 1)), x=(0.0, 1.0), y=(9.0, 0.0))):
        with pytest.raises(NotImplementedError, match="singleton"):
            flat.intersect_rays(o, d)
        with pytest.raises(NotImplementedError, match="singleton"):
            cam.uv_to_dem(uv, flat)
        with pytest.raises(NotImplementedError, match="singleton"):
            cam.xyz_map(flat)
    layered = Raster(np.zeros((sc.NY, sc.NX, 2)), x=dem.xlim, y=dem.ylim)
    with pytest.raises(ValueError, match="a DEM is two-dimensional"):
        layered.intersect_rays(o, d)
    with pytest.raises(ValueError, match="a DEM is two-dimensional"):
        cam.xyz_map(layered)
    for block in (3, 48, -16):
        with pytest.raises(ValueError, match="block is 0 or a power of two"):
            dem.intersect_rays(o, d, block=block)
        with pytest.raises(ValueError, match="block is 0 or a power of two"):
            cam.uv_to_dem(uv, dem, block=block)
        with pytest.raises(ValueError, match="block is 0 or a power of two"):
            cam.xyz_map(dem, block=block)
    with pytest.raises(ValueError, match=r"directions must be \(n, 3\)"):
        dem.intersect_rays(o, np.zeros((4, 2)))
    with pytest.raises(ValueError, match="origin must be"):
        dem.intersect_rays(np.zeros((2, 3)), np.ones((4, 3)))
    with pytest.raises(ValueError, match=r"uv must be \(n, 2\)"):
        cam.uv_to_dem(np.zeros((4, 3)), dem)
    for step in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="step must be a positive integer"):
            cam.xyz_map(dem, step=step)
    with pytest.raises(ValueError, match="leaves no pixel"):
        cam.xyz_map(dem, step=49)
    with pytest.raises(TypeError):
        dem.intersect_rays(o, d, correction={"radius": 6.3781e6, "altitude": 3.0})
    with pytest.raises(TypeError, match="a DEM of dtype"):
        Raster(np.zeros((4, 4), dtype=complex), x=(0.0, 4.0), y=(4.0, 0.0)).intersect_rays(o, d)


def test_stage_raycast_checks_its_arguments_before_the_library(monkeypatch, tmp_path):
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    z, x, y, d = np.zeros((3, 4)), np.arange(4.0), np.arange(3.0), (1.0, 1.0)
    o, rays = np.zeros(3), np.ones((5, 3))
    cam = np.zeros(_lib.CAM_LEN)
    cam[6:8] = 8, 6
    with pytest.raises(ValueError, match="block is 0 or a power of two"):
        _lib.stage_raycast(z, x, y, d, origins=o, directions=rays, block=12)
    with pytest.raises(ValueError, match="one of directions, uv and step"):
        _lib.stage_raycast(z, x, y, d, origins=o)
    with pytest.raises(ValueError, match="one of directions, uv and step"):
        _lib.stage_raycast(z, x, y, d, origins=o, directions=rays, cam=cam, step=1)
    with pytest.raises(ValueError):
        _lib.stage_raycast(z, x[:3], y, d, origins=o, directions=rays)
    with pytest.raises(ValueError, match="origins must be"):
        _lib.stage_raycast(z, x, y, d, origins=np.zeros((2, 3)), directions=rays)
    with pytest.raises(ValueError, match="uv must be"):
        _lib.stage_raycast(z, x, y, d, cam=cam, uv=np.zeros((5, 3)))
    with pytest.raises(ValueError, match="leaves no pixel"):
        _lib.stage_raycast(z, x, y, d, cam=cam, step=7)
    with pytest.raises(TypeError):
        _lib.stage_raycast(z.astype(np.int32), x, y, d, origins=o, directions=rays)
    with pytest.raises(_lib.GlhError):  # (every argument in order: only now is the library asked for)
        _lib.stage_raycast(z, x, y, d, origins=o, directions=rays)


# ---- the stage without a device ------------------------------------------------------------------------------------------
GLH_E_INVALID, GLH_E_HIP, GLH_E_UNSUPPORTED = -1, -2, -5


def stage_call(lib, **changes):
    """glh_stage_raycast on a valid 2 x 2 job of one ray, with `changes` to its arguments."""
    from glimpse_amd import _lib

    a = dict(z=np.zeros((2, 2)), z_dtype=0, nx=2, ny=2, x=np.array([5.0, 15.0]), y=np.array([15.0, 5.0]), d0=10.0, d1=-10.0,
             mode=0, cam=None, origins=np.array([[10.0, 10.0, 5.0]]), n_origins=1, rays=np.array([[0.1, 0.2, -1.0]]), n=1, step=0,
             correction=0, radius=6.3781e6, refraction=0.13, block=0, t=np.empty(1), xyz=np.empty((1, 3)),
             patch=np.empty(1, np.int32), status=np.empty(1, np.uint8))
    a.update(changes)
    p = _lib._ptr
    return lib.glh_stage_raycast(0, p(a["z"]), a["z_dtype"], a["nx"], a["ny"], p(a["x"]), p(a["y"]), a["d0"], a["d1"], a["mode"],
                                 p(a["cam"]), p(a["origins"]), a["n_origins"], p(a["rays"]), a["n"], a["step"], a["correction"],
                                 a["radius"], a["refraction"], a["block"], p(a["t"]), p(a["xyz"]), p(a["patch"]), p(a["status"]),
                                 None)


def test_the_c_abi_checks_its_arguments_before_a_device():
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    cam = sc.camera().vector24
    grid = cam.copy()
    grid[23] = 1.0
    uv = np.array([[3.5, 2.5]])
    unsupported = dict(
        grid_camera_uv=dict(mode=1, cam=grid, origins=None, rays=uv),
        grid_camera_pixels=dict(mode=2, cam=grid, origins=None, rays=None, step=1, n=64 * 48),
        one_row=dict(ny=1), one_column=dict(nx=1),
        uneven_x=dict(nx=3, z=np.zeros((2, 3)), x=np.array([5.0, 15.0, 28.0])),
        uneven_y=dict(ny=3, z=np.zeros((3, 2)), y=np.array([15.0, 5.0, -8.0])),
        wrong_cell_size=dict(d0=-10.0),
        cells=dict(nx=65536, ny=32768),
        block_3=dict(block=3), block_48=dict(block=48), block_negative=dict(block=-16), block_huge=dict(block=65536),
        mode=dict(mode=3), z_dtype=dict(z_dtype=2),
        pixels=dict(mode=2, cam=np.concatenate((cam[:6], [65536.0, 32768.0], cam[8:])), origins=None, rays=None, step=1, n=1),
    )
    for name, changes in unsupported.items():
        assert stage_call(lib, **changes) == GLH_E_UNSUPPORTED, name
        assert lib.glh_last_error().startswith(b"raycast"), name
    invalid = dict(
        z=dict(z=None), x=dict(x=None), y=dict(y=None), t=dict(t=None), xyz=dict(xyz=None), patch=dict(patch=None),
        status=dict(status=None), origins=dict(origins=None), directions=dict(rays=None),
        no_camera=dict(mode=1, origins=None, rays=uv), no_uv=dict(mode=1, cam=cam, origins=None, rays=None),
        no_rays=dict(n=0), no_columns=dict(nx=0), no_rows=dict(ny=0),
        origins_count=dict(n_origins=2, origins=np.zeros((2, 3))),
        step=dict(mode=2, cam=cam, origins=None, rays=None, step=0, n=64 * 48),
        grid_size=dict(mode=2, cam=cam, origins=None, rays=None, step=1, n=64 * 48 - 1),
        nan_x=dict(x=np.array([5.0, np.nan])), zero_cell=dict(d0=0.0), infinite_cell=dict(d1=np.inf),
        radius=dict(correction=1, radius=0.0),
    )
    for name, changes in invalid.items():
        assert stage_call(lib, **changes) == GLH_E_INVALID, name
        assert lib.glh_last_error().startswith(b"raycast"), name


def test_a_valid_job_reaches_the_stage_file():
    """A valid 2 x 2 job of each mode fails at the first HIP call of glh_raycast.hip where no device is present, with that
    call, the runtime's words, the file and the line in glh_last_error() (tests/test_stage_errors.py asks this of the
    other stages).  Skipped where a device is present: there the calls succeed (tests/test_gpu_raycast.py)."""
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    try:
        if _lib.device_count() >= 1:
            pytest.skip("a device is present: the HIP calls succeed")
    except _lib.GlhError:
        pass
    lib = _lib.load()
    cam = sc.camera().vector24
    for changes in (dict(), dict(block=16), dict(mode=1, cam=cam, origins=None, rays=np.array([[3.5, 2.5]])),
                    dict(mode=2, cam=cam, origins=None, rays=None, step=4, n=16 * 12, t=np.empty(192), xyz=np.empty((192, 3)),
                         patch=np.empty(192, np.int32), status=np.empty(192, np.uint8))):
        assert stage_call(lib, **changes) == GLH_E_HIP
        message = lib.glh_last_error().decode()
        found = re.fullmatch(r"(hip\w+)\(.*\) failed: (.+) \((.+):(\d+)\)", message)
        assert found, message
        assert found.group(3).endswith("glh_raycast.hip") and int(found.group(4)) > 0


# ---- the plane helper ------------------------------------------------------------------------------------------------------
def test_intersect_rays_plane_on_the_four_rays_of_the_reference():
    """The example of the reference's docstring (helpers.py:1053-1101): down from z = 1 meets the xy-plane at the origin; up
    from z = 1 has the plane behind it; along x at z = 1 is parallel; along x at z = 0 lies in the plane, which counts as
    parallel."""
    from glimpse_amd import helpers

    plane = (0, 0, 0, 1, 0, 0, 0, 1, 0)
    rays = [(0, 0, 1, 0, 0, -1), (0, 0, 1, 0, 0, 1), (0, 0, 1, 1, 0, 0), (0, 0, 0, 1, 0, 0)]
    got = helpers.intersect_rays_plane(rays, plane)
    assert got.shape == (4, 3) and (got[0] == 0).all() and np.isnan(got[1:]).all()
    # a tilted plane and an oblique ray, against the closed form; one ray alone is (1, 3)
    got = helpers.intersect_rays_plane((1.0, 2.0, 10.0, 0.5, -0.25, -2.0), (0.0, 0.0, 1.0, 1.0, 0.0, 0.5, 0.0, 1.0, -0.25))
    t = (1.0 + 0.5 * 1.0 - 0.25 * 2.0 - 10.0) / (-2.0 - 0.5 * 0.5 - 0.25 * 0.25)
    assert got.shape == (1, 3) and np.allclose(got[0], (1.0 + 0.5 * t, 2.0 - 0.25 * t, 10.0 - 2.0 * t), rtol=1e-15, atol=0)
