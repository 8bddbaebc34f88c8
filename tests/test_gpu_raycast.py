"""Rays cast onto a DEM on the device (`glh_stage_raycast`, kernels `k_raycast` and `k_rc_block_max`), through `_lib` and
the Python API, against the restatement of the rule in tests/raycast_rule.py.

In explicit-directions mode the device and the restatement get the same origins, directions and DEM, and t, xyz, patch
and status must agree bit for bit (NaN for NaN), no ray left out, whether the device marches every patch (block = 0) or
skips blocks of 16.  The other two ray sources are held to that mode: `uv` mode to directions mode fed with the existing
unprojection stage's directions, the pixel-grid mode to `uv` mode on the same pixel centres.  Two cross-checks against
existing stages need bounds; where they come from (neither was fitted to the kernel):

* hits lie on the surface: |z_hit - dem.sample(xy_hit, order=1)| stays within 4 x the residual the restatement's own
  hits show against scipy's bilinear interpolator on the CPU (tests/test_raycast.py: HIT_RESIDUAL, 1.71e-13 m); the 4
  covers the two roundings of o + t d and the sampler's own.
* round trip: `cam.xyz_to_uv(cam.uv_to_dem(uv, dem))` returns uv within 4 x the deviation the existing
  `stage_unproject` -> `stage_project` pair shows on the same uv at depth 1, measured in the test.

The scenes are tests/raycast_scene.py's: 37 x 29 cells (more than one block of 16 patches each way, a multiple of 16
on neither) and a distorted 64 x 48 camera inside the DEM's rectangle.
"""
import numpy as np
import pytest

from tests import raycast_rule as rr
from tests import raycast_scene as sc
from tests.test_raycast import HIT_RESIDUAL, same

pytestmark = pytest.mark.gpu

NAMES = ("t", "xyz", "patch", "status")


def device(dem, o, d, correction=None, block=16, **kwargs):
    from glimpse_amd import _lib

    z = dem.array if dem.array.dtype == np.float32 else np.asarray(dem.array, dtype=np.float64)
    return _lib.stage_raycast(z, dem.x, dem.y, dem.d, origins=o, directions=d, correction=correction, block=block, **kwargs)


def agree(dem, o, d, correction=None, blocks=(0, 16)):
    """The device at every block size against the restatement's plain march; returns the restatement's results."""
    want = rr.cast(o, d, *sc.grid_args(dem), correction=None if correction is None else (correction["radius"],
                                                                                       correction["refraction"]))
    assert want[2].dtype == np.int32 and want[3].dtype == np.uint8
    for block in blocks:
        got = device(dem, o, d, correction=correction, block=block)
        for name, g, w in zip(NAMES, got, want):
            assert same(g, w), (name, block, int((~((g == w) | (np.isnan(g) & np.isnan(w)))).sum()))
    return want


def counts(status):
    return dict(zip(rr.STATUS, np.bincount(status, minlength=5)))


@pytest.fixture(scope="module")
def base():
    """The base case: the distorted camera's 3072 pixel centres, their directions from the existing unprojection stage,
    and the restatement's results, computed once."""
    from glimpse_amd import _lib

    cam, dem = sc.camera(), sc.dem()
    uv = sc.pixel_centres()
    d = _lib.stage_unproject(cam.vector24, uv)
    o = np.array(cam.xyz)
    want = rr.cast(o, d, *sc.grid_args(dem))
    return {"cam": cam, "dem": dem, "uv": uv, "o": o, "d": d, "want": want}


def test_the_base_case_equals_the_restatement_at_both_block_sizes(base):
    want = agree(base["dem"], base["o"], base["d"])
    assert all(same(a, b) for a, b in zip(want, base["want"]))
    print(counts(want[3]))
    hits = want[3] == rr.HIT
    assert hits.sum() > 2000 and (want[3] == rr.LEAVES).sum() > 100 and len(np.unique(want[2][hits])) > 300
    # more than one block of 16 patches is hit on both axes
    rows, cols = want[2][hits] // (sc.NX - 1), want[2][hits] % (sc.NX - 1)
    assert len(np.unique(rows // 16)) == 2 and len(np.unique(cols // 16)) == 3
    for block in (1, 4, 64):  # (a block of one patch, one that tiles unevenly, one larger than the DEM)
        agree(base["dem"], base["o"], base["d"], blocks=(block,))


@pytest.mark.parametrize("variant", [dict(x_descending=True), dict(y_ascending=True), dict(x_descending=True, y_ascending=True),
                                     dict(dtype=np.float32)], ids=lambda v: "-".join(v))
def test_dem_variants(base, variant):
    """The same world with the array stored the other way round, and as float32: the hits are the base case's own on the
    flipped rasters, to the rounding of the grid coordinates (the patch indices count from the other end)."""
    dem = sc.dem(**variant)
    want = agree(dem, base["o"], base["d"])
    if "dtype" in variant:
        return
    both = (want[3] == rr.HIT) & (base["want"][3] == rr.HIT)
    assert both.sum() >= (base["want"][3] == rr.HIT).sum() - 3
    assert np.abs(want[1][both] - base["want"][1][both]).max() < 1e-6
    rows, cols = want[2][both] // (sc.NX - 1), want[2][both] % (sc.NX - 1)
    brows, bcols = base["want"][2][both] // (sc.NX - 1), base["want"][2][both] % (sc.NX - 1)
    moved = (np.abs((sc.NX - 2 - cols if variant.get("x_descending") else cols) - bcols) > 1) \
        | (np.abs((sc.NY - 2 - rows if variant.get("y_ascending") else rows) - brows) > 1)
    assert not moved.any()


PLACEMENTS = {
    # outside the rectangle, looking in through its west edge: some rays enter below the terrain's rim
    "outside": ((-150.0, 60.0, 140.0), (80.0, -8.0, 0.0), {rr.HIT, rr.BELOW, rr.LEAVES}),
    "below the surface": ((120.0, 120.0, 90.0), (40.0, 5.0, 0.0), {rr.BELOW}),
    "misses the domain": ((-200.0, -200.0, 300.0), (250.0, -10.0, 0.0), {rr.MISS}),
    "towards the sky": (sc.XYZ, (52.0, 35.0, 0.0), {rr.LEAVES}),
}


@pytest.mark.parametrize("name", list(PLACEMENTS))
def test_camera_placements(name):
    from glimpse_amd import _lib

    xyz, viewdir, statuses = PLACEMENTS[name]
    cam = sc.camera(xyz=xyz, viewdir=viewdir)
    d = _lib.stage_unproject(cam.vector24, sc.pixel_centres())
    want = agree(sc.dem(), np.array(cam.xyz), d)
    print(name, counts(want[3]))
    assert set(want[3]) == statuses


def test_degenerate_rays():
    """An axis-parallel ray along each axis (dp == 0, dq == 0 exactly), vertical rays, rays from a cell centre along the
    grid's diagonals, where every crossing is a tie, and rays that are no rays."""
    dem = sc.dem()
    z, x0, y0, d0, d1 = sc.grid_args(dem)
    a, b = (x0 + 3 * d0, y0 + 4 * d1, 230.0), (x0 + 30 * d0, y0 + 22 * d1, 260.0)
    rays = [
        (a, (1.0, 0.0, -0.45), rr.HIT), (a, (0.0, -1.0, -0.5), rr.HIT), (a, (0.0, 1.0, -0.2), rr.LEAVES),
        (a, (0.0, 0.0, -1.0), rr.HIT), (a, (0.0, 0.0, 1.0), rr.LEAVES), ((a[0], a[1], 50.0), (0.0, 0.0, 1.0), rr.BELOW),
        (a, (d0, d1, -4.5), rr.HIT), (b, (-d0, -d1, -8.0), rr.HIT), (a, (-d0, d1, -7.0), rr.LEAVES),
        (b, (d0, -d1, -3.0), None), (b, (-d0, d1, -3.0), None),
        (a, (np.nan, 0.0, 0.0), rr.INVALID), (a, (0.0, 0.0, 0.0), rr.INVALID), (a, (np.inf, 1.0, 1.0), rr.INVALID),
        (a, (1.0, -np.inf, 0.0), rr.INVALID), ((np.nan, a[1], a[2]), (1.0, 0.0, -0.45), rr.INVALID),
        ((a[0], np.inf, a[2]), (1.0, 0.0, -0.45), rr.INVALID), (a, (1e-320, 1.0, -0.5), None),
    ]
    o, d = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    want = agree(dem, o, d, blocks=(0, 16, 1))
    print([rr.STATUS[s] for s in want[3]])
    for k, (_, _, status) in enumerate(rays):
        assert status is None or want[3][k] == status, (k, rr.STATUS[want[3][k]])
    assert np.isnan(want[0][want[3] != rr.HIT]).all() and (want[2][want[3] != rr.HIT] == -1).all()
    # the diagonal rays: dp == dq, so every crossing is a tie and the patches hit lie on the diagonal through the origin's
    t, xyz, patch, status = want
    for k, (col, row) in ((6, (3, 4)), (7, (30, 22))):
        i, j = patch[k] % (sc.NX - 1), patch[k] // (sc.NX - 1)
        assert abs(i - col) == abs(j - row) and abs(i - col) > 3


def test_a_block_of_nan_cells_in_front_of_a_slope(base):
    z = sc.terrain().copy()
    z[12:19, 12:20] = np.nan
    dem = sc.dem(z=z)
    want = agree(dem, base["o"], base["d"], blocks=(0, 16, 4))
    was = base["want"]
    through = (was[3] == rr.HIT) & (want[3] == rr.HIT) & (was[2] != want[2])
    print(f"{through.sum()} rays pass through the NaN cells and hit the slope behind them")
    assert through.sum() > 100 and (want[0][through] > was[0][through]).all()
    rows, cols = want[2][want[3] == rr.HIT] // (sc.NX - 1), want[2][want[3] == rr.HIT] % (sc.NX - 1)
    assert not ((rows >= 11) & (rows < 19) & (cols >= 11) & (cols < 20)).any()  # (no patch with a NaN corner is hit)


def test_the_elevation_correction():
    from glimpse_amd import _lib

    dem, cam = sc.long_dem(), sc.long_camera(True)
    d = _lib.stage_unproject(cam.vector24, sc.pixel_centres())
    o = np.array(cam.xyz)
    with_c = agree(dem, o, d, correction=cam.correction)
    without = agree(dem, o, d)
    both = (with_c[3] == rr.HIT) & (without[3] == rr.HIT)
    print(counts(with_c[3]), f"{(with_c[2][both] != without[2][both]).sum()} hits in another patch than without")
    assert (with_c[2][both] != without[2][both]).sum() >= 1
    # the API passes the camera's own correction
    xyz = cam.uv_to_dem(sc.pixel_centres(), dem)
    assert same(xyz, with_c[1])


@pytest.mark.parametrize("n", [1, 70000])
def test_ray_counts(n):
    """One ray, and more than a workgroup's worth that is no multiple of 64, each with its own origin."""
    rng = np.random.default_rng(3)
    o = np.column_stack((rng.uniform(-50, 420, n), rng.uniform(-50, 340, n), rng.uniform(120, 400, n)))
    d = rng.normal(size=(n, 3))
    d[:, 2] = -0.3 * np.abs(d[:, 2])
    want = agree(sc.dem(), o, d)
    if n > 1:
        print(counts(want[3]))
        assert all((want[3] == s).sum() > 1000 for s in (rr.HIT, rr.MISS, rr.BELOW, rr.LEAVES))


def test_two_calls_return_the_same_bytes(base):
    first = device(base["dem"], base["o"], base["d"])
    second = device(base["dem"], base["o"], base["d"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))


def test_uv_mode_equals_directions_mode(base):
    from glimpse_amd import _lib

    cam, dem = base["cam"], base["dem"]
    for block in (0, 16):
        got = _lib.stage_raycast(dem.array, dem.x, dem.y, dem.d, cam=cam.vector24, uv=base["uv"], block=block)
        for name, g, w in zip(NAMES, got, base["want"]):
            assert same(g, w), (name, block)
    # through the API, with what it returns on request; a uv that is not finite is an invalid ray
    uv = np.vstack((base["uv"][:100], [[np.nan, 3.0], [np.inf, 3.0]]))
    xyz, depth, status = cam.uv_to_dem(uv, dem, return_depth=True, return_status=True)
    assert same(xyz[:100], base["want"][1][:100]) and same(depth[:100], base["want"][0][:100])
    assert (status[:100] == base["want"][3][:100]).all() and (status[100:] == rr.INVALID).all() and np.isnan(xyz[100:]).all()


@pytest.mark.parametrize("step", [1, 4, 5])
def test_grid_mode_equals_uv_mode(base, step):
    """The pixel grid made on the device against the same pixel centres uploaded: step 1 is the base case; step 4 and 5
    leave 16 x 12 and 12 x 9 pixels, a tile of 16 x 16 cut on one axis and on both."""
    from glimpse_amd import _lib

    cam, dem = base["cam"], base["dem"]
    centres = rr.grid_uv(sc.IMGSZ, step)
    rows, cols = centres.shape[:2]
    by_uv = _lib.stage_raycast(dem.array, dem.x, dem.y, dem.d, cam=cam.vector24, uv=centres.reshape(-1, 2))
    for block in (0, 16):
        got = _lib.stage_raycast(dem.array, dem.x, dem.y, dem.d, cam=cam.vector24, step=step, block=block)
        for name, g, w in zip(NAMES, got, by_uv):
            assert same(g, w), (name, step, block)
    if step == 1:
        assert all(same(g, w) for g, w in zip(by_uv, base["want"]))
    xyz, depth = cam.xyz_map(dem, step=step, return_depth=True)
    assert xyz.shape == (rows, cols, 3) and depth.shape == (rows, cols)
    assert same(xyz.reshape(-1, 3), by_uv[1]) and same(depth.ravel(), by_uv[0])


def test_hits_lie_on_the_surface(base):
    """Against the existing sampler: the bilinear surface Raster.sample(order=1) returns at the hits' xy."""
    cam, dem = base["cam"], base["dem"]
    xyz, status = cam.uv_to_dem(base["uv"], dem, return_status=True)
    hits = status == rr.HIT
    assert same(xyz, base["want"][1]) and hits.sum() > 2000
    residual = np.abs(xyz[hits, 2] - dem.sample(xyz[hits, 0:2], order=1))
    print(f"largest |z_hit - dem.sample(xy_hit)| of {hits.sum()} hits: {residual.max():.3e} m; the restatement's own on the "
          f"CPU: {HIT_RESIDUAL:.3e} m")
    assert residual.max() <= 4 * HIT_RESIDUAL


def test_round_trip(base):
    from glimpse_amd import _lib

    cam, dem, uv = base["cam"], base["dem"], base["uv"]
    xyz, status = cam.uv_to_dem(uv, dem, return_status=True)
    hits = status == rr.HIT
    back = cam.xyz_to_uv(xyz[hits])
    pair = _lib.stage_project(cam.vector24, _lib.stage_unproject(cam.vector24, uv[hits], directions=False))
    allowed = np.abs(pair - uv[hits]).max()
    print(f"round trip of {hits.sum()} hits: {np.abs(back - uv[hits]).max():.3e} px; unproject -> project at depth 1: "
          f"{allowed:.3e} px")
    assert allowed > 0 and np.abs(back - uv[hits]).max() <= 4 * allowed


def test_stage_times(base):
    """As tests/test_gpu_stage_times.py asks of the other stages: the times are named, finite and not negative, the copies
    and the march take some time, so does the pyramid where there is one, and the results are those of the call without times."""
    import math

    from glimpse_amd import _lib

    for block in (0, 16):
        *result, times = device(base["dem"], base["o"], base["d"], block=block, return_times=True)
        print(block, times)
        assert tuple(times) == _lib.RAYCAST_TIMES
        assert all(math.isfinite(v) and v >= 0.0 for v in times.values())
        assert times["upload_ms"] + times["download_ms"] > 0.0 and times["march_ms"] > 0.0
        assert times["pyramid_ms"] > 0.0 or not block
        assert all(same(a, b) for a, b in zip(result, base["want"]))
