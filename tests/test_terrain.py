"""`Raster.gradient`, `hillshade`, `rasterize_polygons`, `rasterize`, `fill_circle`, `shift`, `data_extent` and
`crop_to_data` without a device: the committed g33 fixture is what the reference writes (regenerated where the reference
is present); the NumPy restatement (tests/terrain_restatement.py) equals its gradients in every bit and its hillshade
within the derived bound; the polygon rule gives the reference's two docstring examples, agrees with
matplotlib.path.Path.contains_points away from the edges and decides the boundary as documented; the host-only companions
equal the fixture cell for cell; what is not served is refused before the library is touched; the built library exports
the three stages and refuses bad arguments without a device.  Every test prints what it measured."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import terrain_restatement as tr
from tests import viewshed_terrain as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G33 = "g33_terrain.npz"


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so whatever passes below happened before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def case_of(name, g):
    """(z, d, hillshade kwargs) of a golden case, the DEM checked against the fixture's SHA-256."""
    z, xlim, ylim, kwargs = tr.build(name)
    assert vt.sha256(z).tobytes() == g[f"{name}__sha256"].tobytes(), name
    return z, tr.cell_sizes(z, xlim, ylim), kwargs


def same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.dtype, want.dtype)
    differing = int((~((got == want) | ((got != got) & (want != want)))).sum())
    print(f"terrain {what}: {differing} of {want.size} cells differ")
    assert differing == 0 and got.tobytes() == want.tobytes(), what


def check_hillshade(name, got, want, z, d, kwargs, who):
    """`got` against the reference's `want`: equal NaN masks, |difference| <= 8 eps / min(1, imax - imin)."""
    raw = tr.raw_intensity(z, d, kwargs.get("azimuth", 315), kwargs.get("altitude", 45), kwargs.get("vert_exag", 1))
    _, imin, imax = tr.stretch(raw, kwargs.get("fraction", 1.0))
    bound = tr.hillshade_bound(imin, imax)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), name
    worst = float(np.max(np.abs(got - want)[~np.isnan(want)]))
    spread = float(imax - imin)
    print(f"hillshade {name} ({who}): imax - imin = {spread:.6g}, max |difference| = {worst / tr.EPS:.3g} eps = "
          f"{worst * min(1.0, spread) / tr.EPS if spread > 1e-6 else worst / tr.EPS:.3g} eps / range (bound 8), "
          f"NaN cells {int(np.isnan(want).sum())}, cells at 0 / 1: {int((want == 0).sum())} / {int((want == 1).sum())}")
    # the inputs are chosen far from the 1e-6 switch of the normalisation: a range of 0 (or NaN), or above 1e-3
    assert np.isnan(spread) or spread == 0.0 or spread > 1e-3, name
    assert worst <= bound, name
    return worst * min(1.0, spread) / tr.EPS if spread > 1e-6 else worst / tr.EPS


# ---- the fixture and the restatement ------------------------------------------------------------------------------------
def test_g33_is_what_the_reference_writes(tmp_path, golden):
    """tools/make_golden.py --g33 run again (in a process of its own: it installs stub modules) gives the committed arrays
    byte for byte.  Needs the reference; elsewhere the fixture is taken as committed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import refstubs  # (importing installs nothing; it knows where the reference would be)
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(refstubs.REFERENCE_SRC, "glimpse")):
        pytest.skip("the reference is not on this machine")
    out = tmp_path / "g33.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden.py"), "--g33", "--out", str(out)], check=True,
                   capture_output=True, timeout=900)
    want, got = golden(G33), dict(np.load(out, allow_pickle=False))
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key].dtype == got[key].dtype and want[key].shape == got[key].shape, key
        assert want[key].tobytes() == got[key].tobytes(), key


def test_the_fixture_holds_the_cases_it_says(golden):
    g = golden(G33)
    assert list(g["cases"]) == tr.GOLDEN_CASES
    shapes = {tr.build(name)[0].shape for name in tr.GOLDEN_CASES}
    assert {(2, 2), (2, 67), (67, 2), (3, 3), tr.TILED} <= shapes
    assert tr.TILED[0] > 2 * tr.TILE[0] and tr.TILED[1] > 2 * tr.TILE[1]
    signs = {tuple(np.sign(case_of(name, g)[1])) for name in tr.GOLDEN_CASES}
    assert signs == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    assert any(abs(d[0]) != abs(d[1]) for d in (case_of(name, g)[1] for name in tr.GOLDEN_CASES))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G33)) < 200_000


@pytest.mark.parametrize("name", tr.GOLDEN_CASES)
def test_restated_gradient_equals_the_reference_bit_for_bit(golden, name):
    g = golden(G33)
    z, d, _ = case_of(name, g)
    dzdx, dzdy = tr.gradient(z, d)
    assert dzdx.dtype == (np.float32 if z.dtype == np.float32 else np.float64)
    same_bytes(dzdx, g[f"{name}__dzdx"], f"{name} dzdx ({z.dtype})")
    same_bytes(dzdy, g[f"{name}__dzdy"], f"{name} dzdy ({z.dtype})")


def test_restated_hillshade_is_within_the_bound_of_the_reference(golden):
    """Measured: the largest deviation over the cases is 1.5 eps / range (bound 8)."""
    g = golden(G33)
    worst = 0.0
    for name in tr.GOLDEN_CASES:
        z, d, kwargs = case_of(name, g)
        worst = max(worst, check_hillshade(name, tr.hillshade(z, d, **kwargs), g[f"{name}__hillshade"], z, d, kwargs,
                                           "restatement"))
    print(f"hillshade: the largest deviation of the restatement from the reference is {worst:.3g} eps / range")


def test_hillshade_keeps_the_quirks_of_the_reference(golden):
    g = golden(G33)
    for name, cell in ((tr.case_name("nan_interior", tr.SMALL), (tr.SMALL[0] // 2, tr.SMALL[1] // 2 + 1)),
                       (tr.case_name("nan_corner", tr.SMALL), (tr.SMALL[0] - 1, 0))):
        z, d, kwargs = case_of(name, g)
        want = g[f"{name}__hillshade"]
        r, c = cell
        assert np.isnan(z[r, c]) and np.isnan(z).sum() == 1
        neighbours = [(r + dr, c + dc) for dr, dc in ((-1, 0), (1, 0), (0, -1), (0, 1))
                      if 0 <= r + dr < z.shape[0] and 0 <= c + dc < z.shape[1]]
        nan_cells = {tuple(int(v) for v in rc) for rc in np.argwhere(np.isnan(want))}
        # the central difference does not read the cell itself: its edge neighbours are NaN, and it is only where it ends a line
        on_an_edge = r in (0, z.shape[0] - 1) or c in (0, z.shape[1] - 1)
        assert nan_cells == set(neighbours) | ({(r, c)} if on_an_edge else set()), name
        # no normalisation with a NaN cell: the values are the clipped raw intensity
        raw = tr.raw_intensity(z, d)
        assert np.nanmax(np.abs(np.clip(raw, 0, 1) - want)) <= 8 * tr.EPS
    z, d, kwargs = case_of(tr.case_name("constant", tr.SMALL), g)
    want = g[f"{tr.case_name('constant', tr.SMALL)}__hillshade"]
    assert np.ptp(want) == 0 and abs(want[0, 0] - np.sin(np.radians(45))) <= 2 * tr.EPS  # flat: the sine of the altitude


# ---- the polygon rule -----------------------------------------------------------------------------------------------------
def test_polygon_rule_gives_the_examples_of_the_reference():
    e = tr.DOCTEST_HELPER
    assert np.array_equal(tr.polygons_to_mask(e["polygons"], e["size"], e["holes"]), e["want"])
    assert np.array_equal(tr.polygons_to_mask(tr.DOCTEST_RASTER["polygons"], (3, 3)), tr.DOCTEST_RASTER["want"])


@pytest.mark.parametrize("seed,size,n", [(3341, (13, 9), 3), (3342, (40, 37), 8), (3343, (130, 70), 25), (3344, (33, 65), 12)])
def test_polygon_rule_agrees_with_matplotlib_away_from_the_edges(seed, size, n):
    from matplotlib.path import Path

    polygons, holes = tr.star_scene(seed, size, n)
    distance = tr.distance_to_edges(polygons + holes, size)
    assert distance > 1e-9  # no centre on or next to an edge: the boundary rule is not in play
    nx, ny = size
    centres = np.column_stack([v.ravel() for v in np.meshgrid(np.arange(nx) + 0.5, np.arange(ny) + 0.5)])
    inside = lambda rings: np.any([Path(ring).contains_points(centres) for ring in rings], axis=0).reshape(ny, nx)  # noqa: E731
    want = inside(polygons) & ~(inside(holes) if holes else False)
    got = tr.polygons_to_mask(polygons, size, holes)
    print(f"polygons seed {seed}: {len(polygons)} polygons, {len(holes)} holes on {ny} x {nx}: {int(got.sum())} cells inside, "
          f"nearest centre {distance:.3g} from an edge, {int((got != want).sum())} cells differ from matplotlib")
    assert 0 < got.sum() < got.size and np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(tr.BOUNDARY))
def test_polygon_rule_on_the_boundary(name):
    polygons, size, want = tr.BOUNDARY[name]
    assert np.array_equal(tr.polygons_to_mask(polygons, size), want)


# ---- the host-only companions ------------------------------------------------------------------------------------------
def test_bresenham_circle():
    from glimpse_amd import helpers

    want = np.array([[0, 1], [1, 1], [1, 0], [1, -1], [0, -1], [-1, -1], [-1, 0], [-1, 1], [0, 1]], dtype=float)
    got = helpers.bresenham_circle((0, 0), 1)  # (the reference's docstring example)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(helpers.bresenham_circle((4, -2), 0), [[4.0, -2.0]])
    ring = helpers.bresenham_circle((10, 20), 7)
    assert np.array_equal(ring[0], ring[-1]) and (np.abs(np.diff(ring, axis=0)).max(axis=1) == 1).all()
    assert np.abs(np.hypot(ring[:, 0] - 10, ring[:, 1] - 20) - 7).max() < 1
    with pytest.raises(ValueError):
        helpers.bresenham_circle((0, 0), -2)


@pytest.mark.parametrize("name", sorted(tr.CIRCLES))
def test_fill_circle_equals_the_reference(golden, no_library, name):
    from glimpse_amd import Raster

    xlim, ylim, centre, radius = tr.CIRCLES[name]
    dem = Raster(np.zeros(tr.CIRCLE_SHAPE), x=xlim, y=ylim)
    assert dem.fill_circle(centre, radius) is None
    want = golden(G33)[f"circle_{name}"]
    print(f"fill_circle {name}: radius {np.round(radius / dem.d[0]):.0f} cells, {int(np.isnan(want).sum())} cells filled")
    same_bytes(dem.array, want, name)


def test_fill_circle_value_and_negative_cell_size(golden, no_library):
    from glimpse_amd import Raster

    g = golden(G33)
    dem = Raster(np.arange(180).reshape(tr.CIRCLE_SHAPE), x=tr.CIRCLE_X, y=tr.CIRCLE_Y_DESC)
    dem.fill_circle((72.0, 63.0), 30.0, value=-7)
    same_bytes(dem.array, g["circle_int_value"], "an int raster filled with -7")
    assert list(g["circle_negative_d0__raises"]) == ["ValueError"]
    with pytest.raises(ValueError):
        Raster(np.zeros(tr.CIRCLE_SHAPE), x=tr.CIRCLE_X_DESC, y=tr.CIRCLE_Y_DESC).fill_circle((72.0, 63.0), 20.0)


def test_shift_data_extent_and_crop_to_data_equal_the_reference(golden, no_library):
    from glimpse_amd import Raster

    g = golden(G33)
    z, xlim, ylim = tr.holey()
    assert vt.sha256(z).tobytes() == g["holey__sha256"].tobytes()
    dem = Raster(z.copy(), x=xlim, y=ylim)
    rows, cols = dem.data_extent()
    assert [rows.start, rows.stop, cols.start, cols.stop] == list(g["extent"]) == [2, 8, 3, 9]
    assert dem.crop_to_data() is None
    same_bytes(dem.array, g["crop_to_data__array"], "crop_to_data")
    assert np.array_equal(np.concatenate((dem.xlim, dem.ylim)), g["crop_to_data__limits"])
    assert tuple(dem.size) == (6, 6) and dem.shape == (6, 6)
    with pytest.raises(ValueError, match=str(g["extent_all_nan__raises"][0])):
        Raster(np.full((3, 4), np.nan)).data_extent()
    dem = Raster(z.copy(), x=xlim, y=ylim)
    assert dem.shift(1.5, -2.0, 3.25) is None
    same_bytes(dem.array, g["shift__array"], "shift")
    assert np.array_equal(np.concatenate((dem.xlim, dem.ylim)), g["shift__limits"])
    dem.shift(dy=0.5)
    assert np.array_equal(np.concatenate((dem.xlim, dem.ylim)), g["shift_dy__limits"])
    same_bytes(dem.array, g["shift__array"], "shift without dz")


def rasterize_with_host_means(monkeypatch, dtype):
    """Raster.rasterize with `glh_stage_rasterize` replaced by its definition (ordered float64 sums times 1 / count): what
    the host does around the device call."""
    from glimpse_amd import Raster, _lib

    def host_means(keys, values, n_pixels, **_):
        sums, counts = np.zeros(n_pixels), np.zeros(n_pixels)
        for k, v in zip(keys, values[:, 0]):
            sums[k] += v
            counts[k] += 1
        with np.errstate(all="ignore"):
            return (sums * (1 / counts))[:, None]

    monkeypatch.setattr(_lib, "stage_rasterize", host_means)
    array, xlim, ylim, xy, values = tr.rasterize_case(dtype)
    dem = Raster(array.copy(), x=xlim, y=ylim)
    result = dem.rasterize(xy, values)
    assert np.array_equal(dem.array, array)  # (a copy: the raster keeps its values)
    return result, array


@pytest.mark.parametrize("dtype", ["float64", "float32", "int64"])
def test_rasterize_host_part_equals_the_reference(golden, no_library, monkeypatch, dtype):
    result, array = rasterize_with_host_means(monkeypatch, dtype)
    want = golden(G33)[f"rasterize_{dtype}"]
    written = ~((want == array) | (want != want))
    print(f"rasterize {dtype}: {int(written.sum())} cells take a mean, {int((want != want).sum())} a NaN mean")
    same_bytes(result, want, f"rasterize {dtype}")
    if dtype != "int64":
        assert (want != want).sum() == 1 and not (array != array).any()  # a mean of NaN values, told from no point


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_library(no_library):
    from glimpse_amd import Raster, helpers
    from glimpse_amd._lib import GlhError

    dem = Raster(vt.terrain((6, 8), 3399), x=(0.0, 80.0), y=(60.0, 0.0))
    for name in ("dx", "dy"):
        with pytest.raises(TypeError, match=f"multiple values for keyword argument '{name}'"):
            dem.hillshade(**{name: 1.0})
    with pytest.raises(TypeError, match="unexpected keyword argument 'blend_mode'"):
        dem.hillshade(blend_mode="soft")
    with pytest.raises(TypeError, match="unexpected keyword argument 'azdeg'"):
        dem.hillshade(azdeg=10)
    for shape in ((1, 5), (5, 1), (1, 1)):
        for call in (lambda r: r.gradient(), lambda r: r.hillshade()):
            with pytest.raises(ValueError, match="too small to calculate a numerical gradient"):
                call(Raster(np.zeros(shape)))
    with pytest.raises(ValueError, match="two-dimensional"):
        Raster(np.zeros((4, 5, 3))).gradient()
    with pytest.raises(NotImplementedError, match="float16"):
        Raster(np.zeros((4, 5), dtype=np.float16)).gradient()
    square = [(1.0, 1.0), (4.0, 1.0), (4.0, 4.0)]
    for bad, match in (([[(1.0, 1.0), (2.0, 2.0)]], "at least three"), ([square[:2] + [(np.nan, 1.0)]], "not finite"),
                       ([square[:2] + [(np.inf, 1.0)]], "not finite"), ([[(1.0, 2.0, 3.0)] * 3], "pairs")):
        with pytest.raises(ValueError, match=match):
            helpers.polygons_to_mask(bad, (5, 5))
        with pytest.raises(ValueError, match=match):
            helpers.polygons_to_mask([square], (5, 5), holes=bad)
        with pytest.raises(ValueError, match=match):
            dem.rasterize_polygons(bad)
    with pytest.raises(ValueError, match="at least one cell"):
        helpers.polygons_to_mask([square], (0, 5))
    with pytest.raises(ValueError, match="one value per point"):
        dem.rasterize(np.zeros((3, 2)), np.zeros(4))
    # nothing to burn, nothing to average: answered on the host
    assert not helpers.polygons_to_mask([], (5, 4)).any() and helpers.polygons_to_mask([], (5, 4)).shape == (4, 5)
    assert np.array_equal(dem.rasterize(np.array([[-5.0, 3.0]]), np.array([1.0])), dem.array)
    # and what is served does reach for the library
    for call in (dem.gradient, dem.hillshade, lambda: dem.rasterize_polygons([square])):
        with pytest.raises(GlhError):
            call()


def test_the_library_refuses_what_the_kernels_do_not_take():
    """The three stages are exported and check their arguments before they touch a device."""
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    for name in ("glh_stage_gradient", "glh_stage_hillshade", "glh_stage_polygon_mask"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    z, out, out2 = np.zeros((4, 5)), np.zeros((4, 5)), np.zeros((4, 5))
    light = tr.light_direction(315, 45)
    ptr = _lib._ptr

    def gradient(z=z, dtype=0, nx=5, ny=4, d0=10.0, d1=-10.0, dzdx=out, dzdy=out2):
        return lib.glh_stage_gradient(0, ptr(z), dtype, nx, ny, d0, d1, ptr(dzdx), ptr(dzdy), None)

    def hillshade(z=z, dtype=0, nx=5, ny=4, d0=10.0, d1=10.0, ve=1.0, light=light, fraction=1.0, out=out):
        return lib.glh_stage_hillshade(0, ptr(z), dtype, nx, ny, d0, d1, ve, ptr(light), fraction, ptr(out), None)

    xy = np.array([[1.0, 1.0], [4.0, 1.0], [4.0, 4.0], [1.0, 4.0], [2.0, 2.0], [3.0, 2.0], [3.0, 3.0]])
    off = np.array([0, 4, 7], dtype=np.int32)
    mask = np.zeros((5, 5), dtype=np.uint8)

    def polygons(xy=xy, n=7, off=off, n_polygons=1, n_holes=1, nx=5, ny=5, out=mask):
        return lib.glh_stage_polygon_mask(0, ptr(xy), n, ptr(off), n_polygons, n_holes, nx, ny, ptr(out), None)

    INVALID, UNSUPPORTED = -1, -5
    assert gradient(z=None) == INVALID and "null" in lib.glh_last_error().decode()
    assert gradient(dzdx=None) == INVALID and gradient(dzdy=None) == INVALID
    assert hillshade(z=None) == INVALID and hillshade(light=None) == INVALID and hillshade(out=None) == INVALID
    assert gradient(nx=1) == INVALID and gradient(ny=1) == INVALID and hillshade(nx=0) == INVALID and hillshade(ny=1) == INVALID
    assert gradient(nx=65536, ny=32768) == INVALID and "2^31" in lib.glh_last_error().decode()
    assert hillshade(nx=65536, ny=32768) == INVALID and polygons(nx=65536, ny=32768) == INVALID
    for bad in (0.0, np.nan, np.inf):
        assert gradient(d0=bad) == INVALID and gradient(d1=bad) == INVALID and hillshade(d0=bad) == INVALID
        assert hillshade(d1=-bad) == INVALID and "cell sizes" in lib.glh_last_error().decode()
    assert gradient(dtype=2) == UNSUPPORTED and hillshade(dtype=-1) == UNSUPPORTED and "dtype" in lib.glh_last_error().decode()
    assert hillshade(ve=np.nan) == INVALID and hillshade(fraction=np.inf) == INVALID
    assert hillshade(light=np.array([0.0, np.nan, 1.0])) == INVALID and "finite" in lib.glh_last_error().decode()
    assert polygons(xy=None) == INVALID and polygons(off=None) == INVALID and polygons(out=None) == INVALID
    assert polygons(nx=0) == INVALID and polygons(ny=0) == INVALID
    assert polygons(n=0) == INVALID and polygons(n_polygons=0, n_holes=2) == INVALID and polygons(n_holes=-1) == INVALID
    assert polygons(off=np.array([1, 4, 7], dtype=np.int32)) == INVALID and polygons(n=6) == INVALID
    assert polygons(off=np.array([0, 5, 7], dtype=np.int32)) == INVALID and "at least three" in lib.glh_last_error().decode()
    assert polygons(off=np.array([0, 9, 7], dtype=np.int32)) == INVALID
    bad = xy.copy()
    bad[5, 1] = np.inf
    assert polygons(xy=bad) == INVALID and "not finite" in lib.glh_last_error().decode()
