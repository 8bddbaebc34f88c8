"""`Raster.gradient`, `hillshade`, `rasterize_polygons` / `helpers.polygons_to_mask` and `rasterize` on the device, through
the Python API and so through the C ABI (`glh_stage_gradient`, `glh_stage_hillshade`, `glh_stage_polygon_mask`,
`glh_stage_rasterize`; the kernels of glh_terrain.hip).

Expected: the NumPy restatement (tests/terrain_restatement.py) bit for bit, NaN for NaN -- the kernels do the same
operations in the same order with no contraction, so no tolerance is taken -- the reference's own answers
(tests/golden/g33_terrain.npz) bit for bit for the gradients and within the bound of tests/test_terrain.py for the
hillshade, and the same bytes on a second call.  The shapes are the smallest at which a tiled stencil can go wrong: lines
of two and three cells, and one cell more than two tiles each way.  Every test prints what it measured.
"""
import numpy as np
import pytest

from tests import project_dem_restatement as pr
from tests import terrain_restatement as tr
from tests.test_terrain import G33, case_of, check_hillshade, same_bytes

pytestmark = pytest.mark.gpu


def raster_of(name):
    from glimpse_amd import Raster

    z, xlim, ylim, kwargs = tr.build(name)
    return Raster(z, x=xlim, y=ylim), kwargs


@pytest.mark.parametrize("name", tr.GOLDEN_CASES + tr.TILED_CASES)
def test_gradient_equals_the_restatement_and_the_reference(golden, name):
    dem, _ = raster_of(name)
    dzdx, dzdy = dem.gradient()
    want_x, want_y = tr.gradient(dem.array, dem.d)
    same_bytes(dzdx, want_x, f"{name} dzdx, device against the restatement")
    same_bytes(dzdy, want_y, f"{name} dzdy, device against the restatement")
    if name in tr.GOLDEN_CASES:
        g = golden(G33)
        case_of(name, g)
        same_bytes(dzdx, g[f"{name}__dzdx"], f"{name} dzdx, device against the reference")
        same_bytes(dzdy, g[f"{name}__dzdy"], f"{name} dzdy, device against the reference")
    again = dem.gradient()
    assert again[0].tobytes() == dzdx.tobytes() and again[1].tobytes() == dzdy.tobytes()  # two calls, the same bytes


@pytest.mark.parametrize("name", tr.GOLDEN_CASES + tr.TILED_CASES)
def test_hillshade_equals_the_restatement_and_is_within_the_bound_of_the_reference(golden, name):
    dem, kwargs = raster_of(name)
    got = dem.hillshade(**kwargs)
    same_bytes(got, tr.hillshade(dem.array, dem.d, **kwargs), f"{name} hillshade, device against the restatement")
    if name in tr.GOLDEN_CASES:
        g = golden(G33)
        z, d, _ = case_of(name, g)
        check_hillshade(name, got, g[f"{name}__hillshade"], z, d, kwargs, "device")
    assert dem.hillshade(**kwargs).tobytes() == got.tobytes()  # two calls, the same bytes


def test_hillshade_spans_zero_to_one_and_clips():
    dem, kwargs = raster_of(tr.case_name("fraction_1p5", tr.TILED))
    plain, scaled = dem.hillshade(), dem.hillshade(**kwargs)
    assert plain.min() == 0.0 and plain.max() == 1.0
    assert scaled.max() == 1.0 and (scaled == 1.0).sum() > 100 and scaled.min() >= 0.0  # the clip is active
    dem, _ = raster_of(tr.case_name("constant", tr.TILED))
    flat = dem.hillshade()
    assert np.ptp(flat) == 0.0 and flat[0, 0] == np.sin(np.radians(45))  # a range of 0: nothing is normalised


# ---- polygons -------------------------------------------------------------------------------------------------------------
def device_mask(polygons, size, holes=None):
    from glimpse_amd import helpers

    got = helpers.polygons_to_mask(polygons, size, holes)
    want = tr.polygons_to_mask(polygons, size, holes)
    assert got.dtype == np.bool_ and got.shape == want.shape == (size[1], size[0])
    assert helpers.polygons_to_mask(polygons, size, holes).tobytes() == got.tobytes()  # two calls, the same bytes
    return got, want


def test_polygon_examples_of_the_reference():
    from glimpse_amd import Raster

    e = tr.DOCTEST_HELPER
    got, want = device_mask(e["polygons"], e["size"], e["holes"])
    assert np.array_equal(got, want) and np.array_equal(got, e["want"])
    raster = Raster([[0, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert np.array_equal(raster.rasterize_polygons(tr.DOCTEST_RASTER["polygons"]), tr.DOCTEST_RASTER["want"])


@pytest.mark.parametrize("name", sorted(tr.BOUNDARY))
def test_polygon_boundary_rule(name):
    polygons, size, want = tr.BOUNDARY[name]
    got, restated = device_mask(polygons, size)
    assert np.array_equal(got, want) and np.array_equal(restated, want)


@pytest.mark.parametrize("seed,size,n", [(3341, (13, 9), 3), (3342, (40, 37), 8), (3343, (130, 70), 25), (3344, (33, 65), 12)])
def test_polygon_stars_with_holes(seed, size, n):
    polygons, holes = tr.star_scene(seed, size, n)
    got, want = device_mask(polygons, size, holes)
    print(f"polygons seed {seed}: {int(want.sum())} cells inside, {int((got != want).sum())} differ from the restatement")
    assert np.array_equal(got, want)


def test_polygon_extremes():
    size = (70, 37)  # (nx, ny): three toggle words per row, the last one partly used
    nx, ny = size
    one_cell = [(20.3, 11.2), (20.9, 11.3), (20.8, 11.9), (20.2, 11.8)]  # its bounding box is cell (11, 20)
    got, want = device_mask([one_cell], size)
    assert np.array_equal(got, want) and got.sum() == 1 and got[11, 20]
    for outside in ([(-9.0, 3.0), (-2.0, 3.0), (-4.0, 30.0)], [(75.0, 3.0), (90.0, 3.0), (80.0, 30.0)],
                    [(5.0, -20.0), (60.0, -20.0), (30.0, -0.6)], [(5.0, 37.6), (60.0, 40.0), (30.0, 90.0)]):
        got, want = device_mask([outside], size)
        assert not got.any() and not want.any()
    everything = [(-5.0, -5.0), (nx + 5.0, -5.0), (nx + 5.0, ny + 5.0), (-5.0, ny + 5.0)]
    got, want = device_mask([everything], size)
    assert got.all() and want.all()
    got, want = device_mask([everything], size, holes=[everything])
    assert not got.any() and not want.any()
    # partly outside on every side, with a hole that is partly outside too
    got, want = device_mask([[(-10.0, 18.0), (35.0, -12.0), (85.0, 18.0), (35.0, 50.0)]], size,
                            holes=[[(50.0, 10.0), (90.0, 10.0), (90.0, 30.0), (50.0, 30.0)]])
    assert np.array_equal(got, want) and 0 < got.sum() < got.size


def test_polygon_crossings_at_the_word_boundary():
    """Crossings whose first toggled column is 31, 32 and 33 -- either side of the first 32-bit word of toggle bits -- as
    the left edge and as the right edge, and a row of 2100 cells (more than the 64 words a wave takes at a time)."""
    for nx in (70, 2100):
        size = (nx, 5)
        for first in (31, 32, 33):
            left = [(first - 0.3, 0.2), (first + 9.6, 0.2), (first + 9.6, 3.8), (first - 0.3, 3.8)]  # columns first .. first + 9
            right = [(2.2, 0.2), (first - 0.3, 0.2), (first - 0.3, 3.8), (2.2, 3.8)]  # columns 2 .. first - 1
            for ring in (left, right):
                got, want = device_mask([ring], size)
                assert np.array_equal(got, want)
            assert device_mask([left], size)[0][1, first - 1:first + 11].tolist() == [False] + [True] * 10 + [False]
            assert device_mask([right], size)[0][1, 1:first + 1].tolist() == [False] + [True] * (first - 2) + [False]
        wide = [(1.7, 0.1), (nx - 1.6, 0.4), (nx - 3.2, 4.9), (0.2, 4.2)]
        got, want = device_mask([wide], size, holes=[[(40.2, 1.2), (nx - 5.5, 1.4), (nx - 7.5, 3.7)]])
        assert np.array_equal(got, want) and got.sum() > nx


def test_three_hundred_rings():
    size = (130, 70)
    polygons, holes = tr.star_scene(3345, size, 220)
    assert len(polygons) + len(holes) >= 300 and len(holes) > 50
    got, want = device_mask(polygons, size, holes)
    print(f"{len(polygons)} polygons and {len(holes)} holes on 70 x 130: {int(want.sum())} cells inside, "
          f"{int((got != want).sum())} differ from the restatement")
    assert np.array_equal(got, want) and 0 < got.sum() < got.size


def test_rasterize_polygons_in_world_coordinates():
    dem, _ = raster_of(tr.case_name("x_desc", tr.TILED))
    ny, nx = dem.array.shape
    outline = np.array([[600.0, -150.0], [1500.0, -190.0], [1700.0, 60.0], [900.0, 120.0]])
    hole = np.array([[1000.0, -100.0], [1200.0, -100.0], [1100.0, 0.0]])
    got = dem.rasterize_polygons([outline], holes=[hole])
    corner = np.array((dem.xlim[0], dem.ylim[0]))
    want = tr.polygons_to_mask([((outline - corner) / dem.d - 0.5) + 0.5], (nx, ny), [((hole - corner) / dem.d - 0.5) + 0.5])
    assert got.shape == (ny, nx) and np.array_equal(got, want) and 0 < got.sum() < got.size
    # the centre of an inside cell lies inside the outline
    r, c = np.argwhere(got)[len(np.argwhere(got)) // 2]
    from matplotlib.path import Path

    assert Path(outline).contains_point((dem.x[c], dem.y[r])) and not Path(hole).contains_point((dem.x[c], dem.y[r]))


# ---- the chains ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32", "int64"])
def test_rasterize_equals_the_reference(golden, dtype):
    from glimpse_amd import Raster

    array, xlim, ylim, xy, values = tr.rasterize_case(dtype)
    dem = Raster(array.copy(), x=xlim, y=ylim)
    got = dem.rasterize(xy, values)
    same_bytes(got, golden(G33)[f"rasterize_{dtype}"], f"rasterize {dtype}, device against the reference")
    assert np.array_equal(dem.array, array) and dem.rasterize(xy, values).tobytes() == got.tobytes()


def test_project_dem_drapes_the_hillshade(golden):
    """Camera.project_dem(dem, values=dem.hillshade()): the synthetic image for calibration, equal to the one made from the
    restated hillshade."""
    from glimpse_amd import Raster
    from tests.test_gpu_project_dem import camera_of

    c = pr.g29_case(golden("g29_project_dem.npz"), "tiles32")
    dem = Raster(c["z"], x=c["xlim"], y=c["ylim"])
    shade = dem.hillshade()
    want_shade = tr.hillshade(dem.array, dem.d)
    same_bytes(shade, want_shade, "hillshade of the g29 DEM")
    args = dict(tile_size=c["tile_size"], tile_overlap=c["tile_overlap"])
    image = camera_of(c["cam"]).project_dem(dem, values=shade, **args)
    want = camera_of(c["cam"]).project_dem(dem, values=want_shade, **args)
    seen = ~np.isnan(image)
    print(f"project_dem of a hillshade: {int(seen.sum())} of {image.size} pixels see the DEM, values "
          f"{np.nanmin(image):.3f} .. {np.nanmax(image):.3f}")
    assert image.tobytes() == want.tobytes() and seen.sum() > 100 and np.nanmax(image) - np.nanmin(image) > 0.1
