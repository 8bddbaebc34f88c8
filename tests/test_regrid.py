"""Raster.sample(grid=True) / resample / resize / crop and RasterInterpolant without a GPU.

Three things are checked here.  (1) tests/regrid_restatement.py, which restates what the kernels of glh_regrid.hip do
operation by operation, against the reference's own answers (tests/golden/g32_regrid.npz), within the tolerances the
issue derived from two correct float64 implementations of the same collocation system (FITPACK against a dense solve):
1e-14, 2e-14, 6e-14, 3e-13, 3e-13 of max |reference result| for orders 1 .. 5.  (2) The host logic of glimpse_amd.raster --
bounds, flips, output direction, fill, crop_extent, nearest, the interpolant's flow -- against the golden file, exactly
where it is integer or a copy; for that the three library calls are replaced by the restatement (`restated`), so no
device is touched.  (3) The library's per-axis host arithmetic (glh_regrid_host.h, compiled for the CPU) against the
restatement, bit for bit.  tests/test_gpu_regrid.py then holds the kernels to the restatement bit for bit.

NaN masks: the reference turns every sample below the raster's minimum into NaN.  A sample that lies within the case's
tolerance of that minimum (the minimum cell's own centre, for one) is blanked or not by its last bit, in the reference as
here; such samples (`ties`) are left out of the mask comparison, every other sample's mask must be equal.

Measured here against the reference (max difference / max |result|): order 1 6.3e-16, order 2 1.5e-15, order 3 2.5e-15,
order 4 1.7e-14, order 5 6.7e-14; zoom 4.6e-13 at |z| = 1100 (bound 2.0e-12); the printed lines give them case by case.
"""
import ctypes as C
import datetime
import os
import subprocess

import numpy as np
import pytest

from tests import regrid_restatement as rr
from tests import viewshed_terrain as vt

G32 = "g32_regrid.npz"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- helpers shared with tests/test_gpu_regrid.py -----------------------------------------------------------------------
def regrid_from_source(source, xo, yo):
    """What glh_stage_raster_regrid returns for a _lib.regrid_src pair, by the restatement."""
    st, (z, gx, gy, mask) = source
    return rr.regrid(z, gx, gy, (st.xmin, st.xmax, st.ymin, st.ymax), st.kx, st.ky, np.asarray(xo, dtype=float),
                     np.asarray(yo, dtype=float), nan_mask=mask, zmin=st.zmin if st.use_zmin else None,
                     flip_x=bool(st.flip_x), flip_y=bool(st.flip_y))


def restated_interpolate(m0, m1, scale, scale2, ratio, s0=None, s1=None, xo=None, yo=None):
    if isinstance(m1, tuple):
        m1 = regrid_from_source(m1, xo, yo)
    if isinstance(s1, tuple):
        s1 = regrid_from_source(s1, xo, yo)
    m0, m1 = np.asarray(m0, dtype=np.float64), np.asarray(m1, dtype=np.float64)
    if s0 is None:
        return rr.blend(m0, m1, scale)
    return rr.blend(m0, m1, scale, np.asarray(s0, dtype=np.float64), np.asarray(s1, dtype=np.float64), scale2, ratio)


@pytest.fixture
def restated(monkeypatch):
    """glimpse_amd with its three regridding library calls answered by the restatement: the host logic runs, no device."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "stage_raster_regrid", regrid_from_source)
    monkeypatch.setattr(_lib, "stage_zoom_linear", lambda a, shape: rr.zoom_linear(a, shape))
    monkeypatch.setattr(_lib, "stage_raster_interpolate", restated_interpolate)


@pytest.fixture
def no_device(monkeypatch):
    """Any call into the library fails the test: what is refused is refused before device work."""
    from glimpse_amd import _lib

    def called(*args, **kwargs):
        raise AssertionError("the library was called")

    for name in ("stage_raster_regrid", "stage_zoom_linear", "stage_raster_interpolate", "load"):
        monkeypatch.setattr(_lib, name, called)


def sample_case(name, g):
    """The inputs of a sample case, checked against the golden file's SHA-256."""
    z, xlim, ylim, xy, kwargs = rr.build(name)
    assert vt.sha256(z).tobytes() == g[f"{name}__sha256"].tobytes(), f"{name}: the input is not the one the golden was made from"
    return z, xlim, ylim, xy, kwargs


def compare_with_reference(name, got, want, raw, zmin, order, what):
    """Asserts `got` against the reference's `want`: values relative to max |want| within the order's tolerance, NaN masks
    equal except at ties (`raw`: the samples before the reference's `< minimum` blanking).  Prints the measured figure."""
    assert got.shape == want.shape and got.dtype == np.float64, (name, got.shape, want.shape)
    tol = rr.TOLERANCE[order]
    scale = np.nanmax(np.abs(want))
    with np.errstate(invalid="ignore"):
        ties = np.abs(raw - zmin) <= tol * scale
    mask_differs = (np.isnan(got) != np.isnan(want)) & ~ties
    both = ~np.isnan(got) & ~np.isnan(want)
    diff = float(np.max(np.abs(got[both] - want[both])) / scale) if both.any() else 0.0
    print(f"regrid {what} {name}: max difference / max|result| = {diff:.2e} (tolerance {tol:.0e}), NaN {int(np.isnan(want).sum())} "
          f"of {want.size}, masks differ at {int(mask_differs.sum())}, ties left out {int(ties.sum())}")
    assert both.any() and diff <= tol, (name, diff, tol)
    assert not mask_differs.any(), (name, np.argwhere(mask_differs)[:5])


def raw_samples(z, xlim, ylim, xy, kwargs):
    zmin = float(np.nanmin(np.asarray(z, dtype=np.float64)))
    return rr.sample_grid(z, xlim, ylim, xy, blank_below_min=False, **kwargs), zmin


def as_rasters(items):
    from glimpse_amd import Raster

    if items is None:
        return None
    return [v if np.isscalar(v) else Raster(v[0].copy(), x=v[1], y=v[2]) for v in items]


def interpolant_case(name, g):
    from glimpse_amd import RasterInterpolant

    means, sigmas, x, call = rr.interpolant_inputs(name)
    parts = [m[0].ravel() for m in means]
    if isinstance(sigmas, list) and not np.isscalar(sigmas[0]):
        parts += [s[0].ravel() for s in sigmas]
    assert vt.sha256(np.concatenate(parts)).tobytes() == g[f"{name}__sha256"].tobytes()
    return RasterInterpolant(as_rasters(means), as_rasters(sigmas), x=x), call


def check_interpolant(name, g, exact):
    """Runs the case through glimpse_amd.RasterInterpolant and compares with the reference: shapes, limits and `nearest`
    exactly; the arrays bit for bit when `exact`, else within the order-1 tolerance of max |result| (means and sigmas:
    the square root passes a relative bound on)."""
    interpolant, call = interpolant_case(name, g)
    assert interpolant.nearest(call["xi"], extrapolate=call.get("extrapolate", False)) == tuple(g[f"{name}__ij"])
    result = interpolant(**call)
    mean, sigma = result if isinstance(result, tuple) else (result, None)
    assert np.array_equal(np.concatenate((mean.xlim, mean.ylim)), g[f"{name}__limits"])
    assert (sigma is not None) == (f"{name}__sigma" in g)
    assert mean.datetime == (call["xi"] if isinstance(call["xi"], datetime.datetime) else None)
    for what, got, want in (("z", mean, g[f"{name}__z"]), ("sigma", sigma, g.get(f"{name}__sigma"))):
        if got is None:
            continue
        got = got.array
        assert got.shape == want.shape and got.dtype == np.float64, (name, what, got.shape, want.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, what)
        ok = ~np.isnan(want)
        diff = float(np.max(np.abs(got[ok] - want[ok])) / np.max(np.abs(want[ok])))
        print(f"interpolant {name} {what}: max difference / max|result| = {diff:.2e}", "(bit for bit)" if exact else
              f"(tolerance {rr.TOLERANCE[1]:.0e})")
        if exact:
            assert got[ok].tobytes() == want[ok].tobytes(), (name, what, diff)
        else:
            assert diff <= rr.TOLERANCE[1], (name, what, diff)
    return mean, sigma


EQUAL_GRID_CASES = ("equal_grids", "equal_grids_sigma", "number_sigmas", "no_sigmas", "extrapolate")


def small_raster(shape=(6, 7), seed=3290, **kwargs):
    from glimpse_amd import Raster

    xlim, ylim = rr.limits(shape, **kwargs)
    return Raster(rr.dem(shape, seed), x=xlim, y=ylim)


def check_refusals():
    """Everything the issue lists as refused raises what it says.  Shared by the CPU test (where any library call fails
    the test) and the GPU test."""
    from glimpse_amd import Raster, RasterInterpolant
    from glimpse_amd.raster import SplineOrderError

    dem = small_raster()
    x, y = dem.x, dem.y
    with pytest.raises(ValueError, match="Some of the sampling coordinates are out of bounds"):
        dem.sample((x + 1000.0, y), grid=True)
    with pytest.raises(ValueError, match="out of bounds"):  # (the bounds test comes before anything else)
        dem.sample((x + 1000.0, y), grid=True, order=0)
    with pytest.raises(SplineOrderError):
        dem.sample((x, y), grid=True, order=0)
    with pytest.raises(SplineOrderError):
        dem.sample((x, y), grid=True, order=6)
    assert SplineOrderError.__bases__ == (Exception,)
    with pytest.raises(NotImplementedError, match="1-D"):
        Raster(np.arange(5.0)[None, :], x=(0, 50), y=(0, 10)).sample((np.array([5.0, 15.0]), np.array([5.0])), grid=True)
    with pytest.raises(ValueError, match="needs more than 3 cells"):
        thin = small_raster((3, 7))
        thin.sample((thin.x, thin.y), grid=True, order=3)
    with pytest.raises(ValueError, match="strictly"):
        dem.sample((x[[0, 2, 1]], y), grid=True)
    holes = small_raster()
    holes.array[2, 3] = np.nan
    for order in (2, 3, 4, 5):
        with pytest.raises(ValueError, match="NaN cells: they are served at order 1 only"):
            holes.sample((x, y), grid=True, order=order)
    with pytest.raises(NotImplementedError, match="order 3"):
        dem.resize(0.5, order=3)
    with pytest.raises(NotImplementedError, match="int64"):
        Raster(np.arange(12).reshape(3, 4)).resize(2.0)
    with pytest.raises(NotImplementedError, match="file I/O"):
        RasterInterpolant(["a.tif", "b.tif"], x=[0.0, 1.0])(0.5)
    with pytest.raises(NotImplementedError, match="file I/O"):
        RasterInterpolant([dem, dem], sigmas=["a.tif", "b.tif"], x=[0.0, 1.0])(0.5, return_sigma=True)
    with pytest.raises(ValueError, match="Not bounded on both sides by a Raster"):
        RasterInterpolant([dem, dem], x=[0.0, 1.0]).nearest(2.0)
    with pytest.raises(ValueError, match="Not bounded on both sides by a Raster"):
        RasterInterpolant([dem, dem], x=[0.0, 1.0])(-0.5)
    # grid=False stays as it was
    with pytest.raises(NotImplementedError, match="only point sampling with order 0 or 1 is built"):
        dem.sample(np.array([[x[1], y[1]]]), order=3)


# ---- (3) the library's host arithmetic ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostlib():
    src = os.path.join(ROOT, "tests", "hostcheck", "regrid_hostcheck.cpp")
    out = os.path.join(ROOT, "tests", "hostcheck", "_build", "libregrid_hostcheck.so")
    deps = [src] + [os.path.join(ROOT, "glimpse_amd", "csrc", f) for f in ("glh_regrid_host.h", "glh_regrid.h")]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", out, src], check=True)
    lib = C.CDLL(out)
    lib.rg_basis.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p]
    lib.rg_knots.argtypes = [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_int, C.c_void_p]
    lib.rg_factor.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return lib


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_library_host_arithmetic_equals_the_restatement(hostlib, k):
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for n in (k + 1, k + 2, 13, 130):
        lim = (rr.X0, rr.X0 + n * rr.CELL)
        x = np.ascontiguousarray(rr.centres(lim, n))
        t = np.empty(n + k + 1)
        hostlib.rg_knots(ptr(x), n, lim[0], lim[1], k, ptr(t))
        want = rr.knots(x, lim[0], lim[1], k)
        assert t.tobytes() == want.tobytes(), (k, n)
        assert (np.diff(t) >= 0).all() and len(np.unique(t)) == n - k + 1
        lu = np.empty((n, 2 * k + 1))
        assert hostlib.rg_factor(ptr(x), n, ptr(t), k, ptr(lu)) == 1
        assert lu.tobytes() == rr.factor(x, want, k).tobytes(), (k, n)
        h = np.zeros(6)
        for v in np.concatenate(([lim[0] - 3.0, lim[0], lim[1], lim[1] + 3.0], x[:3], t[k:k + 3], rr.spread(lim, 7.3, 0.4))):
            l = hostlib.rg_basis(ptr(t), n, k, float(v), ptr(h))
            wl, wh = rr.basis(want, n, k, v)
            assert l == wl and h[:k + 1].tobytes() == wh.tobytes(), (k, n, v)
            assert k <= l <= n - 1 and abs(h[:k + 1].sum() - 1.0) < 1e-14  # (a partition of unity on the clamped argument)


def test_knots_are_fitpacks(golden):
    """The knots the issue states, against scipy's own where scipy is installed (it is not a dependency)."""
    interpolate = pytest.importorskip("scipy.interpolate")
    for k in range(1, 6):
        for n in (k + 1, 9, 12):
            lim = (rr.X0, rr.X0 + n * rr.CELL)
            x = rr.centres(lim, n)
            y = rr.centres((0.0, 80.0), 8)
            spline = interpolate.RectBivariateSpline(x, y, np.add.outer(x, y), bbox=(lim[0], lim[1], 0.0, 80.0), kx=k, ky=1, s=0)
            assert np.array_equal(spline.get_knots()[0], rr.knots(x, lim[0], lim[1], k)), (k, n)


# ---- (1), (2): the sample cases -----------------------------------------------------------------------------------------
def test_golden_is_small_and_lists_the_cases(golden):
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G32)) < 400_000
    g = golden(G32)
    assert sorted(g["sample_cases"]) == sorted(rr.SAMPLE_CASES) and sorted(g["interpolant_cases"]) == sorted(rr.INTERPOLANT_CASES)
    orders = {(c["shape"], c["order"]) for c in rr.SAMPLE_CASES.values()}
    assert all(((13, 17), k) in orders and ((70, 130), k) in orders for k in range(1, 6))


@pytest.mark.parametrize("name", sorted(n for n in rr.SAMPLE_CASES if n != "constant_1x1"))
def test_sample_grid_against_the_reference(golden, restated, name):
    from glimpse_amd import Raster

    g = golden(G32)
    z, xlim, ylim, xy, kwargs = sample_case(name, g)
    before = z.copy()
    got = Raster(z, x=xlim, y=ylim).sample(xy, grid=True, **kwargs)
    assert vt.sha256(z).tobytes() == vt.sha256(before).tobytes()  # (the raster is left as it was, NaN cells included)
    # the package's host logic and the restatement's agree in every bit, NaN for NaN
    again = rr.sample_grid(z, xlim, ylim, xy, **kwargs)
    assert got.tobytes() == again.tobytes()
    raw, zmin = raw_samples(z, xlim, ylim, xy, kwargs)
    compare_with_reference(name, got, g[f"{name}__out"], raw, zmin, kwargs["order"], "restatement against the reference")
    if kwargs["fill_value"] is not None and not kwargs["bounds_error"]:
        x, y = xy
        outside = np.add.outer((y < min(ylim)) | (y > max(ylim)), (x < min(xlim)) | (x > max(xlim)))
        assert outside.any() and (got[outside] == kwargs["fill_value"]).all() and (got[~outside] != kwargs["fill_value"]).all()


def test_a_1x1_raster_returns_its_constant(golden, no_device):
    from glimpse_amd import Raster

    g = golden(G32)
    z, xlim, ylim, xy, kwargs = sample_case("constant_1x1", g)
    got = Raster(z, x=xlim, y=ylim).sample(xy, grid=True, **kwargs)
    assert got.dtype == np.float64 and got.shape == (3, 3) and np.array_equal(got, g["constant_1x1__out"])
    got = Raster(z, x=xlim, y=ylim).sample((xy[0], xy[1][:2]), grid=True, **kwargs)
    assert got.shape == (2, 3)  # (len(y), len(x))


def test_the_nan_rule_of_order_1():
    """A NaN at an interior cell centre c blanks the open interval (c - d, c + d); a NaN in cell 0 blanks [limit, centre of
    cell 1); the second cell also takes the first coefficient with it."""
    shape, d = (9, 12), rr.CELL
    xlim, ylim = rr.limits(shape, ydesc=False)
    x = np.unique(np.concatenate((rr.on_grid_lines(xlim, 12), rr.spread(xlim, 1.3, 0.1))))
    y = rr.centres(ylim, 9)[[4]] + 2.0
    cx = rr.centres(xlim, 12)

    def blanked(col):
        z = rr.dem(shape, 3295)
        z[4, col] = np.nan
        return np.isnan(rr.sample_grid(z, xlim, ylim, (x, y))[0])

    assert np.array_equal(blanked(5), (x > cx[5] - d) & (x < cx[5] + d))
    assert np.array_equal(blanked(0), x < cx[1])
    assert np.array_equal(blanked(11), x > cx[10])
    assert np.array_equal(blanked(1), x < cx[2])


def test_resample_in_place(golden, restated):
    from glimpse_amd import Raster

    g = golden(G32)
    z, xlim, ylim, _, _ = sample_case("small_k3", g)
    for order in (1, 3):
        raster = Raster(z.copy(), x=xlim, y=ylim)
        target = Raster(np.zeros((9, 14)), x=(rr.X0 + 12.0, rr.X0 + 152.0), y=(rr.Y0 + 121.0, rr.Y0 + 13.0))
        raster.resample(target, order=order)
        want = g[f"resample_k{order}__out"]
        assert raster.array.shape == (9, 14) and tuple(raster.size) == (14, 9)
        assert np.array_equal(np.concatenate((raster.xlim, raster.ylim)), g[f"resample_k{order}__limits"])
        assert raster.grid == target.grid and np.array_equal(raster.x, target.x)
        raw = rr.sample_grid(z, xlim, ylim, (target.x, target.y), order=order, blank_below_min=False)
        compare_with_reference(f"resample order {order}", raster.array, want, raw, float(z.min()), order, "restatement")


@pytest.mark.parametrize("zoom", rr.ZOOMS)
def test_resize_against_the_reference(golden, restated, zoom):
    from glimpse_amd import Raster

    g = golden(G32)
    a = rr.zoom_input()
    assert vt.sha256(a).tobytes() == g["zoom__sha256"].tobytes()
    raster = Raster(a.copy(), x=(rr.X0, rr.X0 + 310.0), y=(rr.Y0 + 230.0, rr.Y0))
    raster.resize(zoom)
    want = g[f"zoom_{zoom}__out"]
    assert raster.array.shape == want.shape and tuple(raster.size) == want.shape[::-1] and raster.array.dtype == np.float64
    assert np.array_equal(raster.xlim, (rr.X0, rr.X0 + 310.0))  # (`array` only: the limits stay)
    diff, bound = float(np.max(np.abs(raster.array - want))), 8 * EPS * float(np.max(np.abs(a)))
    print(f"zoom {zoom}: {a.shape} -> {want.shape}, max difference {diff:.2e} (bound 8 eps max|z| = {bound:.2e})")
    assert diff <= bound
    single = Raster(a.astype(np.float32))
    single.resize(zoom)
    assert single.array.dtype == np.float32 and single.array.shape == want.shape


def test_crop_extent_and_crop(golden):
    from glimpse_amd import Raster

    g = golden(G32)
    xlim, ylim = rr.limits(rr.CROP_SHAPE)
    z = rr.dem(rr.CROP_SHAPE, 3296)
    for k, (bx, by) in enumerate(rr.CROP_BOXES):
        raster = Raster(z.copy(), x=xlim, y=ylim)
        cx, cy, rows, cols = raster.crop_extent(xlim=bx, ylim=by)
        assert np.array_equal(np.concatenate((cx, cy)), g[f"crop{k}__limits"]), k
        assert np.array_equal(np.concatenate((rows, cols)), g[f"crop{k}__rowcol"]), k
        raster.crop(xlim=bx, ylim=by)
        assert np.array_equal(raster.array, z[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1])
        assert tuple(raster.size) == raster.array.shape[::-1] and np.array_equal(raster.xlim, cx) and np.array_equal(raster.ylim, cy)
        assert np.allclose(np.abs(raster.d), rr.CELL)
    # the snap-down of inner edges: a box on cell edges keeps the cells inside it and no more
    assert tuple(g["crop1__rowcol"]) == (5, 10, 3, 8)
    raster = Raster(z.copy(), x=xlim, y=ylim)
    low, high = np.percentile(z, [20, 80])
    raster.crop(zlim=(high, low))
    assert np.array_equal(np.isnan(raster.array), (z < low) | (z > high)) and 50 < np.isnan(raster.array).sum() < 150
    with pytest.warns(UserWarning, match="cast to float"):
        ints = Raster(np.arange(12).reshape(3, 4))
        ints.crop(zlim=(2, 9))
    assert ints.array.dtype == np.float64 and np.isnan(ints.array[0, 0])
    with pytest.raises(ValueError, match="Boxes do not intersect"):
        raster.crop_extent(xlim=(0.0, 10.0))


def test_copy_grid_and_boxes():
    from glimpse_amd import Raster, helpers
    from glimpse_amd.raster import Grid

    when = datetime.datetime(2014, 7, 1)
    a = Raster(rr.dem((5, 6), 1), x=(10.0, 70.0), y=(50.0, 0.0), datetime=when)
    b = a.copy()
    assert b is not a and b.array is not a.array and np.array_equal(a.array, b.array) and b.datetime == when
    b.array[0, 0] = -1.0
    b.xlim[0] = 0.0
    assert a.array[0, 0] != -1.0 and a.xlim[0] == 10.0
    assert a.grid == a.copy().grid and not (a.grid != a.copy().grid) and a.grid != b.grid
    assert a.grid != Raster(np.zeros((5, 7)), x=(10.0, 70.0), y=(50.0, 0.0)).grid
    assert isinstance(a.grid, Grid) and a.grid.shape == (5, 6) and np.array_equal(a.grid.x, a.x)
    assert np.array_equal(a.box2d, (10.0, 0.0, 70.0, 50.0)) and np.array_equal(a.grid.box2d, a.box2d)
    assert np.array_equal(helpers.intersect_boxes([(0, 0, 10, 10), (5, 5, 15, 15)]), (5, 5, 10, 10))
    assert np.array_equal(helpers.intersect_boxes([a.box2d, (-np.inf, -np.inf, np.inf, 20.0)]), (10.0, 0.0, 70.0, 20.0))
    with pytest.raises(ValueError, match="not divisible"):
        helpers.intersect_boxes([(0, 0, 1)])


def test_nearest(golden, no_device):
    from glimpse_amd import RasterInterpolant

    rows = golden(G32)["nearest"]
    assert len(rows) == 32
    for n, xi, extrapolate, i, j in rows:
        numeric = int(n) == 4
        series = [0.0, 10.0, 30.0, 31.0] if numeric else rr.DATETIMES
        xi = float(xi) if numeric else rr.T0 + datetime.timedelta(days=float(xi))
        interpolant = RasterInterpolant([0] * len(series), x=series)
        if i < 0:
            with pytest.raises(ValueError, match="Not bounded on both sides by a Raster"):
                interpolant.nearest(xi, extrapolate=bool(extrapolate))
        else:
            assert interpolant.nearest(xi, extrapolate=bool(extrapolate)) == (int(i), int(j)), (series, xi, extrapolate)
    dated = [small_raster() for _ in range(2)]
    dated[0].datetime, dated[1].datetime = rr.DATETIMES[:2]
    assert list(RasterInterpolant(dated).x) == rr.DATETIMES[:2]  # (x defaults to the means' datetimes)


@pytest.mark.parametrize("name", sorted(rr.INTERPOLANT_CASES))
def test_interpolant_against_the_reference(golden, restated, name):
    g = golden(G32)
    exact = name in EQUAL_GRID_CASES
    mean, sigma = check_interpolant(name, g, exact)
    if name == "d_given":  # the quirk: 10 m rasters asked for d = 20 come back at 5 m
        assert mean.array.shape == (24, 32) and np.allclose(np.abs(mean.d), 5.0)
        mean, _ = check_interpolant_d_equal()
        assert mean.array.shape == (12, 16)
    if name == "limits_given":
        # zlim blanks cells of the means; the sigma takes the means' difference in and is NaN there too
        assert np.isnan(mean.array).any() and np.array_equal(np.isnan(mean.array), np.isnan(sigma.array))


def check_interpolant_d_equal():
    """d compared by exact float equality: the rasters' own cell size changes nothing."""
    from glimpse_amd import RasterInterpolant

    means, sigmas, x, call = rr.interpolant_inputs("d_given")
    call["d"] = 10.0
    return RasterInterpolant(as_rasters(means), as_rasters(sigmas), x=x)(**call)


def test_interpolant_fun_runs_on_copies(restated):
    from glimpse_amd import RasterInterpolant

    means, _, x, _ = rr.interpolant_inputs("equal_grids")
    rasters = as_rasters(means)
    kept = [r.array.copy() for r in rasters]

    def lift(raster, by):
        raster.array += by

    plain = RasterInterpolant(rasters, x=x)(4.0)
    lifted = RasterInterpolant(rasters, x=x)(4.0, fun=lift, by=100.0)
    assert all(np.array_equal(r.array, k) for r, k in zip(rasters, kept))
    assert np.allclose(lifted.array, plain.array + 100.0, rtol=0, atol=1e-9) and not np.array_equal(lifted.array, plain.array)


def test_refusals_come_before_any_device_work(no_device):
    check_refusals()
