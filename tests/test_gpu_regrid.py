"""`Raster.sample(grid=True)`, `resample`, `resize` and `RasterInterpolant` on the device, through the Python API and so
through the C ABI (`glh_stage_raster_regrid`, `glh_stage_zoom_linear`, `glh_stage_raster_interpolate`; the kernels of
glh_regrid.hip).

Expected: the NumPy restatement (tests/regrid_restatement.py) bit for bit, NaN for NaN -- the kernels do the same float64
operations in the same order with no contraction, so no tolerance is taken -- and the reference's own answers
(tests/golden/g32_regrid.npz) within the tolerances of tests/test_regrid.py, with equal NaN masks.  Every test prints what
it measured.
"""
import numpy as np
import pytest

from tests import regrid_restatement as rr
from tests.test_regrid import (EPS, EQUAL_GRID_CASES, G32, as_rasters, check_interpolant, check_refusals,
                               compare_with_reference, raw_samples, regrid_from_source, restated_interpolate, sample_case,
                               small_raster)

pytestmark = pytest.mark.gpu


def same_bytes(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    differing = int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
    print(f"regrid {what}: {differing} of {want.size} samples differ from the restatement")
    assert differing == 0 and got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("name", sorted(n for n in rr.SAMPLE_CASES if n != "constant_1x1"))
def test_every_g32_sample_case(golden, name):
    from glimpse_amd import Raster

    g = golden(G32)
    z, xlim, ylim, xy, kwargs = sample_case(name, g)
    dem = Raster(z, x=xlim, y=ylim)
    got = dem.sample(xy, grid=True, **kwargs)
    same_bytes(got, rr.sample_grid(z, xlim, ylim, xy, **kwargs), name)
    raw, zmin = raw_samples(z, xlim, ylim, xy, kwargs)
    compare_with_reference(name, got, g[f"{name}__out"], raw, zmin, kwargs["order"], "device against the reference")
    assert dem.sample(xy, grid=True, **kwargs).tobytes() == got.tobytes()  # two calls, the same bytes


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_resample_onto_the_own_grid_returns_the_raster(order):
    dem = small_raster((70, 130), seed=3297)
    before = dem.array.copy()
    dem.resample(dem.grid, order=order)
    diff = float(np.nanmax(np.abs(dem.array - before)) / np.max(np.abs(before)))
    print(f"resample order {order} onto the own grid: max difference / max|z| = {diff:.2e} (tolerance {rr.TOLERANCE[order]:.0e})")
    # (the minimum cell may come back NaN: the reference blanks samples below the minimum, and a last bit decides there)
    assert np.isnan(dem.array).sum() <= 1 and diff <= rr.TOLERANCE[order]
    assert dem.array.shape == before.shape and dem.grid == small_raster((70, 130)).grid


def test_resample_against_the_reference(golden):
    from glimpse_amd import Raster

    g = golden(G32)
    z, xlim, ylim, _, _ = sample_case("small_k3", g)
    for order in (1, 3):
        raster = Raster(z.copy(), x=xlim, y=ylim)
        target = Raster(np.zeros((9, 14)), x=(rr.X0 + 12.0, rr.X0 + 152.0), y=(rr.Y0 + 121.0, rr.Y0 + 13.0))
        raster.resample(target, order=order)
        same_bytes(raster.array, rr.sample_grid(z, xlim, ylim, (target.x, target.y), order=order), f"resample order {order}")
        raw = rr.sample_grid(z, xlim, ylim, (target.x, target.y), order=order, blank_below_min=False)
        compare_with_reference(f"resample order {order}", raster.array, g[f"resample_k{order}__out"], raw, float(z.min()), order,
                               "device")
        assert np.array_equal(np.concatenate((raster.xlim, raster.ylim)), g[f"resample_k{order}__limits"])


@pytest.mark.parametrize("zoom", rr.ZOOMS)
def test_resize(golden, zoom):
    from glimpse_amd import Raster

    g = golden(G32)
    a = rr.zoom_input()
    raster = Raster(a.copy(), x=(rr.X0, rr.X0 + 310.0), y=(rr.Y0 + 230.0, rr.Y0))
    raster.resize(zoom)
    want = g[f"zoom_{zoom}__out"]
    same_bytes(raster.array, rr.zoom_linear(a, want.shape), f"zoom {zoom}")
    diff, bound = float(np.max(np.abs(raster.array - want))), 8 * EPS * float(np.max(np.abs(a)))
    print(f"zoom {zoom}: max difference from the reference {diff:.2e} (bound {bound:.2e})")
    assert diff <= bound
    again = Raster(a.copy())
    again.resize(zoom)
    assert again.array.tobytes() == raster.array.tobytes()


@pytest.mark.parametrize("name", sorted(rr.INTERPOLANT_CASES))
def test_interpolant(golden, name, monkeypatch):
    from glimpse_amd import RasterInterpolant, _lib

    g = golden(G32)
    mean, sigma = check_interpolant(name, g, name in EQUAL_GRID_CASES)
    # the same call with the library answered by the restatement: the device's bytes
    means, sigmas, x, call = rr.interpolant_inputs(name)
    with monkeypatch.context() as m:
        m.setattr(_lib, "stage_raster_regrid", regrid_from_source)
        m.setattr(_lib, "stage_zoom_linear", lambda a, shape: rr.zoom_linear(a, shape))
        m.setattr(_lib, "stage_raster_interpolate", restated_interpolate)
        result = RasterInterpolant(as_rasters(means), as_rasters(sigmas), x=x)(**call)
    want_mean, want_sigma = result if isinstance(result, tuple) else (result, None)
    same_bytes(mean.array, want_mean.array, f"interpolant {name} z")
    if sigma is not None:
        same_bytes(sigma.array, want_sigma.array, f"interpolant {name} sigma")
    again = RasterInterpolant(as_rasters(means), as_rasters(sigmas), x=x)(**call)
    again = again if isinstance(again, tuple) else (again,)
    assert again[0].array.tobytes() == mean.array.tobytes() and (sigma is None or again[1].array.tobytes() == sigma.array.tobytes())


def test_times_and_both_solve_kernels_on_one_raster():
    """Orders that differ per axis go through the C ABI: the general solve on one axis, the closed form on the other."""
    from glimpse_amd import _lib

    dem = small_raster((70, 130), seed=3298, ydesc=False)
    x, y = rr.spread(dem.xlim, 9.7, 0.3), rr.spread(dem.ylim, 11.3, 0.9)
    box = (dem.min[0], dem.max[0], dem.min[1], dem.max[1])
    for kx, ky in ((1, 4), (5, 1), (2, 3)):
        source = _lib.regrid_src(dem.array, dem.x, dem.y, box, kx, ky)
        got, times = _lib.stage_raster_regrid(source, x, y, return_times=True)
        same_bytes(got, rr.regrid(dem.array, dem.x, dem.y, box, kx, ky, x, y), f"orders ({kx}, {ky})")
        assert set(times) == set(_lib.REGRID_TIMES) and all(v > 0.0 for v in times.values())


def test_refusals_and_argument_errors_need_no_kernel():
    from glimpse_amd import _lib

    check_refusals()
    lib = _lib.load()
    INVALID, UNSUPPORTED = -1, -5
    z = rr.dem((6, 7), 3299)
    gx, gy = 5.0 + 10.0 * np.arange(7), 5.0 + 10.0 * np.arange(6)
    box = (0.0, 70.0, 0.0, 60.0)
    xo, yo = np.array([1.0, 2.0, 69.0]), np.array([3.0, 30.0])
    out = np.zeros((2, 3))

    def call(z=z, gx=gx, gy=gy, box=box, kx=1, ky=1, xo=xo, yo=yo, out=out, mask=None):
        pair = _lib.regrid_src(z, gx, gy, box, kx, ky, nan_mask=mask) if z is not None else None  # (keeps its arrays alive)
        return lib.glh_stage_raster_regrid(0, None if pair is None else _lib.C.byref(pair[0]), _lib._ptr(xo), len(xo),
                                           _lib._ptr(yo), len(yo), _lib._ptr(out), None)

    def message():
        return lib.glh_last_error().decode()

    assert call(z=None) == INVALID and "null" in message()
    assert call(out=None) == INVALID and "null" in message()
    assert call(kx=0) == INVALID and "order 0" in message()
    assert call(ky=6) == INVALID and "order 6" in message()
    assert call(z=z[:, :4], gx=gx[:4], kx=4) == INVALID and "needs more than 4" in message()
    assert call(gx=gx[::-1].copy()) == INVALID and "ascending" in message()
    assert call(xo=xo[::-1].copy()) == INVALID and "decreases" in message()
    assert call(box=(10.0, 70.0, 0.0, 60.0)) == INVALID and "leave the box" in message()
    assert call(kx=3, ky=3, mask=np.zeros((6, 7), np.uint8)) == UNSUPPORTED and "order 1 only" in message()
    bad = z.copy()
    bad[2, 2] = np.nan
    assert call(z=bad) == INVALID and "not finite" in message()
    assert call() == 0 and np.isfinite(out).all()
    a = np.zeros((3, 4))
    assert lib.glh_stage_zoom_linear(0, None, 4, 3, 8, 6, _lib._ptr(np.zeros((6, 8))), None) == INVALID
    assert lib.glh_stage_zoom_linear(0, _lib._ptr(a), 4, 3, 0, 6, _lib._ptr(np.zeros((6, 8))), None) == INVALID
    zz = np.zeros((3, 4))
    assert lib.glh_stage_raster_interpolate(0, 4, 3, _lib._ptr(a), None, None, None, None, None, None, None, 0.5, 0.25, 1 / 3,
                                            0.5, _lib._ptr(zz), None, None) == INVALID and "null" in message()
    assert lib.glh_stage_raster_interpolate(0, 4, 3, _lib._ptr(a), _lib._ptr(a), None, None, None, None, None, None, 0.5, 0.25,
                                            1 / 3, 0.5, _lib._ptr(zz), _lib._ptr(zz), None) == INVALID and "sigma" in message()
