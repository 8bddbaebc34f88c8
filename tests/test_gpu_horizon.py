"""`Raster.horizon` on the device, through the Python API and so through the C ABI (`glh_stage_horizon`; kernel `k_horizon`,
one workgroup per heading's line).

Expected: on every heading the reference computed, the reference's own answer (tests/golden/g31_horizon.npz); on ALL
headings, the NumPy restatement (tests/horizon_restatement.py) -- both bit for bit: the kernel does the same float64
operations in the same order, so no tolerance is taken.  Each test prints its count of differing headings and asserts 0.
"""
import numpy as np
import pytest

from tests import horizon_restatement as hr
from tests.test_horizon import G31, case, same_rows, small_dem

pytestmark = pytest.mark.gpu


def differing(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, what
    n = int((~np.all((got == want) | (np.isnan(got) & np.isnan(want)), axis=1)).sum())
    print(f"horizon {what}: {n} of {len(want)} headings differ ({int((~np.isnan(want[:, 0])).sum())} with a point)")
    return n


def same_runs(got, want):
    return isinstance(got, list) and [r.shape for r in got] == [r.shape for r in want] and all(
        same_rows(np.ascontiguousarray(a), np.ascontiguousarray(b)) for a, b in zip(got, want))


def raster_of(c):
    from glimpse_amd import Raster

    return Raster(c["z"], x=c["xlim"], y=c["ylim"])


@pytest.mark.parametrize("name", sorted(hr.CASES))
def test_every_g31_case(golden, name):
    g = golden(G31)
    c = case(name, g)
    dem = raster_of(c)
    with np.errstate(all="ignore"):
        points = dem._horizon_points(c["origin"], c["headings"], c["correction"])
        runs = dem.horizon(c["origin"], headings=c["headings"], correction=c["correction"])
    ok = ~g[f"{name}__raised"]
    n_reference = differing(points[ok], g[f"{name}__hxyz"][ok], f"{name} against the reference")
    n_all = differing(points, c["hxyz"], f"{name} against the restatement")
    assert n_reference == 0 and n_all == 0
    assert same_rows(points, np.array(c["hxyz"])) and same_runs(runs, hr.runs(c["hxyz"]))
    # the headings the reference computes, in one call: the list it returns
    with np.errstate(all="ignore"):
        runs = dem.horizon(c["origin"], headings=np.asarray(c["headings"], dtype=float)[ok], correction=c["correction"])
    lengths = g[f"{name}__run_lengths"]
    assert [len(r) for r in runs] == list(lengths)
    if len(runs):
        assert same_rows(np.concatenate(runs, axis=0), g[f"{name}__runs"])
    if name == "one_by_one":
        assert runs == []


def test_the_default_headings_and_two_calls_give_the_same_bytes(golden):
    c = case("long_lines", golden(G31))
    dem = raster_of(c)
    first = dem._horizon_points(c["origin"], c["headings"], c["correction"])
    second = dem._horizon_points(c["origin"], c["headings"], c["correction"])
    assert first.tobytes() == second.tobytes()
    c = case("base", golden(G31))
    dem = raster_of(c)
    assert same_runs(dem.horizon(c["origin"]), hr.runs(c["hxyz"]))  # headings=range(360), correction=False


def test_three_origins_in_one_call_equal_three_calls(golden):
    from glimpse_amd import _lib

    c = case("long_lines", golden(G31))
    dem = raster_of(c)
    d = abs(dem.d[0])
    origin = c["origin"]
    origins = np.array([origin, (origin[0] - 150.3 * d, origin[1] + 60.0 * d, origin[2] - 100.0),
                        (dem.x[40], dem.y[650], float(dem.array[650, 40]) + 2.0)])
    headings = np.arange(0.0, 360.0, 1.5)
    rays = [dem._horizon_rays(tuple(o), headings) for o in origins]
    starts, ends = np.array([r[0] for r in rays]), np.array([r[1] for r in rays])
    cell, dz, times = _lib.stage_horizon(dem, origins, starts, ends, correction=True, return_times=True)
    assert cell.shape == (3, 240, 2) and cell.dtype == np.int32 and dz.shape == (3, 240) and dz.dtype == np.float64
    assert all(times[k] > 0.0 for k in _lib.HORIZON_TIMES)
    for i in range(3):
        one_cell, one_dz = _lib.stage_horizon(dem, origins[i:i + 1], starts[i:i + 1], ends[i:i + 1], correction=True)
        assert one_cell.tobytes() == cell[i:i + 1].tobytes() and one_dz.tobytes() == dz[i:i + 1].tobytes(), i
        found = cell[i, :, 0] >= 0
        assert 20 < found.sum() < 240 and np.isnan(dz[i][~found]).all() and (cell[i][~found] == -1).all()
        # against the restatement, origin by origin
        with np.errstate(all="ignore"):
            _, want = hr.horizon(c["z"], c["xlim"], c["ylim"], tuple(origins[i]), headings, True)
        assert (cell[i] == want).all(), i
    assert (cell[0] != cell[1]).any() and (cell[1] != cell[2]).any()
    again = _lib.stage_horizon(dem, origins, starts, ends, correction=True)  # nothing of the first call is left behind
    assert again[0].tobytes() == cell.tobytes() and again[1].tobytes() == dz.tobytes()


def test_argument_errors_need_no_kernel():
    from glimpse_amd import _lib

    dem = small_dem()
    with pytest.raises(ValueError, match="outside the raster"):
        dem.horizon((500.0, 22.0, 900.0))
    with pytest.raises(TypeError, match="radious"):
        dem.horizon((41.0, 22.0, 900.0), correction={"radious": 6.0e6})
    assert dem.horizon((41.0, 22.0, 900.0), headings=[]) == []
    lib = _lib.load()
    z, origin = np.zeros((4, 5)), np.array([[2.5, 2.5, 9.0]])  # (the centre of cell row 1, column 2)
    starts, ends = np.array([[2, 1]], dtype=np.int32), np.array([[[4, 0], [0, 3]]], dtype=np.int32)
    cell, dz = np.zeros((1, 2, 2), np.int32), np.zeros((1, 2))

    def call(z=z, dtype=0, ends=ends, radius=6.3781e6, corr=0):
        return lib.glh_stage_horizon(0, _lib._ptr(z), dtype, 5, 4, 0.0, 4.0, 1.0, -1.0, _lib._ptr(origin), _lib._ptr(starts),
                                     _lib._ptr(ends), 1, 2, corr, radius, 0.13, _lib._ptr(cell), _lib._ptr(dz), None)

    INVALID, UNSUPPORTED = -1, -5
    assert call(z=None) == INVALID and "null" in lib.glh_last_error().decode()
    assert call(ends=np.array([[[4, 0], [0, 4]]], dtype=np.int32)) == INVALID and "end cell" in lib.glh_last_error().decode()
    assert call(corr=1, radius=0.0) == INVALID and "radius" in lib.glh_last_error().decode()
    assert call(dtype=7) == UNSUPPORTED and "z_dtype" in lib.glh_last_error().decode()
    assert call() == 0 and (cell[0, :, 0] == -1).all()  # (a flat DEM: the farthest cell is the greatest ratio: no horizon)
