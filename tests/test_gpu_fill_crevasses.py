"""`Raster.fill_crevasses`, `maximum_filter` and `gaussian_filter` on the device, through the Python API and so through the
C ABI (`glh_stage_fill_crevasses`, `glh_stage_max_filter`, `glh_stage_gaussian_filter`; kernels `k_fl_max`, `k_fl_gauss`).

Expected: equal to the reference (g30), to the NumPy restatement and to scipy.ndimage in EVERY value, with the same NaN
pattern (`==`: -0.0 against +0.0 from a maximum is not a difference).  There is no tolerance: the device adds, multiplies
and divides in SciPy's order with the host's weight tables.  Every test prints its count of differing cells before it
asserts that the count is 0.
"""
import numpy as np
import pytest

from tests import fill_crevasses_restatement as fr
from tests.test_fill_crevasses import G30, OUTPUTS, case_of, scipy_fill_crevasses

pytestmark = pytest.mark.gpu


def scipy_ndimage():
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return None
    return ndi


def differing(got, want, what):
    n = fr.mismatches(got, want)
    print(f"fill_crevasses {what}: {n} of {want.size} cells differ (NaN in the result: {int(np.isnan(want).sum())})")
    return n


def through_the_api(z, maximum, gaussian, mask, fill):
    """The three results of a case: Raster.fill_crevasses (a callable mask goes in as it is) and the two functions."""
    from glimpse_amd import Raster, gaussian_filter, maximum_filter

    dem = Raster(z.copy())
    assert dem.fill_crevasses(maximum=maximum, gaussian=gaussian, mask=mask, fill=fill) is None
    array_mask = fr.resolved(mask, z)
    return {"fill_crevasses": dem.array, "maximum": maximum_filter(z, mask=array_mask, fill=fill, **maximum),
            "gaussian": gaussian_filter(z, mask=array_mask, fill=fill, **gaussian)}


def test_every_g30_case_in_every_value(golden):
    g = golden(G30)
    counts = {}
    for name in (str(c) for c in g["cases"]):
        z, maximum, gaussian, mask, fill = case_of(name, g)
        before = z.copy()
        got = through_the_api(z, maximum, gaussian, mask, fill)
        assert before.tobytes() == z.tobytes(), name  # (the functions return new arrays)
        for what in OUTPUTS:
            counts[name, what] = differing(got[what], g[f"{name}__{what}"], f"{name} {what}")
    assert not any(counts.values()), {k: n for k, n in counts.items() if n}


def test_the_fused_call_equals_the_two_functions_chained_and_two_calls_give_identical_bytes(golden):
    from glimpse_amd import Raster, gaussian_filter, maximum_filter

    g = golden(G30)
    for name in ("holes_keep", "holes_fill", "block_fill", "float32_holes_fill", "size_3x7", "sigma_2_0", "defaults"):
        z, maximum, gaussian, mask, fill = case_of(name, g)
        array_mask = fr.resolved(mask, z)
        first, second = Raster(z.copy()), Raster(z.copy())
        first.fill_crevasses(maximum=maximum, gaussian=gaussian, mask=mask, fill=fill)
        second.fill_crevasses(maximum=maximum, gaussian=gaussian, mask=mask, fill=fill)
        assert first.array.tobytes() == second.array.tobytes(), name
        chained = gaussian_filter(maximum_filter(z, mask=array_mask, fill=fill, **maximum), mask=array_mask, fill=fill, **gaussian)
        assert differing(first.array, chained, f"{name} fused against chained") == 0
        assert chained.tobytes() == first.array.tobytes(), name


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_every_tile_seam_and_halo_fold(dtype):
    """300 rows x 217 columns: more than twice the maximum's tile (16 rows x 64 columns) plus one in each direction, no
    multiple of the wave's 64 lanes nor of the Gaussian's 256-cell workgroups; sigma 5 (radius 20) with a mask, `fill`
    off and on; and the widest window with a radius that folds the 217 columns more than once."""
    ndi = scipy_ndimage()
    rng = np.random.default_rng(300217)
    z = fr.crevassed((300, 217), 30).astype(dtype)
    mask = rng.random(z.shape) > 0.07
    mask[100:160, 60:130] = False
    z[~mask] = np.nan
    total = 0
    for maximum, gaussian, fill in (({"size": 5}, {"sigma": 5}, False), ({"size": 5}, {"sigma": 5}, True),
                                    ({"size": (31, 30), "mode": "mirror"}, {"sigma": 40, "radius": (128, 500), "mode": "wrap"}, True)):
        got = through_the_api(z, maximum, gaussian, mask, fill)
        want = {"fill_crevasses": fr.fill_crevasses(z, maximum, gaussian, mask, fill),
                "maximum": fr.maximum_filter(z, mask, fill, **maximum),
                "gaussian": fr.gaussian_filter(z, mask, fill, **gaussian)}
        for what in OUTPUTS:
            total += differing(got[what], want[what], f"300 x 217 {dtype} {maximum} {gaussian} fill={fill} {what}")
            if ndi is not None:
                scipys = scipy_fill_crevasses(ndi, z, maximum, gaussian, mask, fill, stage=what)
                total += differing(got[what], scipys, f"... against scipy.ndimage, {what}")
    assert total == 0


def test_a_dem_of_1024_x_1536_with_holes_filled():
    """float64, 5 % of the cells excluded, fill=True, the defaults: against scipy.ndimage through the reference's formulas
    (the restatement stands in where SciPy is not installed)."""
    from glimpse_amd import Raster

    ndi = scipy_ndimage()
    z = fr.crevassed((1024, 1536), 1024)
    mask = np.random.default_rng(1536).random(z.shape) >= 0.05
    z[~mask] = np.nan
    dem = Raster(z.copy())
    dem.fill_crevasses(mask=mask, fill=True)
    maximum, gaussian = {"size": 5}, {"sigma": 5}
    if ndi is not None:
        want = scipy_fill_crevasses(ndi, z, maximum, gaussian, mask, True)
    else:
        want = fr.fill_crevasses(z, maximum, gaussian, mask, True)
    assert 0.04 < (~mask).mean() < 0.06 and not np.isnan(want).any()
    assert differing(dem.array, want, "1024 x 1536") == 0
