"""`Raster.viewshed` without a device: the warnings, the argument checks and the one-cell answer come before the library
is touched; the committed g28 fixture is what the reference writes (regenerated where the reference is present) and
covers the cases it says; the NumPy restatement (tests/viewshed_restatement.py) equals it in every cell; the built
library exports `glh_stage_viewshed` and refuses bad arguments without a device."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from tests import viewshed_restatement as vr
from tests import viewshed_terrain as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G28 = "g28_viewshed.npz"


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so whatever passes below happened before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def raster_of(name, g):
    from glimpse_amd import Raster

    z, xlim, ylim, origin, correction = vt.build(name, int(g[f"{name}__seed"]))
    return Raster(z, x=xlim, y=ylim), origin, correction


def expected(name, g):
    shape = tuple(int(v) for v in g[f"{name}__shape"])
    return np.unpackbits(g[f"{name}__visible"])[: shape[0] * shape[1]].astype(bool).reshape(shape)


def test_the_warnings_come_first_and_word_for_word(no_library):
    from glimpse_amd import Raster, _lib

    dem = Raster(vt.terrain((6, 8), 1), x=(0.0, 80.0), y=(30.0, 0.0))  # cells 10 x 5
    with pytest.warns(UserWarning) as record:
        with pytest.raises(_lib.GlhError):  # (the library is asked for only after both warnings)
            dem.viewshed((500.0, 10.0, 900.0))
    texts = [str(w.message) for w in record]
    assert texts == ["DEM cells not square " + str(tuple(abs(dem.d))) + " - may lead to unexpected results",
                     "Origin not in DEM - may lead to unexpected results"]
    square = Raster(vt.terrain((6, 8), 1), x=(0.0, 80.0), y=(60.0, 0.0))
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (square cells, origin inside: no warning)
        with pytest.raises(_lib.GlhError):
            square.viewshed((41.0, 22.0, 900.0))


def test_bad_arguments_are_type_errors_before_the_library(no_library):
    from glimpse_amd import Raster

    dem = Raster(vt.terrain((6, 8), 1), x=(0.0, 80.0), y=(60.0, 0.0))
    with pytest.raises(TypeError, match="radious"):
        dem.viewshed((41.0, 22.0, 900.0), correction={"radious": 6.0e6})
    for bad in (np.zeros((6, 8), dtype=complex), np.zeros((6, 8), dtype=np.float16), np.zeros((6, 8), dtype="U1")):
        with pytest.raises(TypeError, match="DEM of dtype"):
            Raster(bad, x=(0.0, 80.0), y=(60.0, 0.0)).viewshed((41.0, 22.0, 900.0))


def test_a_raster_inside_ring_zero_is_all_visible_without_the_library(no_library, golden):
    g = golden(G28)
    dem, origin, correction = raster_of("one_by_one", g)
    got = dem.viewshed(origin, correction=correction)
    assert got.dtype == bool and got.shape == (1, 1) and got.all()
    assert (got == expected("one_by_one", g)).all()


def test_the_float32_flag_follows_numpys_own_promotion():
    """A float32 DEM less a Python float stays float32, less a NumPy float64 becomes float64 (NEP 50): asked of NumPy on
    one element, not guessed.  Integers are computed in float64."""
    from glimpse_amd import _lib

    z32 = vt.terrain((4, 4), 3).astype(np.float32)
    for origin_z, want in ((812.3, (z32[:1, 0] - 812.3).dtype), (np.float64(812.3), (z32[:1, 0] - np.float64(812.3)).dtype)):
        z, flag = _lib.viewshed_dem(z32, origin_z)
        assert z.dtype == want and flag == (_lib.VIEWSHED_F32 if want == np.float32 else _lib.VIEWSHED_F64)
    z, flag = _lib.viewshed_dem(np.arange(16, dtype=np.int16).reshape(4, 4), 3.5)
    assert z.dtype == np.float64 and flag == _lib.VIEWSHED_F64
    z, flag = _lib.viewshed_dem(np.arange(16, dtype=np.int16).reshape(4, 4), 3)
    assert z.dtype == np.float64 and flag == _lib.VIEWSHED_F64


def test_g28_is_what_the_reference_writes(tmp_path, golden):
    """tools/make_golden.py --g28 run again (in a process of its own: it installs stub modules) gives the committed arrays
    byte for byte.  Needs the reference; elsewhere the fixture is taken as committed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import refstubs  # (importing installs nothing; it knows where the reference would be)
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(refstubs.REFERENCE_SRC, "glimpse")):
        pytest.skip("the reference is not on this machine")
    out = tmp_path / "g28.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden.py"), "--g28", "--out", str(out)], check=True,
                   capture_output=True, timeout=900)
    want, got = golden(G28), dict(np.load(out, allow_pickle=False))
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key].dtype == got[key].dtype and want[key].shape == got[key].shape, key
        assert want[key].tobytes() == got[key].tobytes(), key


def test_g28_covers_what_it_says(golden):
    g = golden(G28)
    names = [str(c) for c in g["cases"]]
    assert sorted(names) == sorted(vt.CASES) and len(names) == 14
    built = {}
    for name in names:
        dem, origin, correction = raster_of(name, g)
        built[name] = (dem, origin, correction)
        assert (vt.sha256(dem.array) == g[f"{name}__sha256"]).all(), name  # the rebuilt DEM is the one the reference saw
        assert (np.asarray(origin, dtype=float) == g[f"{name}__origin"]).all(), name
        want = expected(name, g)
        assert want.shape == dem.array.shape and dem.array.size <= 1024 * 1024, name
        if name not in vt.FRACTION_EXEMPT:
            assert 0.01 <= want.mean() <= 0.99, (name, want.mean())  # ("all False" cannot pass)
    assert vt.FRACTION_EXEMPT == ("one_by_one",) and expected("one_by_one", g).all()
    # what each case is there for
    ring = {n: vr.cell_stage(d.array, d.x, d.y, 1 / abs(d.d[0]), o)[0] for n, (d, o, c) in built.items()}
    assert (ring["summit_mast"] == 0).sum() == 1 and ring["summit_mast"].min() == 0  # between centres: ring 0 is one cell
    dem, origin, _ = built["cell_centre"]
    under = np.unravel_index(np.argmin(ring["cell_centre"]), dem.array.shape)
    assert (dem.x[under[1]], dem.y[under[0]]) == origin[:2]  # exactly on a cell centre ...
    assert not expected("cell_centre", g)[under]  # ... whose cell is never tested
    assert ring["outside"].min() > 1 and not built["outside"][0].inbounds_xy(np.atleast_2d(built["outside"][1][:2]))[0]
    assert built["y_ascending"][0].d[1] > 0 and built["summit_mast"][0].d[1] < 0 and built["x_descending"][0].d[0] < 0
    assert built["shape_700x1000"][0].array.shape == (700, 1000)
    dem, origin, _ = built["nan_holes"]
    first = ring["nan_holes"] == np.unique(ring["nan_holes"])[1]  # (ring 0 exists: the first processed ring is the next)
    nan_first = np.isnan(dem.array.ravel()[first])
    assert nan_first.any() and not nan_first.all() and 0.01 < np.isnan(dem.array).mean() < 0.05
    for name in ("correction_true", "correction_dict"):
        dem, origin, correction = built[name]
        plain = vr.of_raster(dem, origin, False)
        assert (plain != expected(name, g)).sum() > 100, name  # coarse enough that the correction changes cells
    assert (expected("correction_true", g) != expected("correction_dict", g)).any()
    assert built["float32_tuple"][0].array.dtype == np.float32 and isinstance(built["float32_tuple"][1], tuple)
    assert isinstance(built["float32_ndarray"][1], np.ndarray) and built["int16"][0].array.dtype == np.int16
    assert built["one_by_one"][0].array.shape == (1, 1) and built["one_by_n"][0].array.shape == (1, 200)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G28)) < 1_000_000


def test_the_periodic_interpolation_is_numpys(golden):
    """interp_periodic -- the sweep's interpolation spelled out, which the kernel follows -- against the installed
    np.interp(period=2 pi) bit for bit: random rings, knot hits, x = 0, x that wraps to the period itself, headings at
    +-pi, NaN and infinite values at the knots, rings of one and two cells."""
    rng = np.random.default_rng(28)
    checked = 0
    for trial in range(400):
        n = int(rng.choice([1, 2, 3, 4, 5, 8, 33, 200]))
        xp = np.sort(rng.uniform(-np.pi, np.pi, n))
        if trial % 5 == 0:
            xp[-1] = np.pi
        if trial % 7 == 0 and n > 2:
            xp[n // 2] = 0.0
            xp = np.sort(xp)
        if trial % 11 == 0:
            xp = np.sort(np.where(xp < 0, xp, -xp - 1e-3))  # all negative
        if trial % 13 == 0:
            xp = np.abs(xp)
            xp = np.sort(xp)  # none negative
        if len(np.unique(vr.np_mod(xp))) != n:
            continue
        fp = rng.normal(size=n)
        if trial % 3 == 0:
            fp[rng.integers(0, n, max(1, n // 4))] = np.nan
        if trial % 17 == 0:
            fp[rng.integers(0, n, 2)] = np.inf
        if trial % 19 == 0:
            fp[rng.integers(0, n, 2)] = -np.inf
        x = np.concatenate((rng.uniform(-np.pi, np.pi, 40), xp, [0.0, -1e-20, np.pi, -np.pi + 1e-9, 1e-300, -1e-300]))
        with np.errstate(all="ignore"):
            want = np.interp(x, xp, fp, period=2 * np.pi)
            got = vr.interp_periodic(x, xp, fp)
        assert want.tobytes() == got.tobytes() or np.array_equal(want, got, equal_nan=True), trial
        checked += len(x)
    assert checked > 5000
    assert vr.np_mod(np.array([-1e-20]))[0] == 2 * np.pi and (np.array([-1e-20]) % (2 * np.pi))[0] == 2 * np.pi


@pytest.mark.parametrize("spelled_out", [False, True])
def test_the_restatement_equals_g28_in_every_cell(golden, spelled_out):
    g = golden(G28)
    for name in (str(c) for c in g["cases"]):
        dem, origin, correction = raster_of(name, g)
        pair = None
        if correction is True:
            correction = {}
        if isinstance(correction, dict):
            pair = (correction.get("radius", 6.3781e6), correction.get("refraction", 0.13))
        with np.errstate(all="ignore"):
            got = vr.viewshed(dem.array, dem.x, dem.y, 1 / abs(dem.d[0]), origin, pair,
                              interp=vr.interp_periodic if spelled_out else None)
        assert got.dtype == bool and (got != expected(name, g)).sum() == 0, name


def test_the_library_refuses_what_it_cannot_sweep():
    """glh_stage_viewshed is exported and checks its arguments before it touches a device."""
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert "glh_stage_viewshed" in _lib.SIGNATURES and hasattr(lib, "glh_stage_viewshed")
    z = np.zeros((4, 5))
    x, y = np.arange(5.0), np.arange(4.0)
    origin, out = np.array([[2.2, 1.1, 9.0]]), np.zeros((1, 4, 5), np.uint8)

    def call(z=z, dtype=0, nx=5, ny=4, x=x, y=y, inv=1.0, origin=origin, m=1, corr=0, radius=6.3781e6, refraction=0.13,
             out=out):
        return lib.glh_stage_viewshed(0, _lib._ptr(z), dtype, nx, ny, _lib._ptr(x), _lib._ptr(y), inv, _lib._ptr(origin), m,
                                      corr, radius, refraction, _lib._ptr(out), None)

    INVALID, UNSUPPORTED = -1, -5
    assert call(z=None) == INVALID and "null" in lib.glh_last_error().decode()
    assert call(x=None) == INVALID and call(y=None) == INVALID and call(origin=None) == INVALID and call(out=None) == INVALID
    assert call(nx=0) == INVALID and call(ny=0) == INVALID and call(m=0) == INVALID
    assert call(nx=65536, ny=32768) == INVALID and "2^31" in lib.glh_last_error().decode()
    assert call(dtype=2) == UNSUPPORTED and "z_dtype" in lib.glh_last_error().decode()
    assert call(inv=0.0) == INVALID and call(inv=float("nan")) == INVALID
    assert call(x=np.array([0, 1, np.nan, 3, 4.0])) == INVALID
    assert call(origin=np.array([[np.inf, 0.0, 0.0]])) == INVALID
    assert call(corr=1, radius=0.0) == INVALID
    assert call(origin=np.array([[1e9, 0.0, 0.0]])) == UNSUPPORTED and "cells" in lib.glh_last_error().decode()
