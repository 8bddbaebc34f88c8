"""`Raster.fill_crevasses`, `maximum_filter` and `gaussian_filter` without a device: the committed g30 fixture is what the
reference writes (regenerated where the reference is present) and covers the cases it says; the NumPy restatement
(tests/fill_crevasses_restatement.py) equals it in every value and equals scipy.ndimage on random shapes; what is not
served is refused before the library is touched; the built library exports the three stages and refuses bad arguments
without a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fill_crevasses_restatement as fr
from tests import viewshed_terrain as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G30 = "g30_fill_crevasses.npz"
OUTPUTS = ("fill_crevasses", "maximum", "gaussian")


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so whatever passes below happened before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def case_of(name, g):
    return fr.build(name, int(g[f"{name}__seed"]))


def scipy_fill_crevasses(ndi, a, maximum, gaussian, mask=None, fill=False, stage="fill_crevasses"):
    """The reference's formulas (helpers.py:347-430, raster.py:1266-1291) around scipy.ndimage `ndi` itself."""
    def top(a):
        if mask is None:
            return ndi.maximum_filter(a, **maximum)
        lowest = np.finfo(a.dtype).min
        x = a.copy()
        x[~mask] = lowest
        x = ndi.maximum_filter(x, **maximum)
        put = x == lowest if fill else ~mask
        x[put] = a[put]
        return x

    def smooth(a):
        if mask is None:
            return ndi.gaussian_filter(a, **gaussian)
        x = a.copy()
        x[~mask] = 0
        xf = ndi.gaussian_filter(x, **gaussian)
        x[mask] = 1
        with np.errstate(all="ignore"):
            x = xf / ndi.gaussian_filter(x, **gaussian)
        if not fill:
            x[~mask] = a[~mask]
        return x

    return {"maximum": top, "gaussian": smooth, "fill_crevasses": lambda a: smooth(top(a))}[stage](a)


def test_the_restatement_equals_g30_in_every_value(golden):
    g = golden(G30)
    for name in (str(c) for c in g["cases"]):
        z, maximum, gaussian, mask, fill = case_of(name, g)
        array_mask = fr.resolved(mask, z)
        got = {"fill_crevasses": fr.fill_crevasses(z, maximum, gaussian, mask, fill),
               "maximum": fr.maximum_filter(z, array_mask, fill, **maximum),
               "gaussian": fr.gaussian_filter(z, array_mask, fill, **gaussian)}
        for what in OUTPUTS:
            assert fr.mismatches(got[what], g[f"{name}__{what}"]) == 0, (name, what)


def test_g30_covers_what_it_says(golden):
    g = golden(G30)
    names = [str(c) for c in g["cases"]]
    assert sorted(names) == sorted(fr.CASES) and len(names) == 21
    built = {}
    for name in names:
        z, maximum, gaussian, mask, fill = built[name] = case_of(name, g)
        assert (vt.sha256(z) == g[f"{name}__sha256"]).all(), name  # the rebuilt input is the one the reference saw
        for what in OUTPUTS:
            assert g[f"{name}__{what}"].shape == z.shape and g[f"{name}__{what}"].dtype == z.dtype, (name, what)
        assert (g[f"{name}__fill_crevasses"] != z).any(), name
    assert built["defaults"][1:] == ({"size": 5}, {"sigma": 5}, None, False) and built["defaults"][0].shape == (40, 56)
    # the crevasses are there, and the filter fills them: the smoothed surface lies above the input nearly everywhere
    assert (g["defaults__maximum"] >= built["defaults"][0]).all()
    assert (g["defaults__maximum"] - built["defaults"][0]).max() > 20
    for name in ("holes_keep", "holes_fill"):
        z, _, _, mask, fill = built[name]
        assert 0.03 < (~mask).mean() < 0.15 and np.isnan(z[~mask]).all() and fill == (name == "holes_fill")
    keep, z = g["holes_keep__fill_crevasses"], built["holes_keep"][0]
    assert np.isnan(keep[np.isnan(z)]).all() and not np.isnan(g["holes_fill__fill_crevasses"]).any()
    # a block wider than the Gaussian's reach: fill=True leaves NaN in its middle, and only there
    z, _, gaussian, mask, fill = built["block_fill"]
    reach = int(4.0 * gaussian["sigma"] + 0.5)
    out = g["block_fill__fill_crevasses"]
    assert fill and np.isnan(out).any() and not mask[8:32, 10:40].any()
    assert np.isnan(out[8 + reach:32 - reach, 10 + reach:40 - reach]).all() and not np.isnan(out[mask]).any()
    assert callable(built["callable_mask"][3]) and callable(built["docstring_keep"][3])
    assert built["float32"][0].dtype == np.float32 and g["float32__fill_crevasses"].dtype == np.float32
    assert built["float32_holes_fill"][0].dtype == np.float32 and built["float32_holes_fill"][4]
    assert built["size_3x7"][1] == {"size": (3, 7)} and built["size_4"][1] == {"size": 4}
    assert built["sigma_2_0"][2] == {"sigma": (2, 0)} and built["sigma_1p5_3_truncate_3"][2] == {"sigma": (1.5, 3), "truncate": 3}
    assert sorted(built[f"mode_{m}"][2]["mode"] for m in ("reflect", "nearest", "mirror", "wrap")) == \
        ["mirror", "nearest", "reflect", "wrap"]
    assert built["shorter_than_radius"][0].shape == (7, 9) and built["shorter_than_radius"][2] == {"sigma": 5}
    assert built["one_row"][0].shape == (1, 60) and built["one_column"][0].shape == (60, 1)
    # the helpers' docstring examples (helpers.py:370-375, :413-418)
    nan = np.nan
    assert np.array_equal(g["docstring_keep__maximum"], [[nan, 2], [2, nan]], equal_nan=True)
    assert np.array_equal(g["docstring_fill__maximum"], [[2, 2], [2, 2]])
    assert np.allclose(g["docstring_keep__gaussian"], [[nan, 1.23154033], [1.76845967, nan]], equal_nan=True, atol=1e-8, rtol=0)
    assert np.allclose(g["docstring_fill__gaussian"], [[1.5, 1.23154033], [1.76845967, 1.5]], atol=1e-8, rtol=0)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G30)) < 400_000


def test_the_restatement_equals_scipy_on_random_shapes():
    """Bit for bit: every mode, float64 and float32, sides shorter than the radius, even and odd windows, masks."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(30)
    for trial in range(60):
        shape = (int(rng.integers(1, 48)), int(rng.integers(1, 48)))
        a = rng.normal(size=shape).astype(("float64", "float32")[trial % 2]) * 100
        mode = ("reflect", "nearest", "mirror", "wrap", "grid-mirror", "grid-wrap")[trial % 6]
        sigma = (5, 1.3, 0.7, (2, 0), (1.5, 3))[trial % 5]
        size = (5, 4, (3, 7), 1, (2, 6))[trial % 5]
        gaussian = {"sigma": sigma, "mode": mode, **({"truncate": 3} if trial % 4 == 0 else {})}
        maximum = {"size": size, "mode": mode}
        assert fr.same(fr.scipy_gaussian(a, **gaussian), ndi.gaussian_filter(a, **gaussian)), (trial, shape, gaussian)
        assert fr.same(fr.scipy_maximum(a, **maximum), ndi.maximum_filter(a, **maximum)), (trial, shape, maximum)
        mask = rng.random(shape) > 0.2
        for fill in (False, True):
            want = scipy_fill_crevasses(ndi, a, maximum, gaussian, mask, fill)
            assert fr.same(fr.fill_crevasses(a, maximum, gaussian, mask, fill), want), (trial, shape, fill)
    # the 300 x 217 arrays of the parity statement, and SciPy's even window: its centre sits at size // 2
    for dtype in ("float64", "float32"):
        a = rng.normal(size=(300, 217)).astype(dtype)
        for sigma in (5, 1.3, 0.7):
            assert fr.same(fr.scipy_gaussian(a, sigma), ndi.gaussian_filter(a, sigma))
    ramp = np.arange(10.0)[None, :]
    assert (ndi.maximum_filter(ramp, size=(1, 4))[0] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9]).all()
    assert (fr.scipy_maximum(ramp, (1, 4))[0] == [1, 2, 3, 4, 5, 6, 7, 8, 9, 9]).all()


def test_the_weights_are_the_restatements_and_skipped_axes_are_none():
    from glimpse_amd import filters

    for sigma, truncate, radius in ((5, 4.0, None), (1.5, 3, None), (0.7, 4.0, None), (3, 4.0, 9), (2.0, 4.0, 0)):
        w = filters.gaussian_weights(sigma, truncate, radius)
        assert w.dtype == np.float64 and w.tobytes() == fr.gaussian_weights(sigma, truncate, radius).tobytes()
        assert (w == w[::-1]).all() and len(w) == 2 * (int(truncate * sigma + 0.5) if radius is None else radius) + 1
    assert filters.gaussian_weights(0, 4.0, None) is None and filters.gaussian_weights(1e-15, 4.0, None) is None
    w0, w1, mode = filters.gaussian_arguments({"sigma": (2, 0), "mode": "grid-wrap"})
    assert len(w0) == 17 and w1 is None and mode == 3
    assert filters.maximum_arguments({"size": (3, 7)}) == (3, 7, 0) and filters.maximum_arguments({"size": 4, "mode": "mirror"}) == (4, 4, 2)
    with pytest.raises(ValueError, match="Radius must be a nonnegative integer"):
        filters.gaussian_arguments({"sigma": 2, "radius": -1})


def test_what_is_not_served_is_refused_before_the_library(no_library):
    from glimpse_amd import Raster, _lib, gaussian_filter, maximum_filter

    a = fr.crevassed((6, 8), 1)
    for name, value in (("footprint", np.ones((3, 3))), ("origin", 1), ("output", np.empty_like(a)), ("axes", (0,)),
                        ("cval", 1.0)):
        with pytest.raises(NotImplementedError, match=f"`{name}`"):
            maximum_filter(a, size=3, **{name: value})
        with pytest.raises(NotImplementedError, match=f"`{name}`"):
            Raster(a).fill_crevasses(maximum={"size": 3, name: value})
    for name, value in (("order", 1), ("output", np.empty_like(a)), ("axes", (0,)), ("cval", 1.0)):
        with pytest.raises(NotImplementedError, match=f"`{name}`"):
            gaussian_filter(a, sigma=2, **{name: value})
        with pytest.raises(NotImplementedError, match=f"`{name}`"):
            Raster(a).fill_crevasses(gaussian={"sigma": 2, name: value})
    for call in (lambda: maximum_filter(a, size=3, mode="constant"), lambda: gaussian_filter(a, sigma=2, mode="constant"),
                 lambda: Raster(a).fill_crevasses(gaussian={"sigma": 5, "mode": "constant"})):
        with pytest.raises(NotImplementedError, match="`mode`"):
            call()
    # scipy's defaults spelled out are not a request for something else: these reach the library (which is not there)
    with pytest.raises(_lib.GlhError):
        maximum_filter(a, size=3, origin=0, cval=0.0, footprint=None)
    with pytest.raises(_lib.GlhError):
        gaussian_filter(a, sigma=2, order=0, output=None)
    for dtype in (np.int16, np.uint8, np.int64, bool):
        with pytest.raises(NotImplementedError, match="convert it first"):
            maximum_filter(a.astype(dtype), size=3)
        with pytest.raises(NotImplementedError, match="convert it first"):
            gaussian_filter(a.astype(dtype), sigma=2)
        with pytest.raises(NotImplementedError, match="convert it first"):
            Raster(a.astype(dtype)).fill_crevasses()
    holed = a.copy()
    holed[2, 3] = np.nan
    mask = ~np.isnan(holed)
    for call in (lambda: maximum_filter(holed, size=3), lambda: gaussian_filter(holed, sigma=2),
                 lambda: Raster(holed).fill_crevasses(), lambda: gaussian_filter(holed, sigma=2, mask=np.ones_like(mask)),
                 lambda: Raster(holed).fill_crevasses(mask=lambda z: np.ones(z.shape, bool))):
        with pytest.raises(ValueError, match="`mask`") as info:
            call()
        assert "NaN at 1 included cells (the first at row 2, column 3)" in str(info.value)
    with pytest.raises(_lib.GlhError):  # (the NaN excluded: served)
        Raster(holed).fill_crevasses(mask=mask)
    for call in (lambda: maximum_filter(a, mask=mask[:, :5], size=3), lambda: gaussian_filter(a, mask=mask[:4], sigma=2),
                 lambda: Raster(a).fill_crevasses(mask=mask.T)):
        with pytest.raises(ValueError, match="`mask` of shape"):
            call()
    with pytest.raises(RuntimeError, match="no footprint or filter size provided"):
        maximum_filter(a)
    with pytest.raises(TypeError, match="sigma"):
        gaussian_filter(a)
    with pytest.raises(TypeError, match="unexpected keyword argument 'sise'"):
        maximum_filter(a, sise=3)
    with pytest.raises(RuntimeError, match="boundary mode not supported"):
        gaussian_filter(a, sigma=2, mode="edge")


def test_g30_is_what_the_reference_writes(tmp_path, golden):
    """tools/make_golden.py --g30 run again (in a process of its own: it installs stub modules) gives the committed arrays
    byte for byte.  Needs the reference; elsewhere the fixture is taken as committed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import refstubs  # (importing installs nothing; it knows where the reference would be)
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(refstubs.REFERENCE_SRC, "glimpse")):
        pytest.skip("the reference is not on this machine")
    out = tmp_path / "g30.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden.py"), "--g30", "--out", str(out)], check=True,
                   capture_output=True, timeout=900)
    want, got = golden(G30), dict(np.load(out, allow_pickle=False))
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key].dtype == got[key].dtype and want[key].shape == got[key].shape, key
        assert want[key].tobytes() == got[key].tobytes(), key


def test_the_library_refuses_what_the_kernels_do_not_take():
    """The three stages are exported and check their arguments before they touch a device."""
    from glimpse_amd import _lib, build, filters

    build.build(verbose=False)
    lib = _lib.load()
    for name in ("glh_stage_max_filter", "glh_stage_gaussian_filter", "glh_stage_fill_crevasses"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    a, out = np.zeros((4, 5)), np.zeros((4, 5))
    w = filters.gaussian_weights(1.0)
    ptr = _lib._ptr

    def top(a=a, dtype=0, nx=5, ny=4, sy=5, sx=5, mode=0, out=out):
        return lib.glh_stage_max_filter(0, ptr(a), dtype, nx, ny, None, 0, sy, sx, mode, ptr(out), None)

    def smooth(a=a, dtype=0, nx=5, ny=4, w0=w, r0=4, w1=w, r1=4, mode=0, out=out):
        return lib.glh_stage_gaussian_filter(0, ptr(a), dtype, nx, ny, None, 0, ptr(w0), r0, ptr(w1), r1, mode, ptr(out), None)

    def both(sy=5, sx=5, max_mode=0, w0=w, r0=4, gauss_mode=0, a=a):
        return lib.glh_stage_fill_crevasses(0, ptr(a), 0, 5, 4, None, 0, sy, sx, max_mode, ptr(w0), r0, ptr(w), 4, gauss_mode,
                                            ptr(out), None)

    INVALID, UNSUPPORTED = -1, -5
    assert top(a=None) == INVALID and "null" in lib.glh_last_error().decode()
    assert top(out=None) == INVALID and smooth(a=None) == INVALID and smooth(out=None) == INVALID and both(a=None) == INVALID
    assert top(nx=0) == INVALID and top(ny=0) == INVALID and smooth(nx=0) == INVALID
    assert top(nx=65536, ny=32768) == INVALID and "2^31" in lib.glh_last_error().decode()
    assert top(dtype=2) == UNSUPPORTED and smooth(dtype=-1) == UNSUPPORTED and "dtype" in lib.glh_last_error().decode()
    assert top(sy=0) == INVALID and top(sx=-3) == INVALID
    assert top(sy=32) == UNSUPPORTED and "31" in lib.glh_last_error().decode() and top(sx=33) == UNSUPPORTED
    assert top(mode=4) == UNSUPPORTED and top(mode=-1) == UNSUPPORTED and smooth(mode=4) == UNSUPPORTED
    assert smooth(r0=-1) == INVALID
    wide = np.ones(2 * 4097 + 1)
    assert smooth(w0=wide, r0=4097) == UNSUPPORTED and "4096" in lib.glh_last_error().decode()
    bad = w.copy()
    bad[1] = np.nan
    assert smooth(w1=bad) == INVALID and "finite" in lib.glh_last_error().decode()
    skew = w.copy()
    skew[0] *= 2
    assert smooth(w0=skew) == UNSUPPORTED and "symmetric" in lib.glh_last_error().decode()
    assert both(sy=40) == UNSUPPORTED and both(max_mode=7) == UNSUPPORTED and both(gauss_mode=7) == UNSUPPORTED
    assert both(w0=skew) == UNSUPPORTED and both(r0=-2) == INVALID
