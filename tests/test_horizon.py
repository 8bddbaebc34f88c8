"""`Raster.horizon` without a device: the closed-form Bresenham cell against the reference's loop; the NumPy restatement
(tests/horizon_restatement.py) against what the reference wrote heading by heading (tests/golden/g31_horizon.npz), bit
for bit; the kernel's index arithmetic, transcribed into Python, against the restatement; the argument checks that come
before the library is touched, and the library's own before it touches a device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import horizon_restatement as hr
from tests import viewshed_terrain as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G31 = "g31_horizon.npz"

_built = {}


def case(name, g):
    """The case as built from the fixture's seed, with the restatement's answer on ALL its headings: computed once and
    shared (nothing below changes it)."""
    if name not in _built:
        z, xlim, ylim, origin, correction, headings = hr.build(name, int(g[f"{name}__seed"]))
        with np.errstate(all="ignore"):
            hxyz, cell = hr.horizon(z, xlim, ylim, origin, headings, correction)
        for a in (z, hxyz, cell):
            a.setflags(write=False)
        _built[name] = dict(z=z, xlim=xlim, ylim=ylim, origin=origin, correction=correction, headings=headings, hxyz=hxyz,
                            cell=cell)
    return _built[name]


def names_of(g):
    return [str(c) for c in g["cases"]]


def same_rows(a, b):
    """Rows equal bit for bit (NaN rows are written as np.nan by both sides)."""
    return a.shape == b.shape and a.dtype == b.dtype == np.float64 and a.tobytes() == b.tobytes()


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so whatever passes below happened before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


# ---- 1: the closed form ---------------------------------------------------------------------------------------------
def test_the_closed_form_cell_is_the_loops_for_every_small_line():
    start, checked = (20, 17), 0
    for ox in range(-12, 13):
        for oy in range(-12, 13):
            end = (start[0] + ox, start[1] + oy)
            want = hr.bresenham_loop(start, end)
            line = hr.line_of(start, end)
            assert line[2] + 1 == len(want) == max(abs(ox), abs(oy)) + 1
            got = hr.line_cells(line, np.arange(len(want)))
            assert (got == want).all(), (start, end)
            assert (got[0] == start).all() and (got[-1] == end).all()  # (k = 0 is the start whichever way it was swapped)
            checked += 1
    assert checked == 625
    # long lines, where j * ady passes 2^31: cells picked along the line against the loop
    for s, e in (((3, 5), (70001, 40002)), ((70001, 40002), (3, 5)), ((5, 3), (40002, 70001)), ((9, 70000), (60000, 2))):
        want = hr.bresenham_loop(s, e)
        line = hr.line_of(s, e)
        assert line[2] * line[3] > 2 ** 31
        k = np.unique(np.concatenate(([0, 1, 2, len(want) - 2, len(want) - 1], np.arange(0, len(want), 997))))
        assert (hr.line_cells(line, k) == want[k]).all()


def test_the_closed_form_and_the_loop_are_the_references_lines(golden):
    g = golden(G31)
    kinds = set()
    for k in range(int(g["lines"])):
        (start, end), want = g[f"line{k:02d}__ends"], g[f"line{k:02d}__points"]
        line = hr.line_of(start, end)
        assert (hr.bresenham_loop(start, end) == want).all(), k
        assert (hr.line_cells(line, np.arange(line[2] + 1)) == want).all(), k
        kinds.add((bool(line[6]), bool(line[7]), line[2] == 0))
    # steep / shallow, reversed / not, and the one-cell line
    assert {(False, False, False), (True, False, False), (False, True, False), (True, True, False),
            (False, False, True)} <= kinds


# ---- 2: the restatement against the reference -----------------------------------------------------------------------
def test_g31_is_what_the_reference_writes(tmp_path, golden):
    """tools/make_golden.py --g31 run again (in a process of its own: it installs stub modules) gives the committed arrays
    byte for byte.  Needs the reference; elsewhere the fixture is taken as committed."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import refstubs  # (importing installs nothing; it knows where the reference would be)
    finally:
        sys.path.pop(0)
    if not os.path.isdir(os.path.join(refstubs.REFERENCE_SRC, "glimpse")):
        pytest.skip("the reference is not on this machine")
    out = tmp_path / "g31.npz"
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden.py"), "--g31", "--out", str(out)], check=True,
                   capture_output=True, timeout=900)
    want, got = golden(G31), dict(np.load(out, allow_pickle=False))
    assert sorted(want) == sorted(got)
    for key in want:
        assert want[key].dtype == got[key].dtype and want[key].shape == got[key].shape, key
        assert want[key].tobytes() == got[key].tobytes(), key


def test_g31_covers_what_it_says(golden):
    g = golden(G31)
    names = names_of(g)
    assert sorted(names) == sorted(hr.CASES) and len(names) == 12
    for name in names:
        c = case(name, g)
        assert (vt.sha256(c["z"]) == g[f"{name}__sha256"]).all(), name  # the rebuilt DEM is the one the reference saw
        assert (np.asarray(c["origin"], dtype=float) == g[f"{name}__origin"]).all(), name
        headings, raised, hxyz = g[f"{name}__headings"], g[f"{name}__raised"], g[f"{name}__hxyz"]
        assert (np.array(c["headings"], dtype=float) == headings).all() and raised.shape == (len(headings),)
        assert hxyz.shape == (len(headings), 3) and np.isnan(hxyz[raised]).all()
        assert (~raised).mean() >= 0.2, name
        # the reference raises exactly where the unclamped end cell is outside the grid
        _, ends, raw = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], c["headings"])
        ny, nx = c["z"].shape
        outside = (raw[:, 0] < 0) | (raw[:, 0] >= nx) | (raw[:, 1] < 0) | (raw[:, 1] >= ny)
        assert (outside == raised).all() and (ends[~raised] == raw[~raised]).all(), name
        if name not in hr.RUNS_EXEMPT:
            assert len(g[f"{name}__run_lengths"]) >= 2 and (~np.isnan(hxyz[:, 0])).sum() >= 20, name
    assert hr.RUNS_EXEMPT == ("three_by_three", "one_by_one")
    for name in hr.RUNS_EXEMPT:
        assert np.isnan(case(name, g)["hxyz"]).all() and len(g[f"{name}__run_lengths"]) == 0
    # what each case is there for
    assert case("base", g)["ylim"][1] > case("base", g)["ylim"][0] and case("reversed", g)["xlim"][1] < case("reversed", g)["xlim"][0]
    c = case("reversed", g)
    start, _, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], [0.0])
    x, y = vt.centres(c["xlim"], 300), vt.centres(c["ylim"], 300)
    assert (x[start[0]], y[start[1]]) == c["origin"][:2] and len(c["headings"]) == 1440  # exactly on a cell centre
    c = case("long_lines", g)
    h = np.asarray(c["headings"])
    assert c["z"].shape == (700, 1000) and (np.diff(h) < 0).any() and len(np.unique(h)) < len(h)
    assert all(v in h for v in (0.0, 90.0, 180.0, 270.0))
    start, ends, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], h)
    assert np.abs(ends - start).max() > 2 * 256  # more than two strides of the widest workgroup
    # both workgroup sizes are met, by the rule the kernel's host side uses
    sizes = set()
    for name in names:
        c = case(name, g)
        start, ends, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], c["headings"])
        sizes.add(hr.workgroup_of(int(np.abs(ends - start).max())))
    assert sizes == {64, 256}
    # holes: missing cells inside lines, lines whose maximum is the last non-missing cell, all-missing lines
    c = case("holes", g)
    size, xlim, ylim, d = hr.grid_of(c["z"].shape, c["xlim"], c["ylim"])
    start, ends, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], c["headings"])
    inside = last_is_max = all_missing = 0
    for i in range(len(ends)):
        line = hr.line_of(start, ends[i])
        rowcol = hr.line_cells(line, np.arange(1, line[2] + 1))[:, ::-1]
        with np.errstate(all="ignore"):
            dz, ratio = hr.ratios(c["z"], xlim, ylim, d, c["origin"], c["correction"], rowcol)
        missing = np.isnan(dz)
        if missing.all():
            all_missing += 1
            continue
        inside += bool(missing[:np.nonzero(~missing)[0][-1]].any())
        last_is_max += int(np.nanargmax(ratio)) == np.nonzero(~missing)[0][-1]
    assert inside > 100 and last_is_max >= 3 and all_missing >= 3, (inside, last_is_max, all_missing)
    assert 0.01 < np.isnan(c["z"]).mean() < 0.1
    for a, b in (("correction_true", "correction_dict"),):
        assert not same_rows(case(a, g)["hxyz"], case(b, g)["hxyz"])  # the correction's arguments move the horizon
    c = case("float32_tuple", g)
    assert c["z"].dtype == np.float32 and isinstance(c["origin"], tuple) and (c["z"][:1, 0] - c["origin"][2]).dtype == np.float32
    c = case("float32_ndarray", g)
    assert c["z"].dtype == np.float32 and (c["z"][:1, 0] - c["origin"][2]).dtype == np.float64
    assert case("int16", g)["z"].dtype == np.int16
    assert case("one_by_n", g)["z"].shape == (1, 200) and case("three_by_three", g)["z"].shape == (3, 3)
    assert case("one_by_one", g)["z"].shape == (1, 1)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", G31)) < 200_000


def test_the_restatement_equals_g31_bit_for_bit(golden):
    """On every heading the reference computed: the same NaN rows and x, y, z equal in every bit (the same operations in
    the same order: no tolerance); and the runs of the non-raised headings are the reference's list."""
    g = golden(G31)
    for name in names_of(g):
        c = case(name, g)
        ok = ~g[f"{name}__raised"]
        got, want = c["hxyz"][ok], g[f"{name}__hxyz"][ok]
        differing = int((~np.all((got == want) | (np.isnan(got) & np.isnan(want)), axis=1)).sum())
        assert differing == 0 and same_rows(np.ascontiguousarray(got), np.ascontiguousarray(want)), (name, differing)
        runs, lengths = hr.runs(got), g[f"{name}__run_lengths"]
        assert [len(r) for r in runs] == list(lengths), name
        if len(runs):
            assert same_rows(np.concatenate(runs, axis=0), g[f"{name}__runs"]), name
        else:
            assert g[f"{name}__runs"].shape == (0, 3)


def test_the_circular_split():
    """hr.runs on hand-made masks: a run over the seam joins, NaN at either end does not, all NaN / no NaN."""
    def rows(present):
        h = np.full((len(present), 3), np.nan)
        for i, p in enumerate(present):
            if p:
                h[i] = i
        return h

    ids = lambda present: [[int(v) for v in r[:, 0]] for r in hr.runs(rows(present))]  # noqa: E731
    assert ids([1, 1, 0, 1, 0, 1]) == [[5, 0, 1], [3]]
    assert ids([0, 1, 1, 0, 1, 0]) == [[1, 2], [4]]
    assert ids([1, 0, 0, 1, 1, 0]) == [[0], [3, 4]]
    assert ids([0, 1, 0, 0, 1, 1]) == [[1], [4, 5]]
    assert ids([1, 1, 1]) == [[0, 1, 2]] and ids([0, 0, 0]) == [] and ids([1]) == [[0]] and ids([0]) == []
    assert hr.runs(np.zeros((0, 3))) == []


# ---- 3: the kernel's index arithmetic -------------------------------------------------------------------------------
def test_the_kernels_striding_and_reduction_choose_the_restatements_cell(golden):
    """Every heading of every case through hr.kernel_line -- lanes striding over k, the skipped start cell, reversal, the
    butterfly within a wave and the waves in order, the tie rule -- at the workgroup size the host would launch and at
    the other one."""
    g = golden(G31)
    lines = 0
    for name in names_of(g):
        c = case(name, g)
        size, xlim, ylim, d = hr.grid_of(c["z"].shape, c["xlim"], c["ylim"])
        start, ends, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], c["headings"])
        tb = hr.workgroup_of(int(np.abs(ends - start).max()))
        for i in range(len(ends)):
            line = hr.line_of(start, ends[i])
            rowcol = hr.line_cells(line, np.arange(1, line[2] + 1))[:, ::-1]
            with np.errstate(all="ignore"):
                dz, ratio = hr.ratios(c["z"], xlim, ylim, d, c["origin"], c["correction"], rowcol)
            for width in (tb, 320 - tb):
                k = hr.kernel_line(dz, ratio, width)
                got = rowcol[k - 1] if k > 0 else np.array((-1, -1))
                assert (got == c["cell"][i]).all(), (name, i, width)
            lines += 1
    assert lines > 3000


def test_the_reduction_keeps_the_first_of_equal_ratios():
    dz = np.ones(700)
    for ties in ([5, 69, 300, 699], [64, 65], [255, 256, 511], [0, 699]):
        ratio = np.zeros(700)
        ratio[ties] = 2.0
        for tb in (64, 256):
            assert hr.kernel_line(dz, ratio, tb) == ties[0] + 1, (ties, tb)
    # the maximum in the last cell with a value: no horizon; a value beyond it: a horizon
    ratio = np.arange(700.0)
    assert hr.kernel_line(dz, ratio, 256) == -1 and hr.kernel_line(dz, ratio, 64) == -1
    gap = dz.copy()
    gap[650:] = np.nan
    assert hr.kernel_line(gap, ratio, 256) == -1
    gap[699] = 1.0
    ratio[699] = 0.0
    assert hr.kernel_line(gap, ratio, 256) == 650 and hr.kernel_line(gap, ratio, 64) == 650
    assert hr.kernel_line(np.full(9, np.nan), np.full(9, np.nan), 64) == -1 and hr.kernel_line(dz[:0], dz[:0], 64) == -1
    assert hr.kernel_line(np.array([1.0, 1.0]), np.array([-np.inf, -np.inf]), 64) == 1  # (-inf is a value)


# ---- the argument checks ----------------------------------------------------------------------------------------------
def small_dem():
    from glimpse_amd import Raster

    return Raster(vt.terrain((6, 8), 1), x=(0.0, 80.0), y=(60.0, 0.0))


def test_bad_arguments_are_refused_before_the_library(no_library):
    from glimpse_amd import Raster, _lib

    dem = small_dem()
    with pytest.raises(TypeError, match="radious"):  # (before anything else: the origin is outside as well)
        dem.horizon((500.0, 22.0, 900.0), correction={"radious": 6.0e6})
    with pytest.raises(TypeError, match="DEM of dtype"):
        Raster(np.zeros((6, 8), dtype=complex), x=(0.0, 80.0), y=(60.0, 0.0)).horizon((41.0, 22.0, 900.0))
    with pytest.raises(ValueError, match="outside the raster"):
        dem.horizon((500.0, 22.0, 900.0))
    with pytest.raises(ValueError, match="outside the raster"):
        dem.horizon((41.0, -0.001, 900.0), headings=[10.0], correction=True)
    with pytest.raises(ValueError, match="two-dimensional"):
        Raster(np.zeros((6, 8, 3)), x=(0.0, 80.0), y=(60.0, 0.0)).horizon((41.0, 22.0, 900.0))
    assert dem.horizon((41.0, 22.0, 900.0), headings=[]) == []
    assert dem.horizon((41.0, 22.0, 900.0), headings=np.zeros(0)) == []
    with pytest.raises(_lib.GlhError):  # (a good call reaches the library)
        dem.horizon((41.0, 22.0, 900.0))


def test_the_rays_are_the_restatements(golden):
    """Raster._horizon_rays (the host part of the method) gives the start and the clamped end cells of the restatement."""
    from glimpse_amd import Raster

    g = golden(G31)
    for name in names_of(g):
        c = case(name, g)
        dem = Raster(c["z"], x=c["xlim"], y=c["ylim"])
        start, ends = dem._horizon_rays(tuple(float(v) for v in c["origin"]), c["headings"])
        want_start, want_ends, _ = hr.rays(c["z"].shape, c["xlim"], c["ylim"], c["origin"], c["headings"])
        assert (start == want_start).all() and (ends == want_ends).all(), name


def test_the_library_refuses_what_it_cannot_trace():
    """glh_stage_horizon is exported and checks its arguments before it touches a device."""
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    assert "glh_stage_horizon" in _lib.SIGNATURES and hasattr(lib, "glh_stage_horizon")
    z = np.zeros((4, 5))
    origin = np.array([[2.2, 1.1, 9.0]])
    starts, ends = np.array([[2, 1]], dtype=np.int32), np.array([[[4, 0], [0, 3]]], dtype=np.int32)
    cell, dz = np.zeros((1, 2, 2), np.int32), np.zeros((1, 2))

    def call(z=z, dtype=0, nx=5, ny=4, x0=0.0, y0=4.0, d0=1.0, d1=-1.0, origin=origin, starts=starts, ends=ends, m=1, n=2,
             corr=0, radius=6.3781e6, refraction=0.13, cell=cell, dz=dz):
        return lib.glh_stage_horizon(0, _lib._ptr(z), dtype, nx, ny, x0, y0, d0, d1, _lib._ptr(origin), _lib._ptr(starts),
                                     _lib._ptr(ends), m, n, corr, radius, refraction, _lib._ptr(cell), _lib._ptr(dz), None)

    INVALID, UNSUPPORTED = -1, -5
    assert call(z=None) == INVALID and "null" in lib.glh_last_error().decode()
    for name in ("origin", "starts", "ends", "cell", "dz"):
        assert call(**{name: None}) == INVALID, name
    assert call(nx=0) == INVALID and call(ny=0) == INVALID and call(m=0) == INVALID and call(n=0) == INVALID
    assert call(nx=65536, ny=32768) == INVALID and "2^31" in lib.glh_last_error().decode()
    assert call(m=4096, n=4096) == INVALID and "2^24" in lib.glh_last_error().decode()  # (a launch holds < 2^32 lanes)
    assert call(dtype=2) == UNSUPPORTED and "z_dtype" in lib.glh_last_error().decode()
    assert call(d0=0.0) == INVALID and call(d1=float("nan")) == INVALID and call(x0=float("inf")) == INVALID
    assert call(origin=np.array([[np.inf, 0.0, 0.0]])) == INVALID and "origin" in lib.glh_last_error().decode()
    assert call(corr=1, radius=0.0) == INVALID and "radius" in lib.glh_last_error().decode()
    assert call(starts=np.array([[5, 1]], dtype=np.int32)) == INVALID and "start cell" in lib.glh_last_error().decode()
    assert call(starts=np.array([[2, -1]], dtype=np.int32)) == INVALID
    for bad in ([[4, 0], [0, 4]], [[-1, 0], [0, 3]], [[4, 0], [5, 3]]):
        assert call(ends=np.array([bad], dtype=np.int32)) == INVALID and "end cell" in lib.glh_last_error().decode(), bad
