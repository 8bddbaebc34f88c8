"""`Camera.project_dem`, `Camera.rasterize` and `Raster.tile_indices` without a device: the NumPy restatement
(tests/project_dem_restatement.py) equals the reference's images of tests/golden/g29_project_dem.npz bit for bit; the
fixture's cases meet the admission rule and cover what they say; the tiling equals the reference's slices; the argument
errors come before the library is touched; the built library exports the two entry points and refuses bad arguments
without a device."""
import numpy as np
import pytest

from tests import project_dem_restatement as pr
from tests import viewshed_terrain as vt

G29 = "g29_project_dem.npz"
MARGIN = 1e-6


@pytest.fixture
def no_library(monkeypatch, tmp_path):
    """Any attempt to load the HIP library fails (GlhError), so whatever passes below happened before one."""
    from glimpse_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))


def same(a, b):
    """NaN in the same places, every other value the same bits."""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.nan_to_num(a).tobytes() == np.nan_to_num(b).tobytes()


def test_the_restatement_equals_g29_bit_for_bit(golden):
    g = golden(G29)
    for name in (str(c) for c in g["cases"]):
        c = pr.g29_case(g, name)
        ny, nx = c["z"].shape
        x, y = vt.centres(c["xlim"], nx), vt.centres(c["ylim"], ny)
        d = ((c["xlim"][1] - c["xlim"][0]) / nx, (c["ylim"][1] - c["ylim"][0]) / ny)
        got, counts = pr.project_dem(c["cam"], c["z"], x, y, d, values=c["values"], mask=c["mask"],
                                     tile_size=c["tile_size"], tile_overlap=c["tile_overlap"],
                                     return_depth=c["return_depth"], return_counts=True)
        assert same(got, c["image"]), name  # value layers and depth alike
        assert np.array_equal(counts, c["counts"]), name
        assert np.array_equal(counts == 0, np.isnan(c["image"][:, :, -1])), name


def test_g29_meets_the_admission_rule_and_covers_its_cases(golden):
    g = golden(G29)
    names = [str(c) for c in g["cases"]]
    cases = {n: pr.g29_case(g, n) for n in names}
    for n, c in cases.items():
        assert c["margins"][0] >= MARGIN and c["margins"][1] >= MARGIN, n
        assert np.isfinite(c["image"]).any() and np.isnan(c["image"]).any(), n
    assert {c["tile_size"] for c in cases.values()} >= {(32, 32), (40, 24), (256, 256)}
    assert {c["tile_overlap"] for c in cases.values()} >= {(1, 1), (0, 0), (3, 2)}
    assert cases["far_field"]["counts"].max() > 256  # (the wavefront's path of the reduction)
    assert any(0 < c["counts"].max() < 64 for c in cases.values())  # (and the single thread's alone)
    assert any(c["cam"][12:20].all() for c in cases.values()) and any(c["cam"][20] for c in cases.values())
    assert any(np.isnan(c["z"]).any() for c in cases.values()) and any(c["mask"] is not None for c in cases.values())
    assert any(c["z"].dtype == np.float32 for c in cases.values())
    assert {c["ylim"][0] < c["ylim"][1] for c in cases.values()} == {True, False}
    kinds = {(None if c["values"] is None else (c["values"].dtype.name, np.atleast_3d(c["values"]).shape[2]), c["return_depth"])
             for c in cases.values()}
    assert {(None, True), (("float64", 1), False), (("float64", 3), True)} <= kinds
    assert {k[0][0] for k in kinds if k[0]} >= {"float32", "uint8", "uint16"}
    # the tile size is part of the answer: same inputs, another tiling, same pixels hit, other values
    a, b = cases["tiles32"], cases["single_tile"]
    assert np.array_equal(a["z"], b["z"]) and np.array_equal(a["cam"], b["cam"])
    assert np.array_equal(np.isnan(a["image"]), np.isnan(b["image"])) and not same(a["image"], b["image"])
    # cells behind the camera in the "inside" cases
    c = cases["inside_depth_only"]
    ny, nx = c["z"].shape
    X, Y = np.meshgrid(vt.centres(c["xlim"], nx), vt.centres(c["ylim"], ny))
    depth = pr.camera_project(c["cam"], np.column_stack((X.ravel(), Y.ravel(), c["z"].ravel())))[1]
    assert (depth < 0).sum() > 1000 and (depth > 0).sum() > 1000


def test_the_doctests(golden):
    g = golden(G29)
    Z = np.array([(0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (0.7, 0.8, 0.9)])
    cam = np.zeros(24)
    cam[0:3], cam[3:6], cam[6:8], cam[8:10] = (0, 0, 3), (0, -90, 0), 3, 3
    got = pr.project_dem(cam, Z, np.array((-1.0, 0.0, 1.0)), np.array((1.0, 0.0, -1.0)), (1.0, -1.0),
                         values=g["doctest__values"], return_depth=True)
    assert same(got, g["doctest__image"]) and np.all(got[:, :, 0] == g["doctest__values"])
    got = pr.rasterize((3, 2), np.array([(0.5, 0.5), (2.5, 1.5), (2.5, 1.5)]), np.array([1, 2, 4]))
    assert same(got, g["rasterize_doctest__image"]) and got[1, 2] == 3.0 and got[0, 0] == 1.0
    uv, values = pr.rasterize_inputs(2929, 5000, (64, 48))
    assert same(pr.rasterize((64, 48), uv, values), g["rasterize_points__image"])
    assert same(pr.rasterize((64, 48), uv, values[:, 0]), g["rasterize_points__one_column"])
    assert len(np.unique(uv, axis=0)) < len(uv)  # (repeated points)


def test_tile_indices_are_the_references(golden, no_library):
    from glimpse_amd import Raster

    g = golden(G29)
    assert int(g["tilings"]) >= 6
    single = 0
    for k in range(int(g["tilings"])):
        ny, nx, sx, sy, ox, oy = (int(v) for v in g[f"tiling{k}__args"])
        want = [tuple(int(v) for v in row) for row in g[f"tiling{k}__slices"]]
        tiles = Raster(np.zeros((ny, nx))).tile_indices(size=(sx, sy), overlap=(ox, oy))
        assert [(i.start, i.stop, j.start, j.stop) for i, j in tiles] == want, k
        assert pr.tile_slices((ny, nx), (sx, sy), (ox, oy)) == want, k
        single += want == [(0, ny, 0, nx)]
    assert single >= 2  # (n = 0: a DEM smaller than half a tile is one tile)
    assert Raster(np.zeros((4, 6))).tile_indices(size=(3, 2)) == Raster(np.zeros((4, 6))).tile_indices((3, 2), (0, 0))


def test_a_narrow_tile_spaces_its_own_coordinates(no_library):
    """Tiles of one or two cells along an axis are built from limits (raster.py:689-692); wider ones keep the slice."""
    from glimpse_amd import Raster

    dem = Raster(np.zeros((5, 7)), x=(0.3, 70.3), y=(50.1, 0.1))
    for dim, coords, d in ((0, dem.x, dem.d[0]), (1, dem.y, dem.d[1])):
        for start, stop in ((0, 1), (2, 4), (1, 4), (0, len(coords)), (len(coords) - 2, len(coords))):
            got = dem._tile_coordinates(dim, start, stop)
            assert np.array_equal(got, pr.tile_axis(coords, d, start, stop))
            assert np.allclose(got, coords[start:stop], rtol=0, atol=1e-9)
            if stop - start >= 3:
                assert np.array_equal(got, coords[start:stop])


def test_the_argument_errors_come_before_the_library(no_library):
    from glimpse_amd import Camera, Raster

    cam = Camera(imgsz=(8, 6), f=10, xyz=(0, 0, 50), viewdir=(0, -90, 0))
    dem = Raster(np.ones((4, 5)), x=(0.0, 5.0), y=(4.0, 0.0))
    with pytest.raises(ValueError, match="^values does not have the same 2-d shape as dem$"):
        cam.project_dem(dem, values=np.ones((5, 4)))
    with pytest.raises(ValueError, match="^values cannot be missing if return_depth is False$"):
        cam.project_dem(dem)
    with pytest.raises(ValueError, match="^mask does not have the same 2-d shape as dem$"):
        cam.project_dem(dem, values=np.ones((4, 5, 2)), mask=np.ones((4, 4), bool))
    # the reference's order: values first, then the mask
    with pytest.raises(ValueError, match="^values does not"):
        cam.project_dem(dem, values=np.ones((5, 4)), mask=np.ones((4, 4), bool))
    for limits in ((0.5, 1), (1, 2), (0.5, 2)):
        with pytest.raises(NotImplementedError, match="scale_limits"):  # (before anything else)
            cam.project_dem(dem, values=np.ones((5, 4)), scale_limits=limits)
    from glimpse_amd import _lib

    with pytest.raises(_lib.GlhError):  # (good arguments reach the library, which is not there)
        cam.project_dem(dem, values=np.ones((4, 5)), scale=3, parallel=True)
    with pytest.raises(_lib.GlhError):
        cam.rasterize(np.array([(0.5, 0.5)]), np.array([1.0]))


def test_the_library_refuses_bad_arguments_without_a_device():
    from glimpse_amd import _lib, build

    build.build(verbose=False)
    lib = _lib.load()
    for name in ("glh_stage_project_dem", "glh_stage_rasterize"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    INVALID, UNSUPPORTED = -1, -5
    cam = np.zeros(24)
    cam[6:8], cam[8:10], cam[2] = (8, 6), 10, 50
    z, vals, out = np.zeros((4, 5)), np.zeros((4, 5, 1)), np.zeros((6, 8, 2))
    xs, xe, ys, ye = (np.array(v, dtype=np.int32) for v in ([0, 2], [3, 5], [0], [4]))
    xc, yc = np.arange(6.0), np.arange(4.0)

    def call(cam=cam, z=z, zt=0, nx=5, ny=4, mask=None, vals=vals, vt_=0, layers=1, ntx=2, xs=xs, xe=xe, xc=xc, nty=1, ys=ys,
             ye=ye, yc=yc, depth=1, out=out):
        p = _lib._ptr
        return lib.glh_stage_project_dem(0, p(cam), p(z), zt, nx, ny, p(mask), p(vals), vt_, layers, ntx, p(xs), p(xe), p(xc),
                                         nty, p(ys), p(ye), p(yc), depth, p(out), None)

    def message():
        return lib.glh_last_error().decode()

    assert call(cam=None) == INVALID and "null" in message()
    for missing in ("z", "xs", "xe", "xc", "ys", "ye", "yc", "out"):
        assert call(**{missing: None}) == INVALID, missing
    assert call(nx=0) == INVALID and call(ny=-1) == INVALID and call(ntx=0) == INVALID and call(nty=0) == INVALID
    assert call(vals=None) == INVALID and call(layers=0) == INVALID and call(layers=-1) == INVALID
    assert call(vals=None, layers=0, depth=0) == INVALID and "neither" in message()
    assert call(zt=2) == UNSUPPORTED and "z_dtype" in message()
    assert call(vt_=4) == UNSUPPORTED and call(vt_=-1) == UNSUPPORTED and "v_dtype" in message()
    grid = cam.copy()
    grid[23] = 1
    assert call(cam=grid) == UNSUPPORTED
    for bad in ((0, 6), (8.5, 6), (np.nan, 6)):
        odd = cam.copy()
        odd[6:8] = bad
        assert call(cam=odd) == INVALID and "imgsz" in message()
    i32 = lambda *v: np.array(v, dtype=np.int32)  # noqa: E731
    assert call(xs=i32(2, 0), xe=i32(5, 3)) == INVALID and "ascending" in message()
    assert call(xs=i32(0, 2), xe=i32(5, 5)) == INVALID and "ascending" in message()
    assert call(xs=i32(0, 3), xe=i32(3, 6)) == INVALID and call(xs=i32(-1, 2), xe=i32(3, 5)) == INVALID
    assert call(xs=i32(0, 3), xe=i32(3, 3)) == INVALID and call(ys=i32(0), ye=i32(5)) == INVALID
    assert call(nx=65536, ny=32768, xe=i32(3, 65536), ye=i32(32768)) == UNSUPPORTED and "2^31" in message()

    keys, values, image = np.array([0, 3, 3], dtype=np.int32), np.ones((3, 2)), np.zeros((6, 2))

    def rcall(keys=keys, n=3, values=values, layers=2, npix=6, image=image):
        return lib.glh_stage_rasterize(0, _lib._ptr(keys), n, _lib._ptr(values), layers, npix, _lib._ptr(image), None)

    assert rcall(keys=None) == INVALID and rcall(values=None) == INVALID and rcall(image=None) == INVALID
    assert rcall(n=0) == INVALID and rcall(layers=0) == INVALID and rcall(npix=0) == INVALID
    assert rcall(npix=3) == INVALID and "key 3" in message()
    assert rcall(keys=np.array([0, -1, 3], dtype=np.int32)) == INVALID
