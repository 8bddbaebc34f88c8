"""`Camera.project_dem` and `Camera.rasterize` on the device, through the Python API and so through the C ABI
(`glh_stage_project_dem`, `glh_stage_rasterize`; kernels `k_pd_project`, `k_pd_keep_winners`, rocPRIM's radix sort,
`k_pd_runs`, `k_pd_reduce`).

Expected: the NaN pattern of the reference (g29) in every pixel, the value layers BIT FOR BIT (they are inputs summed in
the reference's order), the depth layer within rtol 1e-12 (tests/test_gpu_parity.py's relative tolerance for the same
projection: the reference rotates with BLAS, the device operation by operation).  The g29 cases keep every cell 1e-6 px
from a pixel border, so the device's projection (within 1e-9) cannot move a cell to another pixel.
"""
import numpy as np
import pytest

from tests import project_dem_restatement as pr
from tests import viewshed_terrain as vt
from tests.test_project_dem import same

pytestmark = pytest.mark.gpu

G29 = "g29_project_dem.npz"
DEPTH_RTOL = 1e-12


def camera_of(vec):
    from glimpse_amd import Camera

    correction = {"radius": vec[21], "refraction": vec[22]} if vec[20] else False
    return Camera(imgsz=vec[6:8].astype(int), f=vec[8:10], c=vec[10:12], k=vec[12:18], p=vec[18:20], xyz=vec[0:3],
                  viewdir=vec[3:6], correction=correction)


def run_case(c, **kwargs):
    from glimpse_amd import Raster

    args = dict(values=c["values"], mask=c["mask"], tile_size=c["tile_size"], tile_overlap=c["tile_overlap"],
                return_depth=c["return_depth"])
    args.update(kwargs)
    return camera_of(c["cam"]).project_dem(Raster(c["z"], x=c["xlim"], y=c["ylim"]), **args)


def device_project(cam, xyz):
    from glimpse_amd import _lib

    return _lib.stage_project_depth(cam, xyz)


def test_every_g29_case(golden):
    g = golden(G29)
    for name in (str(c) for c in g["cases"]):
        c = pr.g29_case(g, name)
        got, want = run_case(c), c["image"]
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        n_values = want.shape[2] - int(c["return_depth"])
        assert same(got[:, :, :n_values], want[:, :, :n_values]), name
        if c["return_depth"]:
            hit = ~np.isnan(want[:, :, -1])
            err = np.max(np.abs(got[:, :, -1][hit] - want[:, :, -1][hit]) / np.abs(want[:, :, -1][hit]))
            print(f"project_dem {name}: depth relative error {err:.3g}")
            assert err <= DEPTH_RTOL, name


def test_two_calls_give_identical_bytes_and_the_tiling_is_part_of_the_answer(golden):
    g = golden(G29)
    for name in ("tiles40x24_distorted", "far_field"):
        c = pr.g29_case(g, name)
        assert run_case(c).tobytes() == run_case(c).tobytes(), name
    small, single = (run_case(pr.g29_case(g, name)) for name in ("tiles32", "single_tile"))
    assert np.array_equal(np.isnan(small), np.isnan(single)) and not same(small, single)
    # the same case under another tiling than its own is the restatement's image under that tiling (occluding tiles:
    # the camera looks across the DEM)
    c = pr.g29_case(g, "tiles32")
    ny, nx = c["z"].shape
    d = ((c["xlim"][1] - c["xlim"][0]) / nx, (c["ylim"][1] - c["ylim"][0]) / ny)
    for size, overlap in (((64, 16), (2, 5)), ((2, 50), (1, 0))):  # (the second: tiles two cells wide)
        want = pr.project_dem(c["cam"], c["z"], vt.centres(c["xlim"], nx), vt.centres(c["ylim"], ny), d, values=c["values"],
                              tile_size=size, tile_overlap=overlap, return_depth=True, project=device_project)
        assert same(run_case(c, tile_size=size, tile_overlap=overlap, return_depth=True), want), size
        assert not same(want[:, :, :1], small)


def test_the_docstring_example_and_the_value_types(golden):
    from glimpse_amd import Camera, Raster

    g = golden(G29)
    cam = Camera(imgsz=3, f=3, xyz=(0, 0, 3), viewdir=(0, -90, 0))
    Z = np.array([(0.1, 0.2, 0.3), (0.4, 0.5, 0.6), (0.7, 0.8, 0.9)])
    img = cam.project_dem(Raster(Z, x=(-1, 0, 1), y=(1, 0, -1)), values=g["doctest__values"], return_depth=True)
    assert np.all(img[:, :, 0] == g["doctest__values"]) and np.all(img[:, :, 1] == cam.xyz[2] - Z)
    assert same(img, g["doctest__image"])
    # bool, integer and 2-d values are the float64 they convert to
    c = pr.g29_case(g, "mask_u8_dem32")
    want = run_case(c, values=c["values"].astype(np.float64))
    assert same(run_case(c), want) and same(run_case(c, values=c["values"].astype(np.int64)), want)
    flags = c["values"][:, :, 0] > 127
    assert same(run_case(c, values=flags), run_case(c, values=flags.astype(np.float64)))
    assert same(run_case(c, values=flags), run_case(c, values=flags.astype(np.uint16)))
    # an integer DEM
    zi = np.floor(c["z"]).astype(np.int16)
    assert same(run_case(dict(c, z=zi)), run_case(dict(c, z=zi.astype(np.float64))))


def test_rasterize_is_bit_for_bit(golden):
    from glimpse_amd import Camera

    g = golden(G29)
    got = Camera(imgsz=(3, 2), f=1).rasterize(uv=np.array([(0.5, 0.5), (2.5, 1.5), (2.5, 1.5)]), values=np.array([1, 2, 4]))
    assert same(got, g["rasterize_doctest__image"])
    cam = Camera(imgsz=(64, 48), f=40)
    uv, values = pr.rasterize_inputs(2929, 5000, (64, 48))
    assert same(cam.rasterize(uv, values), g["rasterize_points__image"])
    assert same(cam.rasterize(uv, values[:, 0]), g["rasterize_points__one_column"])
    assert same(cam.rasterize(uv, values[:, :1]), g["rasterize_points__one_column"])
    assert np.isnan(cam.rasterize(uv - 1000.0, values)).all()  # (no point in the frame)
    # runs either side of the reduction's switch from one thread to the wavefront (64 cells), and across its 64-cell steps
    counts = [1, 2, 63, 64, 65, 127, 128, 129, 1000, 0, 5, 64, 63]
    keys = np.repeat(np.arange(len(counts)), counts)
    rng = np.random.default_rng(29)
    keys = keys[rng.permutation(len(keys))]
    cam = Camera(imgsz=(len(counts), 1), f=1)
    uv = np.column_stack((keys + 0.5, np.full(len(keys), 0.25)))
    values = rng.integers(-2 ** 40, 2 ** 40, size=(len(keys), 3)) / 2.0 ** 20 * 10.0 ** rng.integers(-6, 7, size=(len(keys), 1))
    got = cam.rasterize(uv, values)
    assert same(got, pr.rasterize((len(counts), 1), uv, values)) and np.isnan(got[0, 9]).all()


def test_a_megapixel_image_of_a_million_cells():
    """1024 x 1024 cells into 1024 x 768 pixels, tiles of 256, against the restatement on the device's own coordinates
    (`glh_stage_project_depth`): pixel membership is out of the comparison, so every layer is bit for bit."""
    from glimpse_amd import Camera, Raster, _lib

    z = vt.holes(vt.terrain((1024, 1024), 2931), 2932, 0.01, (300, 340, 500, 560))
    xlim, ylim = (0.0, 10240.0), (10240.0, 0.0)
    rng = np.random.default_rng(2933)
    values = (rng.integers(-2 ** 20, 2 ** 20, size=(1024, 1024, 2)) / 2.0 ** 8).astype(np.float32)
    cam = Camera(imgsz=(1024, 768), f=(250, 260), c=(3.5, -2.25), k=(0.05, -0.01), p=(0.001, -0.002),
                 xyz=(-500.0, 5120.3, float(np.nanmax(z)) + 150.0), viewdir=(90.0, -5.0, 1.0))
    dem = Raster(z, x=xlim, y=ylim)
    got, times = _lib.stage_project_dem(
        cam.vector24, z, values, None, *_axes(dem, (256, 256), (1, 1)), return_depth=True, return_times=True)
    assert same(got, cam.project_dem(dem, values=values, return_depth=True))
    want, counts = pr.project_dem(cam.vector24, z, dem.x, dem.y, dem.d, values=values, return_depth=True,
                                  project=device_project, return_counts=True)
    print("project_dem 1024^2:", {k: round(v, 3) for k, v in times.items()}, "most cells in a pixel", counts.max())
    assert counts.max() > 256 and ((counts > 0) & (counts < 64)).sum() > 10000 and (counts == 0).sum() > 10000
    assert times["memberships"] == 1027 * 1027 and times["kept"] == counts.sum()
    assert same(got, want)


def _axes(dem, size, overlap):
    tiles = dem.tile_indices(size, overlap)
    rows = list(dict.fromkeys((i.start, i.stop) for i, _ in tiles))
    cols = list(dict.fromkeys((j.start, j.stop) for _, j in tiles))
    return (cols, np.concatenate([dem._tile_coordinates(0, a, b) for a, b in cols]),
            rows, np.concatenate([dem._tile_coordinates(1, a, b) for a, b in rows]))


def test_the_depth_map_of_what_a_viewshed_origin_sees():
    """End to end with Raster.viewshed: a camera at the origin, the visible cells as mask.  Shape and NaN pattern only --
    the reference's project_dem does no occlusion, so visibility is not asserted."""
    from glimpse_amd import Camera, Raster

    z, xlim, ylim, origin, _ = vt.build("y_ascending", 2800)
    dem = Raster(z, x=xlim, y=ylim)
    visible = dem.viewshed(origin)
    cam = Camera(imgsz=(160, 120), f=90, xyz=origin, viewdir=(40.0, -20.0, 0.0))
    depth = cam.project_dem(dem, mask=visible, tile_size=(100, 100), return_depth=True)
    _, counts = pr.project_dem(cam.vector24, z, dem.x, dem.y, dem.d, mask=visible, tile_size=(100, 100), return_depth=True,
                               project=device_project, return_counts=True)
    assert depth.shape == (120, 160, 1) and depth.dtype == np.float64
    assert np.array_equal(~np.isnan(depth[:, :, 0]), counts > 0) and 100 < (counts > 0).sum() < counts.size
    assert np.all(depth[counts > 0] > 0)
