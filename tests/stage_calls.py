"""The thirteen stage exports of the six stage files (glh_viewshed.hip, glh_horizon.hip, glh_regrid.hip,
glh_project_dem.hip, glh_filters.hip, glh_terrain.hip), each as one valid call through its `_lib.stage_*` wrapper on inputs
of a chosen size: what tests/test_stage_errors.py (no device: the error path) and tests/test_gpu_stage_times.py (the
times) run.
"""
import numpy as np

# export (less its glh_stage_ prefix) -> (the translation unit that runs it, the names of its times in _lib)
STAGES = {
    "viewshed": ("glh_viewshed.hip", "VIEWSHED_TIMES"),
    "horizon": ("glh_horizon.hip", "HORIZON_TIMES"),
    "raster_regrid": ("glh_regrid.hip", "REGRID_TIMES"),
    "zoom_linear": ("glh_regrid.hip", "REGRID_TIMES"),
    "raster_interpolate": ("glh_regrid.hip", "INTERPOLATE_TIMES"),
    "project_dem": ("glh_project_dem.hip", "PD_TIMES"),
    "rasterize": ("glh_project_dem.hip", "PD_TIMES"),
    "max_filter": ("glh_filters.hip", "FILTER_TIMES"),
    "gaussian_filter": ("glh_filters.hip", "FILTER_TIMES"),
    "fill_crevasses": ("glh_filters.hip", "FILTER_TIMES"),
    "gradient": ("glh_terrain.hip", "GRADIENT_TIMES"),
    "hillshade": ("glh_terrain.hip", "HILLSHADE_TIMES"),
    "polygon_mask": ("glh_terrain.hip", "POLYGON_MASK_TIMES"),
}


def calls(nx, ny, headings, window, radius):
    """{stage: f(return_times)} on a DEM of nx x ny cells of 10 m with one origin above its middle, `headings` rays, a
    `window` x `window` maximum, a Gaussian of `radius` cells and one triangle."""
    from glimpse_amd import Camera, Raster, _lib

    rng = np.random.default_rng(34)
    z, z2 = 50.0 * rng.random((ny, nx)), 50.0 * rng.random((ny, nx))
    dem = Raster(z, x=(0.0, 10.0 * nx), y=(10.0 * ny, 0.0))
    origin = np.array([5.0 * nx + 1.0, 5.0 * ny + 1.0, 60.0])
    start, ends = dem._horizon_rays(origin, np.arange(headings) * (360.0 / headings) + 10.0)
    gx, gy = (np.arange(nx) + 0.5) * 10.0, (np.arange(ny) + 0.5) * 10.0
    cam = Camera(imgsz=(8, 6), f=(6, 6), xyz=(-20.0, 5.0 * ny, 120.0), viewdir=(90.0, -30.0, 0.0))
    cols, rows = [(0, nx)], [(0, ny)]
    xc, yc = dem._tile_coordinates(0, 0, nx), dem._tile_coordinates(1, 0, ny)
    keys = (np.arange(nx * ny) % 48).astype(np.int32)
    w = np.exp(-0.5 * np.arange(-radius, radius + 1.0) ** 2)
    w /= w.sum()
    light = np.array([-0.5, 0.5, np.sqrt(0.5)])
    triangle = np.array([[0.25, 0.25], [nx - 0.25, 0.75], [0.5 * nx, ny - 0.25]])
    ring_off = np.array([0, 3], dtype=np.int32)

    def regrid(rt):
        src = _lib.regrid_src(z, gx, gy, (0.0, 10.0 * nx, 0.0, 10.0 * ny), 1, 1)
        return _lib.stage_raster_regrid(src, gx, gy, return_times=rt)

    return {
        "viewshed": lambda rt: _lib.stage_viewshed(dem, origin[None, :], return_times=rt),
        "horizon": lambda rt: _lib.stage_horizon(dem, origin[None, :], start[None, :], ends[None, :, :], return_times=rt),
        "raster_regrid": regrid,
        "zoom_linear": lambda rt: _lib.stage_zoom_linear(z, (ny + 1, nx + 1), return_times=rt),
        "raster_interpolate": lambda rt: _lib.stage_raster_interpolate(z, z2, 0.25, 0.0625, 0.5, s0=z2, s1=z, return_times=rt),
        "project_dem": lambda rt: _lib.stage_project_dem(cam.vector24, z, None, None, cols, xc, rows, yc, return_depth=True,
                                                         return_times=rt),
        "rasterize": lambda rt: _lib.stage_rasterize(keys, z.reshape(-1, 1), 48, return_times=rt),
        "max_filter": lambda rt: _lib.stage_max_filter(z, None, True, window, window, return_times=rt),
        "gaussian_filter": lambda rt: _lib.stage_gaussian_filter(z, None, True, w, w, return_times=rt),
        "fill_crevasses": lambda rt: _lib.stage_fill_crevasses(z, None, True, window, window, 0, w, w, 0, return_times=rt),
        "gradient": lambda rt: _lib.stage_gradient(z, 10.0, -10.0, return_times=rt),
        "hillshade": lambda rt: _lib.stage_hillshade(z, 10.0, 10.0, 1.0, light, 1.0, return_times=rt),
        "polygon_mask": lambda rt: _lib.stage_polygon_mask(triangle, ring_off, 1, 0, nx, ny, return_times=rt),
    }
