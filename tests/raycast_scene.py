"""The scenes of tests/test_raycast.py and tests/test_gpu_raycast.py: a small terrain with bumps and an oblique camera
standing inside its rectangle.

The DEM is 37 x 29 cells of 10 m: larger than one block of 16 patches on both axes and a multiple of 16 on neither.  The
camera is 64 x 48 pixels, so a 16 x 16 tile of the pixel-grid mode is cut on neither axis but the last wave of
`n = 3072` rays is full; the tests that need a ragged launch take their own ray counts.
"""
import numpy as np

NX, NY, CELL = 37, 29, 10.0
IMGSZ = (64, 48)
XYZ = (52.0, 41.0, 171.0)
VIEWDIR = (52.0, -24.0, 3.0)  # towards the far corner, pitched down: the upper rows see sky


def terrain(dtype=np.float64, seed=7):
    """z (NY, NX): a smooth slope with a ridge and three Gaussian bumps (seed 7: the first seed tried; the restatement
    misses 0 of the 3072 rays of `camera(False)` as grazes on it)."""
    rng = np.random.default_rng(seed)
    c, r = np.meshgrid(np.arange(NX, dtype=np.float64), np.arange(NY, dtype=np.float64))
    z = 100.0 + 1.1 * c + 0.6 * r + 14.0 * np.sin(c / 5.5) * np.cos(r / 4.0)
    for _ in range(3):
        bc, br, h, s = rng.uniform(6, NX - 6), rng.uniform(6, NY - 6), rng.uniform(12, 30), rng.uniform(1.5, 3.5)
        z += h * np.exp(-0.5 * ((c - bc) ** 2 + (r - br) ** 2) / s ** 2)
    return z.astype(dtype)


def dem(dtype=np.float64, x_descending=False, y_ascending=False, z=None):
    """The terrain as a Raster: x ascending and y descending, as a north-up DEM has them, unless asked otherwise (the
    world stays the same: the array is flipped with its axis)."""
    from glimpse_amd import Raster

    z = terrain(dtype) if z is None else z
    x, y = (0.0, NX * CELL), (NY * CELL, 0.0)
    if x_descending:
        z, x = z[:, ::-1], x[::-1]
    if y_ascending:
        z, y = z[::-1], y[::-1]
    return Raster(np.ascontiguousarray(z), x=x, y=y)


def camera(distorted=True, correction=False, xyz=XYZ, viewdir=VIEWDIR, imgsz=IMGSZ):
    from glimpse_amd import Camera

    extra = dict(k=(0.08, -0.03, 0.01, 0.02, 0.0, 0.0), p=(0.002, -0.001), c=(1.5, -2.0)) if distorted else {}
    return Camera(imgsz=imgsz, f=(58.0, 57.0), xyz=xyz, viewdir=viewdir, correction=correction, **extra)


def pixel_centres(imgsz=IMGSZ):
    u, v = np.meshgrid(np.arange(imgsz[0]) + 0.5, np.arange(imgsz[1]) + 0.5)
    return np.column_stack((u.ravel(), v.ravel()))


def grid_args(raster):
    """(z, x0, y0, d0, d1) of a Raster as tests/raycast_rule.py takes them."""
    d = raster.d
    return raster.array, float(raster.x[0]), float(raster.y[0]), float(d[0]), float(d[1])


def long_dem():
    """300 x 40 cells of 200 m (60 km by 8 km): far enough for the elevation correction (7 m at 10 km) to move hits from
    one patch to another.  A gentle rise away from the camera with a cross swell."""
    from glimpse_amd import Raster

    c, r = np.meshgrid(np.arange(300, dtype=np.float64), np.arange(40, dtype=np.float64))
    z = 400.0 + 1.5 * c + 40.0 * np.sin(c / 9.0) + 25.0 * np.cos(r / 6.0)
    return Raster(z, x=(0.0, 300 * 200.0), y=(40 * 200.0, 0.0))


def long_camera(correction=True):
    from glimpse_amd import Camera

    return Camera(imgsz=(64, 48), f=(120.0, 120.0), xyz=(900.0, 4100.0, 640.0), viewdir=(89.0, -1.5, 0.0),
                  correction=correction)
