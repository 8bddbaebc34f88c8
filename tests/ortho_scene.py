"""The scenes of the orthorectification tests (tests/test_orthorectify.py on the host, tests/test_gpu_orthorectify.py and
tests/test_gpu_orthorectify_batches.py on the device): plain NumPy arrays and `glimpse_amd` objects, no library call.

The closed-form scene is the nadir scene of `Camera.project_dem`'s docstring flattened: a camera 3 above the middle of a
3 x 3 DEM of zeros, looking straight down with f = 3, so that in exact arithmetic every cell centre lands on a pixel
centre and the orthophoto is the frame itself.  In float64 cos(-90 degrees) is 6.1e-17, not 0, and the cells of the
first two rows land 2^-52 px below their pixel centre's row (v = 0.5 + 2^-52, 1.5 + 2^-52; the last row and every u are
exact).  A bilinear sample there is fl(fl(a (1 - 2^-52)) + b 2^-52) for the pixel's value a and the value b below it.
With every value in the lower half of one binade, 8 < a, b < 12, the product a (1 - 2^-52) = a - 1.0x ulp rounds to
a - ulp (ulp = 2^-49), b 2^-52 is between 1 and 1.5 ulp, and the sum rounds back to a: the frame below is chosen so, which
makes "the result is the frame, bit for bit" a property of the rule under "linear" as well, not a matter of luck.

The agreement scene is the smallest that can still go wrong: a DEM of 37 x 29 cells (neither side a multiple of the
32 x 8 workgroup, more than one workgroup along both), descending y, a sloping plane with a ridge across the view and
three NaN cells; a frame of 48 x 40 pixels; an oblique camera inside the DEM with every distortion coefficient and the
elevation correction set, so that some cells are behind it, some project outside the frame and some land within half a
pixel of its edge; a mask that excludes a block of cells the camera would see.

The batch (`stations`) is eight such cameras at three positions, in an order that interleaves the positions, so that a
call over them needs four masks: one per position, and a second one at the first position whose camera has no elevation
correction.  With the Earth's radius the correction moves no cell of a viewshed over 37 cells, and two masks that are
equal could be swapped unnoticed; the corrected cameras of the first position therefore carry a radius of 400, under
which the ridge hides 40 cells more.  Every station's view directions were picked on the host until each frame has the
cells the agreement scene has, and at least ten cells whose value is there under its own mask and not under each other
one (or the reverse): tests/test_orthorectify.py pins that.
"""
import datetime

import numpy as np

T0 = datetime.datetime(2021, 6, 1)
NX, NY, FW, FH = 37, 29, 48, 40
NAN_CELLS = ((6, 11), (15, 20), (21, 17))  # (row, col), each among cells the camera sees
MASK_BLOCK = (slice(16, 20), slice(15, 19))
VIEWDIRS = ((4.0, -24.0, 3.0), (-9.0, -21.0, -2.0), (13.0, -28.0, 1.0))  # one position, three view directions
ODD_SIZE = (47, 39)  # a second frame shape: no byte count of it is a multiple of 16, that of uint8 x 3 not one of 4
POSITIONS = ((17.83, 4.29, 3.37), (7.41, 6.63, 4.12), (29.27, 3.58, 5.21))
SMALL_EARTH = {"radius": 400.0, "refraction": 0.13}  # (a correction that changes the viewshed of a DEM this small)


def closed_form():
    """(camera arguments, frame (3, 3) float64, x, y, z) of the nadir scene."""
    frame = 8.5 + 0.25 * np.array([[4.0, 0.0, 7.0], [2.0, 8.0, 5.0], [6.0, 3.0, 1.0]])
    return (dict(imgsz=3, f=3, xyz=(0, 0, 3), viewdir=(0, -90, 0)), frame, np.array([-1.0, 0.0, 1.0]),
            np.array([1.0, 0.0, -1.0]), np.zeros((3, 3)))


def dem_arrays():
    """(x (NX,), y (NY,) descending, z (NY, NX)): a plane rising to the north-east with a ridge along y = 14."""
    x, y = np.arange(NX) + 0.5, (np.arange(NY) + 0.5)[::-1].copy()
    X, Y = np.meshgrid(x, y)
    z = 0.04 * X + 0.07 * Y + 2.2 * np.exp(-0.5 * ((Y - 14.0) / 1.3) ** 2) * (0.6 + 0.4 * np.cos(0.3 * X))
    for cell in NAN_CELLS:
        z[cell] = np.nan
    return x, y, z


def camera_arguments(viewdir=VIEWDIRS[0], position=0, correction=True, imgsz=(FW, FH)):
    return dict(imgsz=imgsz, f=(31.0, 29.5), c=(1.3, -0.8), k=(0.05, -0.02, 0.005, 0.01, -0.004, 0.002),
                p=(0.003, -0.002), xyz=POSITIONS[position], viewdir=viewdir, correction=correction)


def stations():
    """The batch: eight (position index, viewdir, correction), the positions interleaved.  Four mask keys in order of
    first appearance: position 0 corrected, position 1, position 0 uncorrected (entry 2, the same place as entries 0
    and 5: the key differs by the correction alone), position 2."""
    return [(0, (-29.63, -19.7, 2.0), dict(SMALL_EARTH)), (1, (24.37, -19.7, 2.0), True),
            (0, (-41.63, -22.7, 2.0), False), (2, (-2.63, -16.7, -3.0), True),
            (1, (27.37, -16.7, -3.0), True), (0, (-35.63, -25.7, 2.0), dict(SMALL_EARTH)),
            (2, (3.37, -22.7, -3.0), True), (1, (24.37, -25.7, -3.0), True)]


STATION_MASKS = (0, 1, 2, 3, 1, 0, 3, 1)  # each station's mask, the masks numbered by first appearance


def station_camera(station, imgsz=(FW, FH)):
    from glimpse_amd import Camera

    position, viewdir, correction = station
    return Camera(**camera_arguments(viewdir, position, correction, imgsz))


def discrimination(valued, masks, mask_of):
    """Over every frame i and every mask B other than its own A = masks[mask_of[i]]: the smallest number of cells that
    have a value in frame i under exactly one of A and B, `valued[i]` being the cells of frame i that have a value
    without any mask.  A frame shown through another frame's mask differs from the right answer in at least that many
    cells' NaN pattern."""
    return min(int((valued[i] & (masks[a] ^ masks[b])).sum())
               for i, a in enumerate(mask_of) for b in range(len(masks)) if b != a)


def mask():
    m = np.ones((NY, NX), dtype=bool)
    m[MASK_BLOCK] = False
    return m


def frame(dtype, channels, seed=0, size=(FW, FH)):
    """A frame (h, w) or (h, w, 3) of `dtype`, `size` = (w, h): smooth waves plus noise, gradients everywhere, no two
    neighbours equal for the float types."""
    rng = np.random.default_rng(100 + seed)
    w, h = size
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [0.3 * np.sin(0.21 * u + c) + 0.3 * np.cos(0.17 * v - c) + 0.2 * np.sin(0.11 * (u + v)) + 0.2 * rng.random((h, w))
              for c in range(channels)]
    a = (np.stack(planes, axis=2) + 0.8) / 1.81  # in [0, 1)
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        a = np.floor(a * 256.0)
    elif dtype == np.uint16:
        a = np.floor(a * 65536.0)
    else:
        a = a * 1000.0 - 300.0
    a = a.astype(dtype)
    return a if channels == 3 else a[:, :, 0]


def objects(viewdir=VIEWDIRS[0], ascending_y=False, descending_x=False, **camera):
    """(Camera, Raster) of the agreement scene; `ascending_y`: the same DEM stored bottom row first; `descending_x`:
    stored last column first; `camera`: further arguments of `camera_arguments`."""
    from glimpse_amd import Camera, Raster

    x, y, z = dem_arrays()
    if ascending_y:
        y, z = y[::-1].copy(), z[::-1].copy()
    if descending_x:
        x, z = x[::-1].copy(), z[:, ::-1].copy()
    return Camera(**camera_arguments(viewdir, **camera)), Raster(z, x=x, y=y)


def image(array, cam, day=0):
    from glimpse_amd import Image

    return Image(cam=cam, array=array, datetime=T0 + datetime.timedelta(days=day))
