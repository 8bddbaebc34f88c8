"""Seeded terrain for the viewshed tests, exact on every machine, and the cases of tests/golden/g28_viewshed.npz.

The DEMs are not stored in the golden file: they are rebuilt here.  A DEM is a sum of integer lattices
(`np.random.default_rng(seed).integers`), each upsampled bilinearly by a power of two and weighted by a power of two, so
every intermediate is a dyadic rational far inside float64's 53 bits: no rounding happens anywhere, and the array is the
same bytes wherever it is built (the golden file keeps a SHA-256 of each to prove it).  No FFT, no normal deviates.
Exactly planar or constant DEMs are not test inputs: every visibility comparison on them is a tie.
"""
import hashlib

import numpy as np

OCTAVES = 8  # lattice spacings 128, 64, ..., 1 cells


def _upsample(lattice, factor, ny, nx):
    """Bilinear upsampling by `factor` (a power of two): weights k / factor are exact, so are the products and sums."""
    i, j = np.arange(ny), np.arange(nx)
    i0, j0 = i // factor, j // factor
    ti, tj = (i % factor) / factor, (j % factor) / factor
    a, b = lattice[i0][:, j0], lattice[i0][:, j0 + 1]
    c, d = lattice[i0 + 1][:, j0], lattice[i0 + 1][:, j0 + 1]
    top = a * (1 - tj)[None, :] + b * tj[None, :]
    bottom = c * (1 - tj)[None, :] + d * tj[None, :]
    return top * (1 - ti)[:, None] + bottom * ti[:, None]


def terrain(shape, seed, amplitude=512):
    """float64 (ny, nx): a fractal surface, octave of spacing s cells weighted s / 128; values are multiples of 2^-14."""
    ny, nx = shape
    rng = np.random.default_rng(seed)
    z = np.zeros((ny, nx))
    for p in range(OCTAVES - 1, -1, -1):
        factor = 2 ** p
        lattice = rng.integers(-amplitude, amplitude + 1, size=(ny // factor + 2, nx // factor + 2)).astype(np.float64)
        z += _upsample(lattice, factor, ny, nx) * (factor / 2 ** (OCTAVES - 1))
    return z


def holes(z, seed, share=0.02, block=None):
    """NaN in a seeded `share` of the cells and in `block` = (row0, row1, col0, col1)."""
    z = z.copy()
    rng = np.random.default_rng(seed)
    z[rng.random(z.shape) < share] = np.nan
    if block is not None:
        z[block[0]:block[1], block[2]:block[3]] = np.nan
    return z


def sha256(array):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(array).tobytes()).digest(), dtype=np.uint8)


def centres(lim, n):
    """Cell-centre coordinates of an axis with outer limits `lim`, first to last cell (Grid.x / Grid.y)."""
    lo, hi = min(lim), max(lim)
    d = (hi - lo) / n
    value = np.linspace(lo + d / 2, hi - d / 2, n)
    return value[::-1] if lim[1] < lim[0] else value


def summit(z, xlim, ylim, margin=0.25):
    """(row, col) of the highest cell of the DEM's middle part."""
    ny, nx = z.shape
    r0, c0 = int(ny * margin), int(nx * margin)
    mid = z[r0:ny - r0, c0:nx - c0]
    r, c = np.unravel_index(np.nanargmax(mid), mid.shape)
    return r + r0, c + c0


# name -> how the case is built.  shape (ny, nx); cell size d; x / y "asc" or "desc" (which way the coordinate runs along
# the array); origin: "summit" (between cell centres on the summit, with a mast), "centre" (exactly on a cell centre),
# "outside" (west of the DEM), "row" (over a one-row raster), "under" (the 1 x 1 raster under the origin).
CASES = {
    "summit_mast": dict(shape=(1024, 1024), d=10.0, x="asc", y="desc", origin="summit", mast=30.0),
    "cell_centre": dict(shape=(512, 512), d=10.0, x="asc", y="desc", origin="centre", mast=25.0),
    "outside": dict(shape=(400, 600), d=10.0, x="asc", y="desc", origin="outside", mast=400.0),
    "y_ascending": dict(shape=(300, 300), d=10.0, x="asc", y="asc", origin="summit", mast=20.0),
    "x_descending": dict(shape=(300, 300), d=10.0, x="desc", y="desc", origin="summit", mast=20.0),
    "shape_700x1000": dict(shape=(700, 1000), d=10.0, x="asc", y="desc", origin="summit", mast=30.0),
    "nan_holes": dict(shape=(512, 512), d=10.0, x="asc", y="desc", origin="summit", mast=30.0, holes=True),
    "correction_true": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=300.0, correction=True),
    "correction_dict": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=300.0,
                            correction={"radius": 3.0e6, "refraction": 0.2}),
    "float32_tuple": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=300.3, dtype="float32",
                          correction=True, origin_type="tuple"),
    "float32_ndarray": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=300.3, dtype="float32",
                            correction=True, origin_type="ndarray"),
    "int16": dict(shape=(400, 400), d=10.0, x="asc", y="desc", origin="summit", mast=20.5, dtype="int16"),
    "one_by_one": dict(shape=(1, 1), d=10.0, x="asc", y="desc", origin="under", mast=5.0),
    "one_by_n": dict(shape=(1, 200), d=10.0, x="asc", y="desc", origin="row", mast=3.0),
}
# (a 1 x 1 raster has one cell: its visible fraction is 0 or 1 whatever the algorithm does)
FRACTION_EXEMPT = ("one_by_one",)


def build(name, seed):
    """(array, xlim, ylim, origin, correction) of a case.  `origin` is a tuple of Python floats unless the case asks for an
    ndarray (NumPy promotes a float32 DEM differently with the two)."""
    c = CASES[name]
    ny, nx = c["shape"]
    d = c["d"]
    z = terrain((ny, nx), seed)
    xlim = (0.0, nx * d) if c["x"] == "asc" else (nx * d, 0.0)
    ylim = (0.0, ny * d) if c["y"] == "asc" else (ny * d, 0.0)
    x, y = centres(xlim, nx), centres(ylim, ny)
    kind = c["origin"]
    if kind in ("summit", "centre"):
        r, col = summit(z, xlim, ylim)
        off = (0.0, 0.0) if kind == "centre" else (0.3 * d, 0.2 * d)
        origin = (float(x[col] + off[0]), float(y[r] + off[1]), float(z[r, col] + c["mast"]))
    elif kind == "outside":
        r = ny // 2
        origin = (float(min(xlim) - 12.4 * d), float(y[r] + 0.3 * d), float(np.max(z) + c["mast"]))
    elif kind == "row":
        col = int(np.argmax(z[0]))
        origin = (float(x[col] + 0.3 * d), float(y[0] + 0.1 * d), float(z[0, col] + c["mast"]))
    else:  # "under"
        origin = (float(x[0] + 0.2 * d), float(y[0] - 0.1 * d), float(z[0, 0] + c["mast"]))
    if c.get("holes"):
        r, col = summit(z, xlim, ylim)
        # scattered cells, and a block that covers the cells north-east of the origin: part of the first processed ring
        z = holes(z, seed + 1, 0.02, (r - 6, r + 1, col + 1, col + 7))
    dtype = c.get("dtype", "float64")
    if dtype == "int16":
        z = np.floor(z).astype(np.int16)
    elif dtype == "float32":
        z = z.astype(np.float32)  # (multiples of 2^-14 below 2^11: exact)
    if c.get("origin_type") == "ndarray":
        origin = np.array(origin)
    return z, xlim, ylim, origin, c.get("correction", False)
