"""`Raster.gradient`, `Raster.hillshade` (raster.py:1465-1474, :1249-1264) and `helpers.polygons_to_mask`
(helpers.py:1701-1768) restated in NumPy, operation by operation in the order the kernels of glh_terrain.hip take, and the
cases of tests/golden/g33_terrain.npz.

  gradient   along a line with spacing h: (f[i+1] - f[i-1]) / (2 h) inside, (f[1] - f[0]) / h and (f[-1] - f[-2]) / h at the
             ends; the difference in the array's dtype, the quotient in float64, rounded to the array's dtype.
  hillshade  gradients of vert_exag * array with dy negated; the normal (-e_dx, -e_dy, 1) over sqrt((n0^2 + n1^2) + n2^2);
             the intensity n0 l0 + n1 l1 + n2 l2 summed left to right (matplotlib hands this one product to BLAS, the only
             place where the two can differ); imin, imax (NaN with any NaN cell); I *= fraction; if imax - imin > 1e-6,
             I = (I - imin) / (imax - imin); clip to [0, 1].
  polygons   per ring even-odd on the cell centres (c + 0.5, r + 0.5): an edge with y1 != y2 crosses row r when
             min(y1, y2) <= r + 0.5 < max(y1, y2), at x = x1 + (cy - y1) * (x2 - x1) / (y2 - y1), and toggles every cell of
             the row with c + 0.5 > x.  Polygons are a union; the holes are then cleared.
The DEMs are not stored in the golden file: `build` remakes them from the seed (exact terrain of tests/viewshed_terrain.py),
and the file holds their SHA-256.
"""
import numpy as np

from tests import viewshed_terrain as vt

EPS = 2.0 ** -52
TILE = (16, 64)  # rows, columns of one stencil tile of glh_terrain.hip


# ---- gradient and hillshade ---------------------------------------------------------------------------------------------
def gradient_1d(f, h, axis):
    """np.gradient along one axis with the scalar float64 spacing `h`, spelled out."""
    f = np.moveaxis(f, axis, 0)
    h = np.float64(h)
    out = np.empty(f.shape, dtype=f.dtype)
    out[1:-1] = ((f[2:] - f[:-2]).astype(np.float64) / (2.0 * h)).astype(f.dtype)
    out[0] = ((f[1] - f[0]).astype(np.float64) / h).astype(f.dtype)
    out[-1] = ((f[-1] - f[-2]).astype(np.float64) / h).astype(f.dtype)
    return np.moveaxis(out, 0, axis)


def one_nan(a):
    """Every NaN becomes np.nan, the quiet positive one, as the kernels write it (which NaN an operation returns -- its sign
    and payload -- is the processor's; NumPy on x86 hands on the positive NaN that a DEM holds)."""
    a[np.isnan(a)] = np.nan
    return a


def widened(z):
    """Integers and bool become float64, as np.gradient makes them."""
    z = np.asarray(z)
    return z.astype(np.float64) if z.dtype.kind in "biu" else z


def gradient(z, d):
    """(dzdx, dzdy) of Raster.gradient for the signed cell sizes d = (dx, dy)."""
    z = widened(z)
    with np.errstate(invalid="ignore"):
        return one_nan(gradient_1d(z, d[0], 1)), one_nan(gradient_1d(z, d[1], 0))


def light_direction(azimuth, altitude):
    az, alt = np.radians(90 - azimuth), np.radians(altitude)
    return np.array([np.cos(az) * np.cos(alt), np.sin(az) * np.cos(alt), np.sin(alt)])


def raw_intensity(z, d, azimuth=315, altitude=45, vert_exag=1):
    """The intensity before the contrast stretch, float64."""
    z = widened(z)
    scaled = z.dtype.type(float(vert_exag)) * z  # (a Python number times an array: the product in the array's dtype)
    light = light_direction(azimuth, altitude)
    with np.errstate(invalid="ignore"):
        e_dx, e_dy = gradient_1d(scaled, d[0], 1), gradient_1d(scaled, -d[1], 0)
        n0, n1 = (-e_dx).astype(np.float64), (-e_dy).astype(np.float64)
        magnitude = np.sqrt((n0 * n0 + n1 * n1) + 1.0)
        return ((n0 / magnitude) * light[0] + (n1 / magnitude) * light[1]) + (1.0 / magnitude) * light[2]


def stretch(raw, fraction=1.0):
    """(intensity, imin, imax): matplotlib's shade_normals after the dot product."""
    with np.errstate(invalid="ignore"):
        imin, imax = raw.min(), raw.max()
        intensity = raw * float(fraction)
        if imax - imin > 1e-6:
            intensity = (intensity - imin) / (imax - imin)
        return one_nan(np.clip(intensity, 0, 1)), imin, imax


def hillshade(z, d, azimuth=315, altitude=45, vert_exag=1, fraction=1.0):
    return stretch(raw_intensity(z, d, azimuth, altitude, vert_exag), fraction)[0]


def hillshade_bound(imin, imax):
    """|restatement - matplotlib| <= 8 eps / min(1, imax - imin): three roundings per raw intensity (the three-term dot
    product is the one place the two differ), entering at the value and at both ends of the normalisation.  Where nothing
    is normalised (a range of at most 1e-6, or NaN) the divisor is 1."""
    spread = imax - imin
    return 8 * EPS / min(1.0, spread) if spread > 1e-6 else 8 * EPS


# what a variant changes of the default case: cells of 10 x 10, x ascending, y descending, float64, the default light
VARIANTS = {
    "default": {},
    "x_desc": dict(x="desc"),
    "y_asc": dict(y="asc"),
    "x_desc_y_asc": dict(x="desc", y="asc"),
    "nonsquare": dict(d=(12.5, 7.0)),
    "nonsquare_y_asc": dict(d=(3.0, 20.0), y="asc"),
    "float32": dict(dtype="float32"),
    "float32_x_desc": dict(dtype="float32", x="desc", d=(7.0, 7.0)),
    "float32_exag": dict(dtype="float32", vert_exag=0.1),
    "int16": dict(dtype="int16"),
    "nan_interior": dict(nan="interior"),
    "nan_corner": dict(nan="corner"),
    "constant": dict(constant=True),
    "vert_exag_0p1": dict(vert_exag=0.1),
    "vert_exag_10": dict(vert_exag=10),
    "fraction_1p5": dict(fraction=1.5),
    "light_135_30": dict(azimuth=135, altitude=30),
    "light_0_90": dict(azimuth=0, altitude=90),
    "light_200_10": dict(azimuth=200, altitude=10),
    "light_90_60": dict(azimuth=90, altitude=60),
}
SMALL = (7, 13)
EDGE_SHAPES = ((2, 2), (2, 67), (67, 2), (3, 3))
TILED = (2 * TILE[0] + 1, 2 * TILE[1] + 1)  # one more than two tiles each way


def case_name(variant, shape):
    return f"{variant}@{shape[0]}x{shape[1]}"


# the cases the golden file holds: every variant on a small raster, the default on the shapes where a line has two or three
# cells, and the default on the tiled shape
GOLDEN_CASES = ([case_name(v, SMALL) for v in VARIANTS] + [case_name("default", s) for s in EDGE_SHAPES]
                + [case_name("default", TILED)])
# the device also runs every variant on the tiled shape, against the restatement
TILED_CASES = [case_name(v, TILED) for v in VARIANTS if v != "default"]


def build(name):
    """(z, xlim, ylim, kwargs of hillshade) of a case; the seed is a function of the name's place in the tables."""
    variant, shape = name.split("@")
    ny, nx = (int(v) for v in shape.split("x"))
    c = VARIANTS[variant]
    seed = 3300 + 7 * list(VARIANTS).index(variant) + ny + nx
    z = vt.terrain((ny, nx), seed)
    if c.get("constant"):
        z = np.full((ny, nx), 321.5)
    if c.get("nan") == "interior":
        z[ny // 2, nx // 2 + 1] = np.nan
    elif c.get("nan") == "corner":
        z[ny - 1, 0] = np.nan
    dtype = c.get("dtype", "float64")
    if dtype == "int16":
        z = np.floor(z).astype(np.int16)
    elif dtype == "float32":
        z = (z + 0.3).astype(np.float32)  # (rounded: the float32 differences below are not all exact)
    dx, dy = c.get("d", (10.0, 10.0))
    xlim = (500.0, 500.0 + nx * dx) if c.get("x", "asc") == "asc" else (500.0 + nx * dx, 500.0)
    ylim = (-200.0, -200.0 + ny * dy) if c.get("y", "desc") == "asc" else (-200.0 + ny * dy, -200.0)
    kwargs = {k: c[k] for k in ("azimuth", "altitude", "vert_exag", "fraction") if k in c}
    return z, xlim, ylim, kwargs


def cell_sizes(z, xlim, ylim):
    """Grid.d: the signed cell sizes."""
    return np.hstack((np.diff(xlim), np.diff(ylim))) / np.array(z.shape[::-1])


# ---- polygons -----------------------------------------------------------------------------------------------------------
def ring_parity(ring, size):
    """bool (ny, nx): the cells whose centre an odd number of the ring's edges has toggled."""
    nx, ny = size
    ring = np.asarray(ring, dtype=np.float64)
    cy, cx = np.arange(ny) + 0.5, np.arange(nx) + 0.5
    parity = np.zeros((ny, nx), dtype=bool)
    for (x1, y1), (x2, y2) in zip(ring, np.roll(ring, -1, axis=0)):
        if y1 == y2:
            continue
        rows = np.nonzero((min(y1, y2) <= cy) & (cy < max(y1, y2)))[0]
        with np.errstate(all="ignore"):
            x = x1 + (cy[rows] - y1) * (x2 - x1) / (y2 - y1)
        parity[rows] ^= cx[None, :] > x[:, None]
    return parity


def polygons_to_mask(polygons, size, holes=None):
    nx, ny = size
    mask = np.zeros((ny, nx), dtype=bool)
    for ring in polygons:
        mask |= ring_parity(ring, size)
    for ring in holes or ():
        mask &= ~ring_parity(ring, size)
    return mask


def star(rng, centre, r_lo, r_hi, n):
    """A star-shaped simple polygon (n, 2): ascending angles around `centre`, radii in [r_lo, r_hi)."""
    angles = np.sort(rng.uniform(0.0, 2 * np.pi, n))
    radii = rng.uniform(r_lo, r_hi, n)
    return np.column_stack((centre[0] + radii * np.cos(angles), centre[1] + radii * np.sin(angles)))


def star_scene(seed, size, n_polygons, with_holes=True):
    """(polygons, holes): stars scattered over (and beyond) a grid of `size` = (nx, ny), each hole a smaller star around
    the centre of a polygon."""
    rng = np.random.default_rng(seed)
    nx, ny = size
    polygons, holes = [], []
    for _ in range(n_polygons):
        centre = rng.uniform((-0.1 * nx, -0.1 * ny), (1.1 * nx, 1.1 * ny))
        reach = rng.uniform(1.5, 0.3 * min(nx, ny) + 2.0)
        polygons.append(star(rng, centre, 0.5 * reach, reach, int(rng.integers(3, 12))))
        if with_holes and rng.random() < 0.5:
            holes.append(star(rng, centre, 0.15 * reach, 0.4 * reach, int(rng.integers(3, 8))))
    return polygons, holes


def distance_to_edges(rings, size):
    """The smallest distance from a cell centre to an edge of any ring."""
    nx, ny = size
    p = np.column_stack([g.ravel() for g in np.meshgrid(np.arange(nx) + 0.5, np.arange(ny) + 0.5)])
    best = np.inf
    for ring in rings:
        a, b = np.asarray(ring, dtype=float), np.roll(np.asarray(ring, dtype=float), -1, axis=0)
        ab = b - a
        t = np.clip(((p[:, None, :] - a[None]) * ab[None]).sum(-1) / (ab * ab).sum(-1)[None], 0.0, 1.0)
        nearest = a[None] + t[..., None] * ab[None]
        best = min(best, float(np.sqrt(((p[:, None, :] - nearest) ** 2).sum(-1)).min()))
    return best


# the two examples of the reference's docstrings (raster.py:1136-1141 through a 3 x 3 raster of unit cells, helpers.py:1717-1727)
DOCTEST_RASTER = dict(polygons=[[(0.1, 0.1), (1.9, 0.1), (1.9, 1.9), (0.1, 1.9)]],
                      want=np.array([[1, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=bool))
DOCTEST_HELPER = dict(polygons=[[(1, 1), (4, 1), (4, 4), (1, 4)], [(0, 0), (0.6, 0), (0.6, 0.6), (0, 0.6)]],
                      holes=[[(2, 2), (3, 2), (3, 3), (2, 3)]], size=(5, 5),
                      want=np.array([[1, 0, 0, 0, 0], [0, 1, 1, 1, 0], [0, 1, 0, 1, 0], [0, 1, 1, 1, 0], [0, 0, 0, 0, 0]],
                                    dtype=bool))
# the boundary rule, by hand: name -> (polygons, size (nx, ny), the mask the rule gives)
BOUNDARY = {
    # the right vertex lies on the centre line of row 1: of the two edges that meet there only the one that goes on downwards
    # (lo <= cy) counts, so the row is crossed twice and filled between the crossings at x = 0.2 and x = 3.7
    "vertex_on_a_centre_line": ([[(0.2, 0.2), (3.7, 1.5), (0.2, 2.8)]], (5, 3),
                                np.array([[1, 0, 0, 0, 0], [1, 1, 1, 1, 0], [1, 0, 0, 0, 0]], dtype=bool)),
    # vertical edges through the centres of columns 1 and 3: c + 0.5 > x is false on the edge, so the centre on the left
    # edge is out and the one on the right edge is in
    "edge_through_a_centre": ([[(1.5, 0.2), (3.5, 0.2), (3.5, 1.8), (1.5, 1.8)]], (5, 2),
                              np.array([[0, 0, 1, 1, 0], [0, 0, 1, 1, 0]], dtype=bool)),
    # horizontal edges on the centre lines of rows 1 and 3 count for nothing; the vertical edges span 1.5 <= cy < 3.5, so
    # the row on the top edge is in and the row on the bottom edge is out
    "horizontal_edge_on_a_centre_line": ([[(0.2, 1.5), (2.8, 1.5), (2.8, 3.5), (0.2, 3.5)]], (3, 5),
                                         np.array([[0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0], [0, 0, 0]], dtype=bool)),
}


# ---- the host-only companions: the cases of the golden file -----------------------------------------------------------------
# fill_circle on a raster of 12 x 15 cells of 10 x 10: (xlim, ylim, centre, radius)
CIRCLE_X, CIRCLE_Y_DESC, CIRCLE_Y_ASC = (0.0, 150.0), (120.0, 0.0), (0.0, 120.0)
CIRCLES = {
    "inside_r0": (CIRCLE_X, CIRCLE_Y_DESC, (72.0, 63.0), 4.0),
    "inside_r1": (CIRCLE_X, CIRCLE_Y_DESC, (72.0, 63.0), 10.0),
    "inside_r2": (CIRCLE_X, CIRCLE_Y_DESC, (72.0, 63.0), 20.0),
    "inside_r7": (CIRCLE_X, CIRCLE_Y_DESC, (72.0, 63.0), 70.0),
    "edge_cell_r2": (CIRCLE_X, CIRCLE_Y_DESC, (3.0, 117.0), 20.0),
    "edge_cell_r0": (CIRCLE_X, CIRCLE_Y_DESC, (149.0, 2.0), 3.0),
    "outside_r7": (CIRCLE_X, CIRCLE_Y_DESC, (-25.0, 60.0), 70.0),
    "outside_r2_misses": (CIRCLE_X, CIRCLE_Y_DESC, (-55.0, 60.0), 20.0),
    "y_ascending_r2": (CIRCLE_X, CIRCLE_Y_ASC, (72.0, 63.0), 20.0),
    "y_ascending_r7": (CIRCLE_X, CIRCLE_Y_ASC, (140.0, 10.0), 70.0),
}
CIRCLE_SHAPE = (12, 15)
CIRCLE_X_DESC = (150.0, 0.0)  # d[0] < 0: the radius in cells is negative, which raises


def rasterize_case(dtype):
    """(array, xlim, ylim, xy, values): repeated cells, a point on each outer edge, a point outside; NaN values for a
    floating array."""
    array = (np.arange(30.0).reshape(5, 6) * 3 - 11).astype(dtype)
    xlim, ylim = (100.0, 160.0), (50.0, 0.0)
    xy = np.array([[105.0, 45.0], [106.0, 44.0], [109.5, 41.0],   # three points in cell (0, 0)
                   [125.0, 25.0], [125.0, 25.0],                  # a repeated point
                   [100.0, 33.0], [160.0, 33.0], [131.0, 50.0], [131.0, 0.0],  # one on each outer edge
                   [160.0, 0.0],                                  # the far corner
                   [120.0, 20.0],                                 # on an inner cell corner: the higher cells
                   [99.0, 25.0], [130.0, 51.0], [400.0, -3.0],    # outside
                   [155.0, 45.0], [156.0, 46.0], [143.0, 12.0]])
    values = np.array([1.0, 2.0, 4.5, -3.0, 8.0, 10.0, 20.0, 30.0, 40.0, 50.0, 60.0, 7e9, 8e9, 9e9, 0.1, 0.2, 5.0])
    if np.dtype(dtype).kind == "f":
        values[[14, 15]] = np.nan  # a cell whose mean is NaN
    return array, xlim, ylim, xy, values


def holey(shape=(9, 11)):
    """A raster with NaN borders of different widths, a NaN inside, and its limits (y descending)."""
    z = vt.terrain(shape, 3391)
    z[:2] = np.nan
    z[-1:] = np.nan
    z[:, :3] = np.nan
    z[:, -2:] = np.nan
    z[4, 5] = np.nan
    return z, (1000.0, 1000.0 + 5.0 * shape[1]), (2000.0 + 4.0 * shape[0], 2000.0)
