"""`Raster.horizon` (raster.py:1391-1463) restated in NumPy, the cases of tests/golden/g31_horizon.npz, and the device
kernel's index arithmetic transcribed into Python.  Nothing here imports glimpse_amd.

The restatement is the reference's method with two changes.  Each line is not walked: cell k of helpers.bresenham_line
(helpers.py:1139-1180) is computed in closed form (`line_of` / `line_cells`; `bresenham_loop` is the loop itself, kept to
hold the closed form to).  And the end cell of every ray is clamped into the grid -- the reference's snap_xy(inbounds=
True) repairs only exact hits on the far edges, so an exit that lies a rounding error outside the box becomes row or
column -1 or `size` and the reference raises.  Where the reference computes a heading the clamp changes nothing, and the
arithmetic is the same operations in the same order: equal bit for bit.

The DEMs are the seeded exact terrain of tests/viewshed_terrain.py; the masts are lower than the viewshed cases' so that
the horizon lies inside the DEM for a good share of the headings.
"""
import numpy as np

from tests import viewshed_terrain as vt

# name -> how the case is built (the fields of viewshed_terrain.CASES, plus `headings`).  origin "cell": inside the
# middle cell of a 3 x 3 raster, off its centre.
CASES = {
    "base": dict(shape=(300, 300), d=10.0, x="asc", y="asc", origin="summit", mast=2.0, headings="degrees"),
    "reversed": dict(shape=(300, 300), d=10.0, x="desc", y="desc", origin="centre", mast=2.0, headings="quarters"),
    "long_lines": dict(shape=(700, 1000), d=10.0, x="asc", y="desc", origin="summit", mast=2.0, headings="shuffled"),
    "holes": dict(shape=(512, 512), d=10.0, x="asc", y="desc", origin="summit", mast=2.0, holes=True, headings="degrees"),
    "correction_true": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=2.0, correction=True,
                            headings="degrees"),
    "correction_dict": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=2.0,
                            correction={"radius": 3.0e6, "refraction": 0.2}, headings="degrees"),
    "float32_tuple": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=2.3, dtype="float32",
                          correction=True, origin_type="tuple", headings="degrees"),
    "float32_ndarray": dict(shape=(400, 400), d=500.0, x="asc", y="desc", origin="summit", mast=2.3, dtype="float32",
                            origin_type="ndarray", headings="degrees"),
    "int16": dict(shape=(400, 400), d=10.0, x="asc", y="desc", origin="summit", mast=2.5, dtype="int16",
                  headings="degrees"),
    "one_by_n": dict(shape=(1, 200), d=10.0, x="asc", y="desc", origin="row", mast=3.0, headings="degrees"),
    "three_by_three": dict(shape=(3, 3), d=10.0, x="asc", y="desc", origin="cell", mast=1.0, headings="degrees"),
    "one_by_one": dict(shape=(1, 1), d=10.0, x="asc", y="desc", origin="under", mast=5.0, headings="degrees"),
}
# Rasters too small to hold a horizon: a 1 x 1 raster has no line at all, and in a 3 x 3 one every line has one cell after
# the start, which is its last (never a horizon point).  The fixture's "two runs" rule cannot hold for them; everything
# else is asked of them.
RUNS_EXEMPT = ("three_by_three", "one_by_one")


def headings_of(kind):
    if kind == "degrees":
        return range(360)
    if kind == "quarters":
        return np.arange(0, 360, 0.25)
    # unsorted, with repeats, and the four headings along the axes
    rng = np.random.default_rng(31)
    h = np.concatenate(([0.0, 90.0, 180.0, 270.0], rng.integers(0, 1440, size=236) * 0.25, [90.0, 33.25, 33.25]))
    rng.shuffle(h)
    return h


def build(name, seed):
    """(array, xlim, ylim, origin, correction, headings) of a case."""
    c = CASES[name]
    ny, nx = c["shape"]
    d = c["d"]
    z = vt.terrain((ny, nx), seed)
    xlim = (0.0, nx * d) if c["x"] == "asc" else (nx * d, 0.0)
    ylim = (0.0, ny * d) if c["y"] == "asc" else (ny * d, 0.0)
    x, y = vt.centres(xlim, nx), vt.centres(ylim, ny)
    kind = c["origin"]
    if kind in ("summit", "centre"):
        r, col = vt.summit(z, xlim, ylim)
        off = (0.0, 0.0) if kind == "centre" else (0.3 * d, 0.2 * d)
        origin = (float(x[col] + off[0]), float(y[r] + off[1]), float(z[r, col] + c["mast"]))
    elif kind == "row":
        col = int(np.argmax(z[0]))
        origin = (float(x[col] + 0.3 * d), float(y[0] + 0.1 * d), float(z[0, col] + c["mast"]))
    elif kind == "cell":
        origin = (float(x[1] + 0.2 * d), float(y[1] - 0.1 * d), float(z[1, 1] + c["mast"]))
    else:  # "under"
        origin = (float(x[0] + 0.2 * d), float(y[0] - 0.1 * d), float(z[0, 0] + c["mast"]))
    if c.get("holes"):
        r, col = vt.summit(z, xlim, ylim)
        # scattered cells (missing cells inside lines, lines that end in missing cells), and a block from the origin's own
        # column eastwards that reaches the DEM's north edge: a line that leaves through the block's north side is missing
        # from start to end
        z = vt.holes(z, seed + 1, 0.02, (0, r + 1, col, col + 40))
    dtype = c.get("dtype", "float64")
    if dtype == "int16":
        z = np.floor(z).astype(np.int16)
    elif dtype == "float32":
        z = z.astype(np.float32)  # (multiples of 2^-14 below 2^11: exact)
    if c.get("origin_type") == "ndarray":
        origin = np.array(origin)
    return z, xlim, ylim, origin, c.get("correction", False), headings_of(c["headings"])


# ---- helpers.bresenham_line ----------------------------------------------------------------------------------------
def bresenham_loop(start, end):
    """helpers.bresenham_line (helpers.py:1139-1180) as it is written: the points (x, y) from `start` to `end`."""
    x1, y1 = (int(v) for v in start)
    x2, y2 = (int(v) for v in end)
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    swapped = x1 > x2
    if swapped:
        x1, x2, y1, y2 = x2, x1, y2, y1
    dx, ady = x2 - x1, abs(y2 - y1)
    error = int(dx / 2)
    ystep = 1 if y1 < y2 else -1
    y, points = y1, []
    for x in range(x1, x2 + 1):
        points.append((y, x) if steep else (x, y))
        error -= ady
        if error < 0:
            y += ystep
            error += dx
    if swapped:
        points.reverse()
    return np.array(points)


def line_of(start, end):
    """The constants of a line: (x1, y1, dx, ady, e0, ystep, steep, swapped).  It has dx + 1 points.

    The loop keeps 0 <= error < dx after every step (it starts at dx // 2 < dx, loses ady <= dx and gains dx back when
    it falls below 0), and after j steps error = e0 - j ady + s dx with s the number of y steps taken so far: s is the
    smallest count that keeps that sum >= 0, max(0, ceil((j ady - e0) / dx)).  dx = 0 leaves ady = 0: one point."""
    x1, y1 = (int(v) for v in start)
    x2, y2 = (int(v) for v in end)
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    swapped = x1 > x2
    if swapped:
        x1, x2, y1, y2 = x2, x1, y2, y1
    dx, ady = x2 - x1, abs(y2 - y1)
    return x1, y1, dx, ady, dx // 2, (1 if y1 < y2 else -1), steep, swapped


def line_cells(line, k):
    """Points k (an integer array, 0 = the start) of the line, (x, y) columns, without walking."""
    x1, y1, dx, ady, e0, ystep, steep, swapped = line
    k = np.asarray(k, dtype=np.int64)
    j = dx - k if swapped else k
    num = j * ady - e0
    s = np.where(num > 0, (num + dx - 1) // max(dx, 1), 0)
    x, y = x1 + j, y1 + ystep * s
    return np.column_stack((y, x) if steep else (x, y))


# ---- Raster.horizon -------------------------------------------------------------------------------------------------
def grid_of(shape, xlim, ylim):
    size = np.array((shape[1], shape[0]))
    xlim, ylim = np.asarray(xlim, dtype=float), np.asarray(ylim, dtype=float)
    d = np.hstack((np.diff(xlim), np.diff(ylim))) / size  # Grid.d (raster.py:115-118)
    return size, xlim, ylim, d


def snapped_colrow(xy, xlim, ylim, d):
    """Grid.xy_to_rowcol(xy, snap=True) (raster.py:478-500 with snap_xy, :343-388), as (col, row)."""
    corner = np.append(xlim[0], ylim[0])
    nxy = (xy - corner) / d
    nxy -= 0.5
    nxy = np.floor(nxy + 0.5)
    nxy[xy == np.append(xlim[1], ylim[1])] -= 1  # exact hits on the far edges stay in bounds
    nxy += 0.5
    snapped = nxy * d + corner
    return ((snapped - corner) / d - 0.5).astype(int)


def exits(origin, headings, xlim, ylim):
    """Where the rays leave the raster's box (raster.py:1418-1423; helpers.intersect_rays_box, helpers.py:955-1001, in
    two dimensions).  Only the exits are used: the origin is inside."""
    headings = np.array(headings, dtype=float)
    thetas = -(headings - 90) * (np.pi / 180)
    directions = np.column_stack((np.cos(thetas), np.sin(thetas)))
    lo, hi = (min(xlim), min(ylim)), (max(xlim), max(ylim))
    with np.errstate(divide="ignore", invalid="ignore"):
        invdir = 1 / directions
        neg = invdir < 0
        tmin = (np.where(neg[:, 0], hi[0], lo[0]) - origin[0]) * invdir[:, 0]
        tmax = (np.where(neg[:, 0], lo[0], hi[0]) - origin[0]) * invdir[:, 0]
        tymin = (np.where(neg[:, 1], hi[1], lo[1]) - origin[1]) * invdir[:, 1]
        tymax = (np.where(neg[:, 1], lo[1], hi[1]) - origin[1]) * invdir[:, 1]
        misses = (tmin > tymax) | (tymin > tmax)
        tmax[misses] = np.nan
        closer = tymax < tmax
        tmax[closer] = tymax[closer]
        tmax[tmax < 0] = np.nan
    return np.asarray(origin[0:2], dtype=float) + tmax[:, None] * directions


def rays(shape, xlim, ylim, origin, headings):
    """(start (col, row), ends (n, 2) as (col, row) clamped into the grid, ends before the clamp)."""
    size, xlim, ylim, d = grid_of(shape, xlim, ylim)
    start = snapped_colrow(np.atleast_2d(np.asarray(origin[0:2], dtype=float)), xlim, ylim, d)[0]
    raw = snapped_colrow(exits(origin, headings, xlim, ylim), xlim, ylim, d)
    ends = np.column_stack((np.clip(raw[:, 0], 0, size[0] - 1), np.clip(raw[:, 1], 0, size[1] - 1)))
    return start, ends, raw


def ratios(array, xlim, ylim, d, origin, correction, rowcol):
    """(dz, elevation ratio) of the cells `rowcol` (raster.py:1444-1454), in the reference's dtypes."""
    dz = array[rowcol[:, 0], rowcol[:, 1]] - origin[2]
    xy = (rowcol + 0.5)[:, ::-1] * d + np.array((xlim[0], ylim[0]))
    dxy = np.sum((xy - origin[0:2]) ** 2, axis=1)
    if correction is True:
        correction = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        if isinstance(correction, dict):
            radius, refraction = correction.get("radius", 6.3781e6), correction.get("refraction", 0.13)
            delta = (refraction - 1) * dxy / (2 * radius)
            return dz, (dz + delta) / np.sqrt(dxy)
        return dz, dz / np.sqrt(dxy)


def choose(dz, ratio):
    """Index of the horizon cell among a line's cells, or -1 (raster.py:1445-1456)."""
    missing = np.isnan(dz)
    if np.all(missing):
        return -1
    best = int(np.nanargmax(ratio))
    return best if np.any(~missing[best + 1:]) else -1


def horizon(array, xlim, ylim, origin, headings, correction=False):
    """(hxyz (n, 3) with NaN rows where a heading has no horizon point, cell (n, 2) (row, col) or -1)."""
    array = np.asarray(array)
    size, xlim, ylim, d = grid_of(array.shape, xlim, ylim)
    n = len(headings)
    hxyz, cell = np.full((n, 3), np.nan), np.full((n, 2), -1)
    if n == 0:
        return hxyz, cell
    start, ends, _ = rays(array.shape, xlim, ylim, origin, headings)
    for i in range(n):
        line = line_of(start, ends[i])
        rowcol = line_cells(line, np.arange(1, line[2] + 1))[:, ::-1]  # (the start cell is skipped)
        dz, ratio = ratios(array, xlim, ylim, d, origin, correction, rowcol)
        best = choose(dz, ratio)
        if best >= 0:
            cell[i] = rowcol[best]
            hxyz[i, 0:2] = (rowcol[best] + 0.5)[::-1] * d + np.array((xlim[0], ylim[0]))
            hxyz[i, 2] = dz[best]
    hxyz[:, 2] += origin[2]
    return hxyz, cell


def runs(hxyz):
    """helpers.boolean_split(hxyz, mask, axis=0, circular=True)[mask[0]::2] (helpers.py:799-803): the unbroken runs of
    rows that are not NaN, the last joined to the first when both ends have a point."""
    mask = np.isnan(hxyz[:, 0])
    if len(mask) == 0:
        return []
    cuts = np.nonzero(mask[1:] != mask[:-1])[0] + 1
    splits = np.split(hxyz, cuts, axis=0)
    if len(splits) > 1 and mask[0] == mask[-1]:
        splits[0] = np.concatenate((splits[-1], splits[0]), axis=0)
        splits.pop(-1)
    return splits[int(mask[0])::2]


# ---- the kernel's index arithmetic (glimpse_amd/csrc/glh_horizon.hip: k_horizon) -------------------------------------
WAVE = 64
SHORT_LINE = 256  # lines of at most this many cells: one wave per line; longer ones: four


def workgroup_of(longest):
    return WAVE if longest <= SHORT_LINE else 4 * WAVE


def better(ra, ka, rb, kb):
    """Whether candidate a = (ratio, k) beats b: the greater ratio, the lower k among equals.  k < 0: no candidate."""
    if ka < 0:
        return False
    return kb < 0 or ra > rb or (ra == rb and ka < kb)


def kernel_line(dz, ratio, tb):
    """One workgroup of `tb` lanes on one line whose cells k = 1 .. dx have the values dz[k - 1], ratio[k - 1] (the cells
    themselves: line_cells(line, k), the closed form the kernel uses): lane t visits k = 1 + t, 1 + t + tb, ... <= dx,
    keeps its best (ratio, k) and its last non-missing k; the lanes of a wave are combined by a butterfly (xor 32, 16,
    ... 1), the waves in order by lane 0.  Returns the chosen k or -1."""
    dx = len(dz)
    missing = np.isnan(dz)
    lanes = []
    for t in range(tb):
        br, bk, last = 0.0, -1, -1
        for k in range(1 + t, dx + 1, tb):
            if missing[k - 1]:
                continue
            if better(ratio[k - 1], k, br, bk):
                br, bk = ratio[k - 1], k
            last = k
        lanes.append((br, bk, last))
    waves = []
    for w in range(tb // WAVE):
        lane = lanes[w * WAVE:(w + 1) * WAVE]
        step = WAVE // 2
        while step:
            new = []
            for t in range(WAVE):
                (ra, ka, la), (rb, kb, lb) = lane[t], lane[t ^ step]
                new.append(((rb, kb) if better(rb, kb, ra, ka) else (ra, ka)) + (max(la, lb),))
            lane = new
            step //= 2
        waves.append(lane[0])
    br, bk, last = waves[0]
    for rb, kb, lb in waves[1:]:
        if better(rb, kb, br, bk):
            br, bk = rb, kb
        last = max(last, lb)
    return bk if bk >= 0 and last > bk else -1
