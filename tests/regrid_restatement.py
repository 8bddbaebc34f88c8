"""A NumPy restatement of exactly what glimpse_amd/csrc/glh_regrid.hip does, and the cases of tests/golden/g32_regrid.npz.

`regrid` is glh_stage_raster_regrid: per axis FITPACK's interpolating knots, the banded collocation matrix and its LU
factors without pivoting, forward and backward substitution down the columns and then along the rows with the same
summation orders as the kernels, the closed form of the first and last coefficient at order 1, the evaluation summed rows
outer, columns inner, and the NaN rule of order 1 (a mask carried beside the values).  Every operation is a separate
float64 NumPy operation, as the kernels' are separate round-to-nearest intrinsics, so the device's result equals this one
in every bit.  `zoom_linear` is glh_stage_zoom_linear, `blend` the cell arithmetic of glh_stage_raster_interpolate.

`sample_grid` is the host logic of Raster.sample(grid=True) around it (bounds, flips, direction, fill), restated apart
from glimpse_amd.raster so that the CPU tests can check the restatement against the reference without a device.

The inputs are not stored in the golden file: `build(name)` rebuilds them from seeds (tests/viewshed_terrain.py's exact
terrain), and the file pins each by SHA-256.
"""
import datetime

import numpy as np

from tests import viewshed_terrain as vt

MAX_K = 5


# ---- per-axis host arithmetic (glh_regrid.hip: regrid_knots, regrid_basis, regrid_factor) -------------------------------
def knots(x, lo, hi, k):
    n = len(x)
    t = np.zeros(n + k + 1)
    t[:k + 1] = lo
    t[n:] = hi
    for m in range(n - k - 1):
        if k % 2:
            t[k + 1 + m] = x[(k + 1) // 2 + m]
        else:
            t[k + 1 + m] = (x[k // 2 + m] + x[k // 2 + m + 1]) / 2
    return t


def basis(t, n, k, x):
    """(l, h [k + 1]): the knot interval of x clamped to the box, and de Boor's recurrence as fpbspl runs it."""
    x = np.float64(min(max(x, t[k]), t[n]))
    l = k + int(np.searchsorted(t[k + 1:n], x, side="right"))
    h = np.zeros(MAX_K + 1)
    hh = np.zeros(MAX_K)
    h[0] = 1.0
    for j in range(1, k + 1):
        hh[:j] = h[:j]
        h[0] = 0.0
        for i in range(j):
            li = l + i + 1
            lj = li - j
            f = hh[i] / (t[li] - t[lj])
            h[i] = h[i] + f * (t[li] - x)
            h[i + 1] = f * (x - t[lj])
    return l, h[:k + 1].copy()


def factor(x, t, k):
    """lu [n][2 k + 1]: the collocation matrix in band storage ((i, j) at [i][j - i + k]), LU without pivoting in place."""
    n, w = len(x), 2 * k + 1
    lu = np.zeros((n, w))
    for i in range(n):
        l, h = basis(t, n, k, x[i])
        for a in range(k + 1):
            d = l - k + a - i + k
            if d < 0 or d >= w:
                assert h[a] == 0.0, "the collocation matrix leaves its band"
                continue
            lu[i, d] = h[a]
    for p in range(n):
        pivot = lu[p, k]
        assert pivot != 0.0
        last = min(p + k, n - 1)
        for i in range(p + 1, last + 1):
            m = lu[i, p - i + k] / pivot
            lu[i, p - i + k] = m
            for j in range(p + 1, last + 1):
                lu[i, j - i + k] = lu[i, j - i + k] - m * lu[p, j - p + k]
    return lu


def solve_lines(w, lu, k):
    """k_solve_cols on w [n][lines] (k_solve_rows is the same along the other axis): in place."""
    n = w.shape[0]
    for i in range(n):
        acc = w[i].copy()
        for d in range(k):
            j = i - k + d
            if j >= 0:
                acc = acc - lu[i, d] * w[j]
        w[i] = acc
    for i in range(n - 1, -1, -1):
        acc = w[i].copy()
        for d in range(k):
            j = i + 1 + d
            if j < n:
                acc = acc - lu[i, k + 1 + d] * w[j]
        w[i] = acc / lu[i, k]
    return w


def ends(w, x, lo, hi):
    """k_ends_cols on w [n][lines], order 1 and n >= 3: the closed form of the first and last coefficient."""
    n = len(x)
    a00 = (x[1] - x[0]) / (x[1] - lo)
    a01 = (x[0] - lo) / (x[1] - lo)
    b0 = (hi - x[n - 1]) / (hi - x[n - 2])
    b1 = (x[n - 1] - x[n - 2]) / (hi - x[n - 2])
    first = (w[0] - a01 * w[1]) / a00
    last = (w[n - 1] - b0 * w[n - 2]) / b1
    w[0], w[n - 1] = first, last
    return w


def coefficients(z, gx, gy, box, kx, ky):
    c = np.array(z, dtype=np.float64)
    xmin, xmax, ymin, ymax = box
    if ky == 1 and len(gy) >= 3:
        ends(c, gy, ymin, ymax)
    else:
        solve_lines(c, factor(gy, knots(gy, ymin, ymax, ky), ky), ky)
    ct = np.ascontiguousarray(c.T)
    if kx == 1 and len(gx) >= 3:
        ends(ct, gx, xmin, xmax)
    else:
        solve_lines(ct, factor(gx, knots(gx, xmin, xmax, kx), kx), kx)
    return np.ascontiguousarray(ct.T)


def _tables(g, lo, hi, k, out):
    t = knots(g, lo, hi, k)
    pairs = [basis(t, len(g), k, v) for v in out]
    return np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs]).reshape(len(out), k + 1)


def _partner(i, n):
    return np.where(i == 0, 1, np.where(i == n - 1, n - 2, i))


def regrid(z, gx, gy, box, kx, ky, xo, yo, nan_mask=None, zmin=None, flip_x=False, flip_y=False):
    """glh_stage_raster_regrid: z (ny, nx) with ascending axes and no NaN (0 under nan_mask); xo, yo ascending."""
    ny, nx = z.shape
    c = coefficients(z, gx, gy, box, kx, ky)
    lx, hx = _tables(gx, box[0], box[1], kx, xo)
    ly, hy = _tables(gy, box[2], box[3], ky, yo)
    acc = np.zeros((len(yo), len(xo)))
    blank = np.zeros(acc.shape, dtype=bool)
    for p in range(ky + 1):
        for q in range(kx + 1):
            r, col = ly - ky + p, lx - kx + q
            acc = acc + c[r][:, col] * (hy[:, p][:, None] * hx[:, q][None, :])
            if nan_mask is not None:
                weight = (hy[:, p] != 0.0)[:, None] & (hx[:, q] != 0.0)[None, :]
                r2, c2 = _partner(r, ny), _partner(col, nx)
                cell = nan_mask[r][:, col] | nan_mask[r][:, c2] | nan_mask[r2][:, col] | nan_mask[r2][:, c2]
                blank |= weight & cell.astype(bool)
    if zmin is not None and not np.isnan(zmin):
        blank |= acc < zmin
    acc[blank] = np.nan
    return acc[::-1 if flip_y else 1, ::-1 if flip_x else 1].copy()


def zoom_linear(a, shape):
    """glh_stage_zoom_linear."""
    a = np.asarray(a, dtype=np.float64)
    ny, nx = a.shape
    my, mx = shape
    sy = np.float64(ny - 1) / np.float64(my - 1) if my > 1 else 0.0
    sx = np.float64(nx - 1) / np.float64(mx - 1) if mx > 1 else 0.0
    cy, cx = np.arange(my, dtype=np.float64) * sy, np.arange(mx, dtype=np.float64) * sx
    i0 = np.minimum(np.floor(cy).astype(np.int64), ny - 1)
    j0 = np.minimum(np.floor(cx).astype(np.int64), nx - 1)
    i1, j1 = np.minimum(i0 + 1, ny - 1), np.minimum(j0 + 1, nx - 1)
    ty, tx = (cy - i0)[:, None], (cx - j0)[None, :]
    uy, ux = 1.0 - ty, 1.0 - tx
    acc = a[i0][:, j0] * (uy * ux)
    acc = acc + a[i0][:, j1] * (uy * tx)
    acc = acc + a[i1][:, j0] * (ty * ux)
    acc = acc + a[i1][:, j1] * (ty * tx)
    return acc


def blend(m0, m1, scale, s0=None, s1=None, scale2=None, ratio=None):
    """k_blend: RasterInterpolant._interpolate's arithmetic (raster.py:1681-1698)."""
    dz = m1 - m0
    z = m0 + dz * scale
    if s0 is None:
        return z, None
    v0, v1 = s0 * s0, s1 * s1
    z_var = v0 + scale2 * (v0 + v1)
    zi = ((1 / 3) * dz) * ratio
    return z, np.sqrt(z_var + zi * zi)


# ---- the host logic of Raster.sample(grid=True) around the kernel -------------------------------------------------------
def centres(lim, n):
    return vt.centres(lim, n)


def sample_grid(z, xlim, ylim, xy, order=1, bounds_error=True, fill_value=np.nan, blank_below_min=True):
    """`blank_below_min=False` leaves out the reference's `samples < min -> NaN` (raster.py:1068): the tests use it to find
    the samples that lie within a rounding error of the raster's minimum, where that test is decided by the last bit."""
    z = np.asarray(z)
    ny, nx = z.shape
    x, y = (np.asarray(v, dtype=float) for v in xy)
    lo = (min(xlim), min(ylim))
    hi = (max(xlim), max(ylim))
    xout, yout = ~((x >= lo[0]) & (x <= hi[0])), ~((y >= lo[1]) & (y <= hi[1]))
    if bounds_error and (xout.any() or yout.any()):
        raise ValueError("Some of the sampling coordinates are out of bounds")
    sx = 1 if xlim[1] > xlim[0] else -1
    sy = 1 if ylim[1] > ylim[0] else -1
    za = np.asarray(z[::sy, ::sx], dtype=np.float64)
    nan = np.isnan(za)
    zmin = float(np.min(za[~nan]))
    mask = nan if nan.any() else None
    za = np.where(nan, 0.0, za)
    xdir = 1 if len(x) < 2 or x[1] > x[0] else -1
    ydir = 1 if len(y) < 2 or y[1] > y[0] else -1
    out = regrid(za, centres(xlim, nx)[::sx], centres(ylim, ny)[::sy], (lo[0], hi[0], lo[1], hi[1]), order, order,
                 x[::xdir], y[::ydir], nan_mask=mask, zmin=zmin if blank_below_min else None, flip_x=xdir < 0, flip_y=ydir < 0)
    if not bounds_error and fill_value is not None:
        out[yout, :] = fill_value
        out[:, xout] = fill_value
    return out


# ---- the cases of g32 ---------------------------------------------------------------------------------------------------
X0, Y0, CELL = 512000.0, 6702000.0, 10.0  # UTM-scale coordinates, 10 m cells
TOLERANCE = {1: 1e-14, 2: 2e-14, 3: 6e-14, 4: 3e-13, 5: 3e-13}  # relative to max |reference result| of the case


def dem(shape, seed, dtype="float64"):
    """Elevations around 1100 m: multiples of 2^-16, exact in float64 (and, rounded once, the float32 case's input)."""
    z = 1100.0 + vt.terrain(shape, seed) * 0.25
    return z.astype(np.float32) if dtype == "float32" else z


def limits(shape, xdesc=False, ydesc=True, x0=X0, y0=Y0, d=CELL):
    ny, nx = shape
    xlim = (x0, x0 + nx * d)
    ylim = (y0, y0 + ny * d)
    return (xlim[::-1] if xdesc else xlim), (ylim[::-1] if ydesc else ylim)


def spread(lim, step, offset):
    lo, hi = min(lim), max(lim)
    return lo + offset + step * np.arange(int(np.floor((hi - lo - offset) / step)) + 1)


def on_grid_lines(lim, n):
    """The limits, every cell centre and every midpoint between centres (the knots of the even orders) of an axis."""
    c = np.sort(centres(lim, n))
    return np.unique(np.concatenate(([min(lim)], c, (c[:-1] + c[1:]) / 2, [max(lim)])))


SAMPLE_CASES = {}
for _k in range(1, 6):
    SAMPLE_CASES[f"small_k{_k}"] = dict(shape=(13, 17), seed=3200 + _k, order=_k)
    SAMPLE_CASES[f"big_k{_k}"] = dict(shape=(70, 130), seed=3210 + _k, order=_k)
    SAMPLE_CASES[f"thin_y_k{_k}"] = dict(shape=(_k + 1, 9), seed=3220 + _k, order=_k)
    SAMPLE_CASES[f"thin_x_k{_k}"] = dict(shape=(11, _k + 1), seed=3230 + _k, order=_k)
SAMPLE_CASES.update({
    "y_ascending_k3": dict(shape=(13, 17), seed=3241, order=3, ydesc=False),
    "x_descending_k2": dict(shape=(13, 17), seed=3242, order=2, xdesc=True),
    "x_descending_k1": dict(shape=(13, 17), seed=3243, order=1, xdesc=True),
    "out_descending_k3": dict(shape=(13, 17), seed=3244, order=3, out="descending"),
    "out_x_descending_k1": dict(shape=(13, 17), seed=3245, order=1, out="x_descending"),
    "out_y_descending_k5": dict(shape=(70, 130), seed=3246, order=5, out="y_descending"),
    "lines_k1": dict(shape=(13, 17), seed=3251, order=1, out="lines"),
    "lines_k2": dict(shape=(13, 17), seed=3252, order=2, out="lines"),
    "lines_k3": dict(shape=(13, 17), seed=3253, order=3, out="lines"),
    "lines_k4": dict(shape=(13, 17), seed=3254, order=4, out="lines"),
    "lines_k5": dict(shape=(13, 17), seed=3255, order=5, out="lines"),
    "fill_k1": dict(shape=(13, 17), seed=3261, order=1, out="beyond", bounds_error=False, fill_value=-9999.0),
    "fill_k3": dict(shape=(13, 17), seed=3262, order=3, out="beyond", bounds_error=False, fill_value=-9999.0),
    "clamped_k1": dict(shape=(13, 17), seed=3263, order=1, out="beyond", bounds_error=False, fill_value=None),
    "clamped_k4": dict(shape=(13, 17), seed=3264, order=4, out="beyond", bounds_error=False, fill_value=None),
    "nan_interior_k1": dict(shape=(13, 17), seed=3271, order=1, out="fine", nan=[(5, 7), (9, 3), (3, 11), (3, 12), (6, 8)]),
    # a NaN in cell 0 of a line.  float64: only along the ascending y axis, and off the neighbouring columns' centres --
    # elsewhere on the rim the reference's float64 stand-in overflows and blanks hundreds of samples.
    # float32: the stand-in is float32's minimum and nothing overflows, so cell 0 of either axis and their corner follow
    # the local rule.  (A NaN in the LAST cell of a line is left out of both: FITPACK's rotations mix the stand-in into
    # the coefficient before it, and the reference returns values of 1e22 beside the blanked cells.)
    "nan_cell0_k1": dict(shape=(13, 17), seed=3272, order=1, out="dense", nan=[(12, 5), (12, 11)]),
    "nan_cell0_float32_k1": dict(shape=(13, 17), seed=3274, order=1, out="fine", dtype="float32",
                                 nan=[(12, 0), (5, 0), (12, 9), (9, 0), (6, 7)]),
    "nan_big_k1": dict(shape=(70, 130), seed=3273, order=1, nan=[(17, 64), (40, 63), (40, 64), (33, 5), (64, 100), (50, 127)]),
    "float32_k1": dict(shape=(13, 17), seed=3281, order=1, dtype="float32"),
    "float32_k3": dict(shape=(13, 17), seed=3282, order=3, dtype="float32"),
    "constant_1x1": dict(shape=(1, 1), seed=3283, order=1, out="square"),
})
ZOOMS = (0.37, 0.5, 1.7, 2.0)
ZOOM_SHAPE, ZOOM_SEED = (23, 31), 3291


def build(name):
    """(z, xlim, ylim, (x, y), kwargs of sample) of a sample case."""
    c = SAMPLE_CASES[name]
    shape = c["shape"]
    if shape == (1, 1):
        z = dem((4, 4), c["seed"])[:1, :1]
    else:
        z = dem(shape, c["seed"], c.get("dtype", "float64"))
    for cell in c.get("nan", ()):
        z[cell] = np.nan
    xlim, ylim = limits(shape, c.get("xdesc", False), c.get("ydesc", True))
    out = c.get("out", "spread")
    ny, nx = shape
    if out == "lines":
        x, y = on_grid_lines(xlim, nx), on_grid_lines(ylim, ny)
    elif out == "beyond":
        x = min(xlim) - 25.0 + 6.1 * np.arange(int((nx * CELL + 50.0) / 6.1) + 1)
        y = min(ylim) - 25.0 + 7.3 * np.arange(int((ny * CELL + 50.0) / 7.3) + 1)
    elif out == "fine":
        # dense, and with the limits and every cell centre: the ends of the intervals a NaN cell blanks
        x = np.unique(np.concatenate((spread(xlim, 4.3, 0.7), on_grid_lines(xlim, nx))))
        y = np.unique(np.concatenate((spread(ylim, 4.7, 0.3), on_grid_lines(ylim, ny))))
    elif out == "dense":
        x = np.concatenate(([min(xlim)], spread(xlim, 4.3, 0.7), [max(xlim)]))
        y = np.concatenate(([min(ylim)], spread(ylim, 4.7, 0.3), [max(ylim)]))
    elif out == "square":
        x, y = min(xlim) + np.array([1.0, 4.0, 9.0]), min(ylim) + np.array([2.0, 5.0, 7.0])
    else:
        big = ny * nx > 1000  # (fewer samples of the large rasters: the golden file stays small)
        x, y = spread(xlim, 23.3 if big else 7.3, 0.4), spread(ylim, 19.1 if big else 6.1, 1.7)
        if out in ("descending", "x_descending"):
            x = x[::-1]
        if out in ("descending", "y_descending"):
            y = y[::-1]
    kwargs = dict(order=c["order"], bounds_error=c.get("bounds_error", True), fill_value=c.get("fill_value", np.nan))
    return z, xlim, ylim, (x, y), kwargs


def zoom_input():
    return dem(ZOOM_SHAPE, ZOOM_SEED)


# RasterInterpolant: the rasters of a case are (seed, shape, x0 offset in cells, y0 offset in cells, cell size); x the
# coordinates of the series; call the arguments of __call__.
T0 = datetime.datetime(2013, 6, 10, 12)
INTERPOLANT_CASES = {
    "equal_grids": dict(rasters=[(3301, (20, 26), 0, 0, 10.0), (3302, (20, 26), 0, 0, 10.0), (3303, (20, 26), 0, 0, 10.0)],
                        x=[0.0, 10.0, 30.0], call=dict(xi=4.0)),
    "equal_grids_sigma": dict(rasters=[(3301, (20, 26), 0, 0, 10.0), (3302, (20, 26), 0, 0, 10.0)], sigmas="rasters",
                              x=[0.0, 10.0], call=dict(xi=7.5, return_sigma=True)),
    "number_sigmas": dict(rasters=[(3301, (20, 26), 0, 0, 10.0), (3302, (20, 26), 0, 0, 10.0)], sigmas=[0.5, 2.0],
                          x=[0.0, 10.0], call=dict(xi=2.5, return_sigma=True)),
    "no_sigmas": dict(rasters=[(3301, (20, 26), 0, 0, 10.0), (3302, (20, 26), 0, 0, 10.0)], x=[0.0, 10.0],
                      call=dict(xi=2.5, return_sigma=True)),
    "differing_grids": dict(rasters=[(3311, (20, 26), 0, 0, 10.0), (3312, (34, 40), -7, -9, 10.0)], x=[2.0, 12.0],
                            call=dict(xi=5.0)),
    "differing_grids_sigma": dict(rasters=[(3311, (20, 26), 0, 0, 10.0), (3312, (34, 40), -7, -9, 10.0)], sigmas="rasters",
                                  x=[2.0, 12.0], call=dict(xi=9.0, return_sigma=True)),
    "shifted_grids": dict(rasters=[(3313, (20, 26), 0, 0, 10.0), (3314, (24, 30), -1.3, -2.7, 10.0)], sigmas="rasters",
                              x=[2.0, 12.0], call=dict(xi=3.0, return_sigma=True)),
    "d_given": dict(rasters=[(3321, (12, 16), 0, 0, 10.0), (3322, (12, 16), 0, 0, 10.0)], sigmas="rasters", x=[0.0, 10.0],
                    call=dict(xi=6.0, d=20.0, return_sigma=True)),
    "limits_given": dict(rasters=[(3331, (20, 26), 0, 0, 10.0), (3332, (34, 40), -7, -9, 10.0)], sigmas="rasters",
                         x=[0.0, 10.0], call=dict(xi=6.0, xlim=(45.0, 190.0), ylim=(31.0, 160.0), zlim=(1000.0, 1250.0),
                                                  return_sigma=True)),
    "datetimes": dict(rasters=[(3341, (20, 26), 0, 0, 10.0), (3342, (34, 40), -7, -9, 10.0), (3343, (20, 26), 0, 0, 10.0)],
                      sigmas="rasters", x="datetimes", call=dict(xi=T0 + datetime.timedelta(days=3, hours=7),
                                                                 return_sigma=True)),
    "extrapolate": dict(rasters=[(3351, (20, 26), 0, 0, 10.0), (3352, (20, 26), 0, 0, 10.0), (3353, (20, 26), 0, 0, 10.0)],
                        sigmas="rasters", x=[0.0, 10.0, 30.0], call=dict(xi=33.0, return_sigma=True, extrapolate=True)),
}
DATETIMES = [T0, T0 + datetime.timedelta(days=11), T0 + datetime.timedelta(days=40)]


def interpolant_inputs(name):
    """(means, sigmas or None, x, call): means / sigmas as lists of (array, xlim, ylim) or numbers.  `xlim` / `ylim` of the
    call are offsets from (X0, Y0) in the case table and absolute here."""
    c = INTERPOLANT_CASES[name]
    means, sigmas = [], []
    for seed, shape, ox, oy, d in c["rasters"]:
        xlim, ylim = limits(shape, x0=X0 + ox * d, y0=Y0 + oy * d, d=d)
        means.append((dem(shape, seed), xlim, ylim))
        sigmas.append((0.5 + (vt.terrain(shape, seed + 50) + 1024.0) / 1024.0, xlim, ylim))
    kind = c.get("sigmas")
    sigmas = sigmas if kind == "rasters" else kind
    x = DATETIMES[:len(means)] if c["x"] == "datetimes" else c["x"]
    call = dict(c["call"])
    if "xlim" in call:
        call["xlim"] = (X0 + call["xlim"][0], X0 + call["xlim"][1])
        call["ylim"] = (Y0 + call["ylim"][0], Y0 + call["ylim"][1])
    return means, sigmas, x, call


# (xlim, ylim) boxes whose crop_extent is kept in the golden file, on a 13 x 17 raster with a descending y axis: inside,
# on inner cell edges (the snap-down), on the outer limits, beyond them
CROP_BOXES = [((X0 + 23.0, X0 + 91.0), (Y0 + 18.0, Y0 + 77.0)), ((X0 + 30.0, X0 + 90.0), (Y0 + 20.0, Y0 + 80.0)),
              ((X0, X0 + 170.0), (Y0, Y0 + 130.0)), ((X0 - 50.0, X0 + 60.0), (Y0 + 40.0, Y0 + 500.0)),
              ((X0 + 90.0, X0 + 30.0), (Y0 + 80.0, Y0 + 20.0)), ((X0 + 35.0, X0 + 36.0), (Y0 + 61.0, Y0 + 62.0))]
CROP_SHAPE = (13, 17)
