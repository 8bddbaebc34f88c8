"""`Raster.fill_crevasses` (raster.py:1266-1291), `helpers.maximum_filter` and `helpers.gaussian_filter` (helpers.py:347-430)
restated in NumPy with no SciPy call in the filters, and the cases of tests/golden/g30_fill_crevasses.npz.

The filters are scipy.ndimage's, spelled out:
  maximum   the separable maximum over a window of `size` cells that reaches size // 2 cells back and size - 1 - size // 2
            forward, the array extended by the boundary mode;
  Gaussian  weights exp(-0.5 / sigma^2 x^2) / sum for x = -r .. r, r = int(truncate sigma + 0.5) (or `radius`); along axis 0,
            then axis 1 (an axis whose sigma is <= 1e-15 is skipped):  tmp = in[0] w[0];  for j = -r .. -1:  tmp += (in[j] +
            in[-j]) w[j], in float64 in that order, rounded to the array's dtype after each axis.
The inputs are not stored in the golden file: `build` remakes them from the seed it keeps (exact terrain of
tests/viewshed_terrain.py less crevasses of dyadic depth), and the file holds their SHA-256.
"""
import numpy as np

from tests import viewshed_terrain as vt

ALIASES = {"grid-mirror": "reflect", "grid-wrap": "wrap"}


# ---- the filters --------------------------------------------------------------------------------------------------------
def border_index(i, n, mode):
    """scipy.ndimage's extension of an axis of n cells: reflect (d c b a | a b c d | d c b a), nearest, mirror
    (d c b | a b c d | c b a), wrap; folded as often as the index needs."""
    i = np.asarray(i)
    mode = ALIASES.get(mode, mode)
    if mode == "reflect":
        i = np.mod(i, 2 * n)
        return np.where(i >= n, 2 * n - 1 - i, i)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "mirror":
        if n == 1:
            return np.zeros_like(i)
        i = np.mod(i, 2 * n - 2)
        return np.where(i >= n, 2 * n - 2 - i, i)
    if mode == "wrap":
        return np.mod(i, n)
    raise ValueError(mode)


def _extended(a, axis, before, after, mode):
    """`a` with `axis` first, extended by `before` cells in front and `after` behind."""
    x = np.moveaxis(a, axis, 0)
    return x[border_index(np.arange(-before, x.shape[0] + after), x.shape[0], mode)]


def maximum_1d(a, size, axis, mode):
    n = a.shape[axis]
    ext = _extended(a, axis, size // 2, size - 1 - size // 2, mode)
    out = ext[0:n]
    for k in range(1, size):
        out = np.maximum(out, ext[k:k + n])
    return np.moveaxis(out, 0, axis)


def scipy_maximum(a, size, mode="reflect"):
    size = (size, size) if np.isscalar(size) else tuple(size)
    for axis in (0, 1):
        if size[axis] > 1:
            a = maximum_1d(a, int(size[axis]), axis, mode)
    return a.copy()


def gaussian_weights(sigma, truncate=4.0, radius=None):
    r = int(truncate * float(sigma) + 0.5) if radius is None else radius
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return phi / phi.sum()


def correlate_symmetric(a, w, axis, mode, work=np.float64):
    """SciPy's symmetric correlation along one axis; `work`: the type the sum is formed in (float64 as SciPy does;
    np.longdouble measures what float64 loses)."""
    r, n = len(w) // 2, a.shape[axis]
    ext = _extended(a, axis, r, r, mode).astype(work)
    w = w.astype(work)
    tmp = ext[r:r + n] * w[r]
    for j in range(-r, 0):
        tmp = tmp + (ext[r + j:r + j + n] + ext[r - j:r - j + n]) * w[r + j]
    return np.moveaxis(tmp.astype(a.dtype), 0, axis)


def scipy_gaussian(a, sigma, truncate=4.0, radius=None, mode="reflect", work=np.float64):
    sigma = (sigma, sigma) if np.isscalar(sigma) else tuple(sigma)
    radius = (radius, radius) if radius is None or np.isscalar(radius) else tuple(radius)
    for axis in (0, 1):
        if sigma[axis] > 1e-15:
            a = correlate_symmetric(a, gaussian_weights(sigma[axis], truncate, radius[axis]), axis, mode, work)
    return a.copy()


def maximum_filter(a, mask=None, fill=False, **kwargs):
    """helpers.py:390-430"""
    if mask is None:
        return scipy_maximum(a, **kwargs)
    lowest = np.finfo(a.dtype).min
    x = a.copy()
    mask = ~mask
    x[mask] = lowest
    x = scipy_maximum(x, **kwargs)
    if fill:
        mask = x == lowest
    x[mask] = a[mask]
    return x


def gaussian_filter(a, mask=None, fill=False, **kwargs):
    """helpers.py:347-387"""
    if mask is None:
        return scipy_gaussian(a, **kwargs)
    x = a.copy()
    x[~mask] = 0
    xf = scipy_gaussian(x, **kwargs)
    x[mask] = 1
    xf_sum = scipy_gaussian(x, **kwargs)
    with np.errstate(all="ignore"):
        x = xf / xf_sum
    if not fill:
        x[~mask] = a[~mask]
    return x


def fill_crevasses(a, maximum={"size": 5}, gaussian={"sigma": 5}, mask=None, fill=False):
    """raster.py:1266-1291 (returns the new array)."""
    if callable(mask):
        mask = mask(a)
    return gaussian_filter(maximum_filter(a, **maximum, mask=mask, fill=fill), **gaussian, mask=mask, fill=fill)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def crevassed(shape, seed):
    """Exact terrain with crevasse-like narrow negative noise: short one-cell-wide trenches along a row or a column, their
    depths multiples of 1/4 -- every value stays a dyadic rational, the same bytes on every machine."""
    z = vt.terrain(shape, seed)
    ny, nx = shape
    rng = np.random.default_rng(seed + 1)
    for _ in range(max(1, ny * nx // 60)):
        r, c = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        length, depth = int(rng.integers(2, 9)), int(rng.integers(8, 200)) / 4
        if rng.integers(0, 2):
            z[r, c:c + length] -= depth
        else:
            z[r:r + length, c] -= depth
    return z


def not_nan(a):
    return ~np.isnan(a)


BIG, SMALL = (40, 56), (20, 30)
DEFAULTS = dict(maximum={"size": 5}, gaussian={"sigma": 5}, mask=None, fill=False, dtype="float64")
# name -> what differs from DEFAULTS.  mask: None, "holes" (a seeded share of cells, NaN in the array), "block" (holes and a
# block wider than the Gaussian's reach), "callable" (not_nan, handed to Raster.fill_crevasses as a callable)
CASES = {
    "defaults": dict(shape=BIG),
    "holes_keep": dict(shape=BIG, mask="holes"),
    "holes_fill": dict(shape=BIG, mask="holes", fill=True),
    "block_fill": dict(shape=BIG, mask="block", fill=True, gaussian={"sigma": 1.5}),
    "callable_mask": dict(shape=SMALL, mask="callable", gaussian={"sigma": 2}),
    "float32": dict(shape=BIG, dtype="float32"),
    "float32_holes_fill": dict(shape=SMALL, dtype="float32", mask="holes", fill=True, gaussian={"sigma": 2}),
    "size_3x7": dict(shape=SMALL, mask="holes", maximum={"size": (3, 7)}, gaussian={"sigma": 2}),
    "size_4": dict(shape=SMALL, mask="holes", maximum={"size": 4}, gaussian={"sigma": 2}),
    "sigma_2_0": dict(shape=SMALL, mask="holes", gaussian={"sigma": (2, 0)}),
    "sigma_1p5_3_truncate_3": dict(shape=SMALL, gaussian={"sigma": (1.5, 3), "truncate": 3}),
    "radius_4_9": dict(shape=SMALL, mask="holes", fill=True, gaussian={"sigma": 3, "radius": (4, 9)}),
    "mode_reflect": dict(shape=SMALL, mask="holes", maximum={"size": 5, "mode": "reflect"},
                         gaussian={"sigma": 3, "mode": "reflect"}),
    "mode_nearest": dict(shape=SMALL, mask="holes", maximum={"size": 5, "mode": "nearest"},
                         gaussian={"sigma": 3, "mode": "nearest"}),
    "mode_mirror": dict(shape=SMALL, mask="holes", maximum={"size": 5, "mode": "mirror"},
                        gaussian={"sigma": 3, "mode": "mirror"}),
    "mode_wrap": dict(shape=SMALL, mask="holes", maximum={"size": 5, "mode": "wrap"}, gaussian={"sigma": 3, "mode": "wrap"}),
    "shorter_than_radius": dict(shape=(7, 9)),
    "one_row": dict(shape=(1, 60)),
    "one_column": dict(shape=(60, 1)),
    # the helpers' docstring examples that are served (helpers.py:366-375, :409-418): a = [[nan, 1], [2, nan]]
    "docstring_keep": dict(shape=(2, 2), mask="callable", maximum={"size": 3}, gaussian={"sigma": 1}),
    "docstring_fill": dict(shape=(2, 2), mask="callable", fill=True, maximum={"size": 3}, gaussian={"sigma": 1}),
}


def build(name, seed):
    """(array, maximum, gaussian, mask, fill) of a case; `mask` is None, a bool array or the callable."""
    c = {**DEFAULTS, **CASES[name]}
    shape = c["shape"]
    if name.startswith("docstring"):
        z = np.array([[np.nan, 1], [2, np.nan]])
    else:
        z = crevassed(shape, seed)
    mask = None
    if c["mask"] in ("holes", "block", "callable") and not name.startswith("docstring"):
        block = (8, 32, 10, 40) if c["mask"] == "block" else None  # 24 x 30 cells; the Gaussian of the case reaches 6
        z = vt.holes(z, seed + 2, 0.08, block)
    if c["mask"] in ("holes", "block"):
        mask = ~np.isnan(z)
    elif c["mask"] == "callable":
        mask = not_nan
    z = z.astype(c["dtype"])  # (float32: one IEEE rounding per cell, the same on every machine)
    return z, dict(c["maximum"]), dict(c["gaussian"]), mask, c["fill"]


def resolved(mask, z):
    return mask(z) if callable(mask) else mask


def same(got, want):
    """Equal in every value with the same NaN pattern (-0.0 == +0.0), same dtype and shape."""
    return got.dtype == want.dtype and got.shape == want.shape and bool(np.array_equal(got, want, equal_nan=True))


def mismatches(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    return int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum())
