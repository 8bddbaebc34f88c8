"""`maximum_filter` and `gaussian_filter` of `glimpse.helpers` (helpers.py:347-430) on the GPU: scipy.ndimage's filters
with cells excluded by a mask, the two halves of `Raster.fill_crevasses` (raster.py:1266-1291).

    maximum_filter(a, mask=None, fill=False, size=5)
    gaussian_filter(a, mask=None, fill=False, sigma=5)

Both return a new array of `a`'s dtype and shape and equal the reference's (SciPy's) result in every bit: the kernels
(`glh_stage_max_filter`, `glh_stage_gaussian_filter`; csrc/glh_filters.hip) add, multiply and divide in SciPy's order, and
the Gaussian's weights are made here with NumPy exactly as SciPy makes them.

Served: two-dimensional float64 / float32 arrays; `size` (an int or a (rows, columns) pair, odd or even) and `mode` for the
maximum; `sigma` (a scalar or a pair), `truncate`, `radius` and `mode` for the Gaussian; `mode` one of "reflect", "nearest",
"mirror", "wrap" (or SciPy's aliases "grid-mirror", "grid-wrap").  Everything else is refused before the library is loaded
(INPUTS.md, round 9): `footprint`, `origin`, `output`, `axes`, `mode="constant"` / `cval`, a non-zero `order`
(NotImplementedError naming the argument), integer arrays (NotImplementedError: convert first -- the reference divides by a
weight sum truncated to 0 or 1), a NaN at an included cell (ValueError naming `mask`: SciPy's maximum there depends on its
comparison order, and an unmasked Gaussian spreads the NaN over its whole reach), a mask of another shape (ValueError).
"""
import numbers

import numpy as np

from . import _lib

MODES = _lib.HIGHPASS_MODES  # the boundary modes the device's border_index knows, with scipy's grid-* aliases
GAUSSIAN_SKIP = 1e-15  # scipy.ndimage.gaussian_filter filters an axis only when its sigma exceeds this


def _refuse(who, kwargs, defaults, allowed):
    """NotImplementedError for a scipy argument that is not built (unless it holds scipy's default), TypeError for a name
    scipy does not know."""
    for name, value in kwargs.items():
        if name in allowed:
            continue
        if name not in defaults:
            raise TypeError(f"{who}() got an unexpected keyword argument '{name}'")
        default = defaults[name]
        if value is default or (default is not None and np.isscalar(value) and value == default):
            continue
        raise NotImplementedError(f"{who}: `{name}` is not built (served: {', '.join(allowed)})")


def _mode(who, kwargs):
    mode = kwargs.get("mode", "reflect")
    if not isinstance(mode, str):
        raise NotImplementedError(f"{who}: `mode` per axis is not built (one mode for both axes)")
    if mode == "constant":
        raise NotImplementedError(f"{who}: `mode`=\"constant\" (and `cval`) is not built: {sorted(MODES)} are")
    if mode not in MODES:
        raise RuntimeError("boundary mode not supported")  # (scipy's own error)
    return MODES[mode]


def _pair(who, name, value):
    if np.isscalar(value) or value is None:
        return (value, value)
    value = tuple(value)
    if len(value) != 2:
        raise RuntimeError(f"{who}: sequence argument `{name}` must have length equal to input rank")  # (as scipy)
    return value


def maximum_arguments(kwargs):
    """scipy.ndimage.maximum_filter's keyword arguments -> (rows, columns, mode code)."""
    who = "maximum_filter"
    _refuse(who, kwargs, {"footprint": None, "output": None, "cval": 0.0, "origin": 0, "axes": None}, ("size", "mode"))
    if kwargs.get("size") is None:
        raise RuntimeError("no footprint or filter size provided")  # (scipy's own error)
    size = _pair(who, "size", kwargs["size"])
    if not all(isinstance(s, numbers.Integral) and s >= 1 for s in size):
        raise ValueError(f"{who}: `size` {kwargs['size']!r}: positive integers")
    return int(size[0]), int(size[1]), _mode(who, kwargs)


def gaussian_weights(sigma, truncate=4.0, radius=None):
    """scipy.ndimage's _gaussian_kernel1d(sigma, 0, radius) as gaussian_filter1d calls it (float64, symmetric), or None
    where gaussian_filter skips the axis."""
    if not sigma > GAUSSIAN_SKIP:
        return None
    lw = int(truncate * float(sigma) + 0.5)
    if radius is not None:
        lw = radius
    if not isinstance(lw, numbers.Integral) or lw < 0:
        raise ValueError("Radius must be a nonnegative integer.")  # (scipy's own error)
    sigma2 = sigma * sigma
    x = np.arange(-lw, lw + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    return np.ascontiguousarray(phi_x / phi_x.sum(), dtype=np.float64)


def gaussian_arguments(kwargs):
    """scipy.ndimage.gaussian_filter's keyword arguments -> (weights along rows or None, along columns or None, mode)."""
    who = "gaussian_filter"
    _refuse(who, kwargs, {"order": 0, "output": None, "cval": 0.0, "axes": None}, ("sigma", "truncate", "radius", "mode"))
    if "sigma" not in kwargs:
        raise TypeError("gaussian_filter() missing 1 required positional argument: 'sigma'")
    sigma = _pair(who, "sigma", kwargs["sigma"])
    radius = _pair(who, "radius", kwargs.get("radius"))
    truncate = kwargs.get("truncate", 4.0)
    mode = _mode(who, kwargs)
    w = [gaussian_weights(s, truncate, r) for s, r in zip(sigma, radius)]
    return w[0], w[1], mode


def checked(who, a, mask):
    """(array, mask as uint8 or None) as the kernels take them, after the refusals of the module's docstring."""
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        raise NotImplementedError(f"{who}: an integer array ({a.dtype}) is not built: convert it first, "
                                  "a.astype(float) (the reference divides by a weight sum truncated to 0 or 1)")
    if a.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise NotImplementedError(f"{who}: an array of dtype {a.dtype} is not built: float64 or float32")
    if a.ndim != 2:
        raise NotImplementedError(f"{who}: a {a.ndim}-dimensional array is not built: two dimensions")
    if a.size == 0:
        raise ValueError(f"{who}: an empty array {a.shape}")
    if mask is not None:
        mask = np.asarray(mask)
        if mask.shape != a.shape:
            raise ValueError(f"{who}: `mask` of shape {mask.shape} for an array of shape {a.shape}")
        mask = np.ascontiguousarray(mask, dtype=bool)
    nan = np.isnan(a)
    if mask is not None:
        nan &= mask
    if nan.any():
        r, c = (int(v[0]) for v in np.nonzero(nan))
        raise ValueError(f"{who}: NaN at {int(nan.sum())} included cells (the first at row {r}, column {c}): exclude them "
                         "with `mask`, e.g. mask=~np.isnan(a)")
    return np.ascontiguousarray(a), None if mask is None else mask.view(np.uint8)


def maximum_filter(a, mask=None, fill=False, **kwargs):
    """helpers.maximum_filter (helpers.py:390-430): scipy.ndimage.maximum_filter(a, **kwargs) with the cells where `mask`
    is False excluded (they count as the dtype's lowest value); `a`'s own values stay at the excluded cells, or with
    `fill` only at those whose whole window is excluded."""
    size_y, size_x, mode = maximum_arguments(kwargs)
    a, mask = checked("maximum_filter", a, mask)
    return _lib.stage_max_filter(a, mask, fill, size_y, size_x, mode)


def gaussian_filter(a, mask=None, fill=False, **kwargs):
    """helpers.gaussian_filter (helpers.py:347-387): scipy.ndimage.gaussian_filter(a, **kwargs), with a `mask` as the
    filtered array (0 at excluded cells) over the filtered mask; `a`'s own values stay at the excluded cells unless
    `fill`, which leaves NaN where no included cell is in reach."""
    w0, w1, mode = gaussian_arguments(kwargs)
    a, mask = checked("gaussian_filter", a, mask)
    return _lib.stage_gaussian_filter(a, mask, fill, w0, w1, mode)


def fill_crevasses(a, maximum, gaussian, mask=None, fill=False, return_times=False):
    """gaussian_filter(maximum_filter(a, **maximum, mask, fill), **gaussian, mask, fill) in one library call
    (`glh_stage_fill_crevasses`): one upload, one download, the maximum stays on the device."""
    size_y, size_x, max_mode = maximum_arguments(dict(maximum))
    w0, w1, gauss_mode = gaussian_arguments(dict(gaussian))
    a, mask = checked("fill_crevasses", a, mask)
    return _lib.stage_fill_crevasses(a, mask, fill, size_y, size_x, max_mode, w0, w1, gauss_mode, return_times=return_times)
