"""`displacements`: dense template matching between two frames on the GPU -- a template around each point of a grid in
one frame, found in another frame by zero-normalised cross-correlation, the displacement read off the peak.  The
reference leaves this to its users (ImGRAFT's `templatematch` does it); the rule is INPUTS.md, "Displacements: the rule",
restated in NumPy in tests/displacement_rule.py, which the device equals bit for bit.  It gives a velocity field over two
orthophotos (`Observer.orthorectify`), hence a prior `vxyz`, `vxyz_sigma` for a motion model; it also works on the raw
frames of a fixed camera."""
import numpy as np

from . import _lib

MIN_SIDE, MAX_SIDE, MAX_REACH = 3, 63, 32
FRAME_DTYPES = ("uint8", "uint16", "float32", "float64")  # what the Tracker takes


def check_arguments(shape, dtype, uv, size, reach):
    """The refusals of `displacements`, made before the library is loaded: (uv (n, 2) float64, (w, h), (rx, ry))."""
    if np.size(size) != 2 or np.size(reach) != 2:
        raise ValueError(f"size and reach are pairs, got {size} and {reach}")
    size, reach = tuple(int(v) for v in size), tuple(int(v) for v in reach)
    if not all(MIN_SIDE <= v <= MAX_SIDE for v in size):
        raise ValueError(f"template sides of {MIN_SIDE} .. {MAX_SIDE} pixels, got {size}")
    if not all(1 <= v <= MAX_REACH for v in reach):
        raise ValueError(f"a reach of 1 .. {MAX_REACH} pixels per axis, got {reach}")
    if np.dtype(dtype).name not in FRAME_DTYPES or not (len(shape) == 2 or (len(shape) == 3 and shape[2] == 3)):
        raise NotImplementedError("frames must be uint8, uint16, float32 or float64, two-dimensional or with three "
                                  f"channels, not {np.dtype(dtype)} {tuple(shape)}")
    uv = np.asarray(uv, dtype=np.float64)
    if uv.ndim != 2 or uv.shape[1] != 2:
        raise ValueError(f"uv must be (n, 2), got {uv.shape}")
    return uv, size, reach


def frame_plane(array):
    """The plane of pixels that is matched: a 2-D uint8 frame as it is (the integer path); everything else as float32
    (the float path) -- three channels averaged first by array.mean(axis=2), in float64 as the Tracker does."""
    array = np.asarray(array)
    if array.ndim == 3:
        array = array.mean(axis=2)
    return array if array.dtype == np.uint8 else array.astype(np.float32)


def template_boxes(uv, size, shape):
    """`Observer.tile_box`'s expression for all points at once, without its raise: (corners (n, 2) int32 = (l, t) with
    l = floor(u - w / 2 + 0.5), t = floor(v - h / 2 + 0.5), inside (n,) bool: the box [l, l + w) x [t, t + h) is finite
    and lies in a frame of `shape` = (rows, cols))."""
    uv = np.asarray(uv, dtype=np.float64)
    halfsize = np.multiply(size, 0.5)
    imgsz = np.array([shape[1], shape[0]], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        low, high = uv - halfsize, uv + halfsize
        inside = np.all((low >= 0) & (low <= imgsz) & (high >= 0) & (high <= imgsz), axis=1)  # (False for NaN)
    corners = np.zeros(uv.shape, dtype=np.int32)
    corners[inside] = np.floor(low[inside] + 0.5).astype(np.int32)
    return corners, inside


def whole_guess(guess):
    """g = rint(guess) as int32; a guess that is not finite, or beyond the limit, becomes the limit, where no window of
    any frame is inside."""
    guess = np.asarray(guess, dtype=np.float64)
    limit = float(_lib.DISPLACEMENT_GUESS_LIMIT)
    with np.errstate(invalid="ignore"):
        g = np.clip(np.rint(guess), -limit, limit)
    return np.where(np.isfinite(guess), g, limit).astype(np.int32)


def _run(planes, pairs, uv, size, reach, guess, subpixel, return_surface):
    """`planes` (F, rows, cols) through one library call -> (duv (P, n, 2), score (P, n), status (P, n)[, surface])."""
    p, n = len(pairs), len(uv)
    if n == 0:
        out = (np.empty((p, 0, 2)), np.empty((p, 0)), np.empty((p, 0), dtype=np.uint8))
        return (*out, np.empty((p, 0, 2 * reach[1] + 1, 2 * reach[0] + 1))) if return_surface else out
    corners, inside = template_boxes(uv, size, planes.shape[1:])
    return _lib.stage_displacements(planes, pairs, corners, inside.astype(np.uint8),
                                    None if guess is None else whole_guess(guess), size, reach, subpixel=subpixel,
                                    return_surface=return_surface)


def displacements(a, b, uv, size=(31, 31), reach=(16, 16), guess=None, subpixel=True, return_surface=False):
    """Where the surroundings of the points `uv` (n, 2) of frame `a` are in frame `b`: (duv (n, 2) float64, score (n,)
    float64, status (n,) uint8), the point's position in `b` being uv + duv.  `a` and `b` are two frames of one pixel
    shape, 2-D or with three channels, of uint8, uint16, float32 or float64.  A template of `size` = (w, h) pixels
    (3 .. 63 a side) around each point -- the box of `Observer.tile_box` -- is compared with the windows of `b` at the
    offsets -rx .. rx by -ry .. ry (`reach`, 1 .. 32 per axis) around rint(`guess`) ((n, 2), or None for 0) by
    zero-normalised cross-correlation; the largest score wins (the first in row-major order among equals) and, with
    `subpixel`, a parabola through it and its two neighbours refines each axis.  `score` is the peak's, in [-1, 1].
    `status` indexes `_lib.DISPLACEMENT_STATUS`: "matched"; "peak on the edge" (a valid result without a sub-pixel term
    on some axis, because the peak lies on the border of the range or beside an invalid offset: the reach is too
    small); and, with NaN in `duv` and `score`, "no valid offset" (no window lies inside `b` with pixels that vary),
    "flat template" (a template that is constant or holds a NaN) and "template outside" (a `uv` that is not finite, or a
    box that leaves the frame).  `return_surface`: also the scores of all offsets (n, 2 ry + 1, 2 rx + 1), NaN where an
    offset is invalid.  A 2-D uint8 frame is matched in exact integer arithmetic; every other frame as float32 (three
    channels averaged first, array.mean(axis=2)), where a NaN or infinite pixel invalidates what it touches -- the NaN
    cells of an orthophoto need no mask.  The rule is INPUTS.md, "Displacements: the rule"."""
    a, b = np.asarray(a), np.asarray(b)
    uv, size, reach = check_arguments(a.shape, a.dtype, uv, size, reach)
    check_arguments(b.shape, b.dtype, uv, size, reach)
    if a.shape != b.shape:
        raise ValueError(f"frames differ in shape: {a.shape} and {b.shape}")
    if guess is not None and np.shape(guess) != uv.shape:
        raise ValueError(f"guess must be {uv.shape}, got {np.shape(guess)}")
    pa, pb = frame_plane(a), frame_plane(b)
    if pa.dtype != pb.dtype:  # (a uint8 frame beside another type: both on the float path)
        pa, pb = pa.astype(np.float32), pb.astype(np.float32)
    out = _run(np.stack([pa, pb]), np.array([[0, 1]], dtype=np.int32), uv, size, reach, guess, subpixel, return_surface)
    return tuple(v[0] for v in out)


def sequence_displacements(arrays, uv, step=1, size=(31, 31), reach=(16, 16), guess=None, subpixel=True,
                           return_surface=False):
    """`displacements` of frame k and frame k + step over `arrays` (frames of one shape and dtype), every frame uploaded
    once: (duv (pairs, n, 2), score (pairs, n), status (pairs, n)[, surface (pairs, n, 2 ry + 1, 2 rx + 1)])."""
    step = int(step)
    if step < 1 or len(arrays) <= step:
        raise ValueError(f"step {step} leaves no pair among {len(arrays)} images")
    if len({(np.shape(f), np.asarray(f).dtype) for f in arrays}) != 1:
        raise ValueError("Images differ in shape or dtype: " +
                         str(sorted({(np.shape(f), str(np.asarray(f).dtype)) for f in arrays})))
    first = np.asarray(arrays[0])
    uv, size, reach = check_arguments(first.shape, first.dtype, uv, size, reach)
    n_pairs = len(arrays) - step
    if guess is not None and np.shape(guess) not in (uv.shape, (n_pairs, *uv.shape)):
        raise ValueError(f"guess must be {uv.shape} or {(n_pairs, *uv.shape)}, got {np.shape(guess)}")
    pairs = np.stack([np.arange(n_pairs), np.arange(n_pairs) + step], axis=1).astype(np.int32)
    return _run(np.stack([frame_plane(f) for f in arrays]), pairs, uv, size, reach, guess, subpixel, return_surface)
