"""The few functions of the reference's src/glimpse/helpers.py that the host-side raster logic needs, restated, and
`polygons_to_mask`, which runs on the GPU."""
import numpy as np


def intersect_boxes(boxes):
    """Intersection of boxes, each (xmin, ..., xmax, ...) (helpers.py:1264-1291); NaN entries are ignored."""
    boxes = np.asarray(boxes)
    if boxes.shape[1] % 2 != 0:
        raise ValueError("Box lengths are not divisible by 2")
    ndim = boxes.shape[1] // 2
    boxmin = np.nanmax(boxes[:, 0:ndim], axis=0)
    boxmax = np.nanmin(boxes[:, ndim:], axis=0)
    if any(boxmax - boxmin <= 0):
        raise ValueError("Boxes do not intersect")
    return np.hstack((boxmin, boxmax))


def bresenham_circle(center, radius):
    """Grid indices (x, y) along a circle by the midpoint circle algorithm (helpers.py:1183-1261), float64 (k, 2): from
    (x0, y0 + radius) through (x0 + radius, y0), (x0, y0 - radius) and (x0 - radius, y0) back to the start, a point that
    repeats its predecessor dropped.  `radius` is in cells; floor((sqrt(2) (radius - 1) + 4) / 2) points are walked per
    octant, and as in the reference a radius for which that count is negative is a ValueError (zero: an IndexError)."""
    x0, y0 = center
    per_octant = int(np.floor((np.sqrt(2) * (radius - 1) + 4) / 2))
    if per_octant < 0:
        raise ValueError(f"radius {radius}: negative dimensions are not allowed")
    if per_octant == 0:
        raise IndexError(f"radius {radius}: the circle has no points")
    # the first octant, from the top clockwise: step right, and down whenever the midpoint falls outside the circle
    x, y, f, dx, dy = 0, radius, 1 - radius, 1, -2 * radius
    octant = [(x, y)]
    for _ in range(per_octant - 1):
        if f > 0:
            y -= 1
            dy += 2
            f += dy
        x += 1
        dx += 2
        f += dx
        octant.append((x, y))
    a = np.array(octant, dtype=float)
    u, v = a[:, 0:1], a[:, 1:2]
    parts = [np.hstack((u, v)), np.hstack((v, u))[::-1], np.hstack((v, -u)), np.hstack((u, -v))[::-1],
             np.hstack((-u, -v)), np.hstack((-v, -u))[::-1], np.hstack((-v, u)), np.hstack((-u, v))[::-1]]
    xy = np.array((x0, y0), dtype=float) + np.vstack(parts)
    keep = np.concatenate(([True], (np.diff(xy, axis=0) != 0).any(axis=1)))
    return xy[keep]


def polygon_rings(polygons, what="polygon"):
    """[(n, 2) float64] of an iterable of rings; a ring of fewer than three vertices or with a vertex that is not finite
    is a ValueError."""
    rings = []
    for k, ring in enumerate(polygons):
        ring = np.asarray(ring, dtype=float)
        if ring.ndim != 2 or ring.shape[1] != 2:
            raise ValueError(f"{what} {k}: vertices are (x, y) pairs, got an array of shape {ring.shape}")
        if len(ring) < 3:
            raise ValueError(f"{what} {k} has {len(ring)} vertices: a ring has at least three")
        if not np.isfinite(ring).all():
            raise ValueError(f"{what} {k} has a vertex that is not finite")
        rings.append(ring)
    return rings


def polygons_to_mask(polygons, size, holes=None, return_times=False):
    """Boolean array (ny, nx) of the cells inside polygons (helpers.py:1701-1768), on the GPU (`glh_stage_polygon_mask`).
    `polygons`, `holes`: [[(x, y), ...], ...] in cell coordinates, the upper-left corner of the upper-left cell at (0, 0);
    `size`: (nx, ny).  Polygons are burnt one after another (a union), then the holes are burnt out.

    The reference hands this to GDAL's RasterizeLayer (without ALL_TOUCHED); GDAL's bytes are not pinned here.  The rule
    is stated instead, per ring and even-odd on the cell centres (c + 0.5, r + 0.5): an edge with y1 != y2 crosses row r
    when min(y1, y2) <= r + 0.5 < max(y1, y2), at x = x1 + (cy - y1) * (x2 - x1) / (y2 - y1) in float64, and toggles
    every cell of the row with c + 0.5 > x; horizontal edges do not count; a ring is closed implicitly.  So a cell is
    inside when its centre is; a centre exactly on a top or right edge is in and one on a bottom or left edge is out.
    The reference's two docstring examples come out as it prints them."""
    from . import _lib

    nx, ny = (int(v) for v in size)
    if nx < 1 or ny < 1:
        raise ValueError(f"size {tuple(size)}: at least one cell on each axis")
    rings = polygon_rings(polygons)
    hole_rings = polygon_rings(holes, "hole") if holes is not None else []
    if not rings:
        mask = np.zeros((ny, nx), dtype=bool)
        return (mask, dict.fromkeys(_lib.POLYGON_MASK_TIMES, 0.0)) if return_times else mask
    ring_off = np.concatenate(([0], np.cumsum([len(r) for r in rings + hole_rings])))
    if ring_off[-1] >= 2 ** 31:
        raise ValueError(f"{ring_off[-1]} vertices: fewer than 2^31 are served")
    return _lib.stage_polygon_mask(np.vstack(rings + hole_rings), ring_off, len(rings), len(hole_rings), nx, ny,
                                   return_times=return_times)
