"""The few functions of the reference's src/glimpse/helpers.py that the host-side raster logic and the camera calibration
(`optimize.Lines`: splitting, clipping and resampling polylines) need, restated, and `polygons_to_mask`, which runs on the
GPU."""
import gzip
import pickle
from pathlib import Path

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


# ---- polylines (optimize.Lines) ------------------------------------------------------------------------------------------
def boolean_split(a, mask, axis=0, circular=False, include="all"):
    """helpers.py:762-812: `a` cut where `mask` changes, as a list of runs; `include`: "all" runs, or only the "true" or
    the "false" ones.  `circular`: the last run joins the first when both ends of `mask` hold the same value."""
    mask = np.asarray(mask)
    cuts = np.nonzero(mask[1:] != mask[:-1])[0] + 1
    splits = np.split(a, cuts, axis=axis)
    if circular and len(splits) > 1 and mask[0] == mask[-1]:
        splits[0] = np.concatenate((splits[-1], splits[0]), axis=axis)
        splits.pop(-1)
    if include == "all":
        return splits
    if include == "true":
        return splits[slice(0, None, 2) if mask[0] else slice(1, None, 2)]
    if include == "false":
        return splits[slice(1, None, 2) if mask[0] else slice(0, None, 2)]
    return []


def unravel_box(box):
    """helpers.py:1414-1436: (xmin, ..., xmax, ...) as [(xmin, ...), (xmax, ...)]."""
    box = np.asarray(box)
    if box.size % 2 != 0:
        raise ValueError("Box length is not divisible by 2")
    return box.reshape(-1, box.size // 2)


def in_box(points, box):
    """helpers.py:815-832: which points (n, ndim) lie in or on the box."""
    box = unravel_box(box)
    return np.all((points >= box[0, :]) & (points <= box[1, :]), axis=1)


def intersect_rays_box(origin, directions, box, t=False):
    """helpers.py:919-1001: entrances and exits of rays from one `origin` through an axis-aligned box (2-d or 3-d), NaN
    for a miss, an origin inside the box (entrance) or an intersection behind the ray; `t`: as multiples of `directions`
    (n, 1) instead of coordinates."""
    directions = np.asarray(directions, dtype=float)
    box = np.asarray(box, dtype=float).ravel()
    ndims = directions.shape[1]
    with np.errstate(divide="ignore"):
        invdir = 1 / directions
    sign = invdir < 0
    with np.errstate(invalid="ignore"):
        def slab(axis):  # the near and the far bound of an axis, along the ray
            near = np.where(sign[:, axis], box[axis + ndims], box[axis])
            far = np.where(sign[:, axis], box[axis], box[axis + ndims])
            return (near - origin[axis]) * invdir[:, axis], (far - origin[axis]) * invdir[:, axis]

        tmin, tmax = slab(0)
        for axis in range(1, min(ndims, 3)):
            amin, amax = slab(axis)
            misses = (tmin > amax) | (amin > tmax)
            tmin[misses] = np.nan
            tmax[misses] = np.nan
            later = amin > tmin
            tmin[later] = amin[later]
            sooner = amax < tmax
            tmax[sooner] = amax[sooner]
        tmin[tmin < 0] = np.nan
        tmax[tmax < 0] = np.nan
    if t:
        return tmin[:, None], tmax[:, None]
    return origin + tmin[:, None] * directions, origin + tmax[:, None] * directions


def intersect_rays_plane(rays, plane):
    """helpers.py:1053-1101: where the rays (n, 6) = (x0, y0, z0, dx, dy, dz) meet the infinite plane
    (x0, y0, z0, dx1, dy1, dz1, dx2, dy2, dz2) through a point and along two directions: (n, 3), NaN for a ray that is
    parallel to the plane (|normal . direction| <= 1e-14, a ray lying in the plane included) or that has the plane behind
    it.  The sea-level companion of `Raster.intersect_rays`."""
    rays = np.atleast_2d(np.asarray(rays, dtype=float))
    plane = np.asarray(plane, dtype=float)
    normal = np.cross(plane[3:6], plane[6:9])
    along = (normal * rays[:, 3:6]).sum(axis=1)
    points = np.full((len(rays), 3), np.nan)
    meets = np.abs(along) > 1e-14
    t = (normal * (plane[0:3] - rays[meets, 0:3])).sum(axis=1) / along[meets]
    ahead = t >= 0
    meets[meets] = ahead
    points[meets] = rays[meets, 0:3] + t[ahead, None] * rays[meets, 3:6]
    return points


def intersect_edge_box(origin, distance, box):
    """helpers.py:890-916: the multiple of `distance` in (0, 1) at which the edge from `origin` meets the box, or None."""
    import warnings

    distance = np.asarray(distance).reshape(1, -1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (all-NaN: a miss)
        t = np.nanmin(intersect_rays_box(origin, distance, box, t=True))
    if t > 0 and t < 1:
        return t
    return None


def clip_polyline_box(line, box, t=False):
    """helpers.py:835-887: the runs of `line` (n, ndim [+ 1 distance measure if `t`]) inside the box, each with a vertex
    inserted where it crosses the boundary.  A crossing between two consecutive outside vertices is not looked for."""
    cols = slice(None, -1) if t else slice(None)
    mask = in_box(line[:, cols], box)
    segments = boolean_split(line, mask)
    trues = slice(int(~mask[0]), None, 2)
    nsegments = len(segments)
    for i in range(*trues.indices(nsegments)):
        if i > 0:
            origin = segments[i - 1][-1, :]
            distance = segments[i][0, :] - origin
            ti = intersect_edge_box(origin[cols], distance[cols], box)
            if ti is not None:
                segments[i] = np.vstack((origin + ti * distance, segments[i]))
        if i < nsegments - 1:
            origin = segments[i][-1, :]
            distance = segments[i + 1][0, :] - origin
            ti = intersect_edge_box(origin[cols], distance[cols], box)
            if ti is not None:
                segments[i] = np.vstack((segments[i], origin + ti * distance))
    return segments[trues]


def line_distances(vertices):
    """The cumulative Euclidean distance at each vertex, from 0 (helpers.py:1373-1377)."""
    return np.insert(np.cumsum(np.sqrt(np.sum(np.diff(vertices, axis=0) ** 2, axis=1))), 0, 0)


def line_count(x, dx):
    """How many evenly spaced points `interpolate_line(dx=dx)` places over the distances `x` (helpers.py:1380-1383)."""
    n = abs((x[-1] - x[0]) / dx)
    if n == int(n):
        n += 1
    return int(round(n))


def interpolate_line(vertices, x=None, xi=None, n=None, dx=None, error=True, fill="endpoints"):
    """helpers.py:1322-1411: points at the distances `xi` along a polyline -- or `n` evenly spaced ones, or ones nominally
    `dx` apart -- by linear interpolation between the vertices, whose distance measures are `x` (default: cumulative
    Euclidean distance)."""
    vertices = np.asarray(vertices)
    if all((xi is None, n is None, dx is None)):
        raise ValueError("One of xi, n, or dx is required")
    if x is None:
        x = line_distances(vertices)
    if xi is None:
        if n is None:
            n = line_count(x, dx)
        xi = np.linspace(start=x[0], stop=x[-1], num=n, endpoint=True)
        error = False
        fill = "endpoints"
    if len(x) > 1 and x[1] < x[0]:
        sort_index = np.argsort(x)
        x = x[sort_index]
        vertices = vertices[sort_index, :]
    result = np.column_stack([np.interp(xi, x, vertices[:, i]) for i in range(vertices.shape[1])])
    if isinstance(fill, str) and fill == "endpoints":
        if error is False:
            return result
        fill = (vertices[0], vertices[-1])
    if not np.iterable(fill):
        fill = (fill, fill)
    left = np.less(xi, x[0])
    right = np.greater(xi, x[-1])
    if x[0] > x[-1]:
        right, left = left, right
    if error and (left.any() or right.any()):
        raise ValueError("Requested distance outside range")
    result[left, :] = fill[0]
    result[right, :] = fill[1]
    return result


def strip_path(path, extensions=True):
    """helpers.py:137-160: the final component of `path` without its file extensions (`extensions`: how many at the
    most, True for all)."""
    basename = Path(path).name
    if extensions:
        if extensions is True:
            extensions = -1
        return basename[::-1].split(".", maxsplit=extensions)[-1][::-1]
    return basename


def write_pickle(obj, path, gz=False, binary=True, **kwargs):
    """helpers.py:210-235: `obj` as a pickle at `path` (its directory is made)."""
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    mode = "wb" if binary else "w"
    with (gzip.open(path, mode=mode) if gz else open(path, mode=mode)) as fp:
        pickle.dump(obj, file=fp, **kwargs)


def read_pickle(path, gz=False, binary=True, **kwargs):
    """helpers.py:238-257: the object of the pickle at `path`."""
    mode = "rb" if binary else "r"
    with (gzip.open(path, mode=mode) if gz else open(path, mode=mode)) as fp:
        return pickle.load(fp, **kwargs)
