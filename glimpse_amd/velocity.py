"""`velocity_field`: from the raw vectors of `displacements` to a velocity field on the GPU -- every vector tested against
its neighbours on the grid (the normalised median test of Westerweel & Scarano, 2005, per image pair), and the survivors of
all pairs stacked into a median velocity, a robust spread (1.4826 x the median absolute deviation) and a count per node:
the prior `vxyz`, `vxyz_sigma` a motion model asks for.  The reference has no such function; the rule is INPUTS.md,
"Velocity field: the rule", restated in NumPy in tests/velocity_field_rule.py, which the device equals bit for bit."""
import datetime

import numpy as np

from . import _lib

MAX_PAIRS, MAX_RADIUS = 1024, 2


def seconds(dt, pairs):
    """`dt` -- a number or a datetime.timedelta for every pair, or `pairs` of them -- as (pairs,) float64 seconds."""
    if isinstance(dt, datetime.timedelta) or np.ndim(dt) == 0:
        dt = [dt] * pairs
    dt = [v.total_seconds() if isinstance(v, datetime.timedelta) else v for v in dt]
    dt = np.asarray(dt, dtype=np.float64)
    if dt.shape != (pairs,):
        raise ValueError(f"dt must be a number or ({pairs},), got {dt.shape}")
    if not np.all(np.isfinite(dt) & (dt != 0)):
        raise ValueError("every dt must be finite and not zero")
    return dt


def check_arguments(duv, score, status, grid, dt, scale, radius, min_neighbors, threshold, epsilon, min_count):
    """The refusals of `velocity_field`, made before the library is loaded: (duv (P, n, 2) float64, score (P, n) float64,
    status (P, n) uint8, (rows, cols), dt (P,) float64 seconds, (scale_u, scale_v), radius, threshold) -- a single pair
    given without the leading axis gets it, and `threshold` None is radius 0."""
    duv, score, status = np.asarray(duv, dtype=np.float64), np.asarray(score, dtype=np.float64), np.asarray(status)
    if duv.ndim == 2 and score.ndim == 1 and status.ndim == 1:
        duv, score, status = duv[None], score[None], status[None]
    if duv.ndim != 3 or duv.shape[2] != 2:
        raise ValueError(f"duv must be (P, n, 2) or (n, 2), got {duv.shape}")
    p, n = duv.shape[:2]
    if score.shape != (p, n) or status.shape != (p, n):
        raise ValueError(f"score and status must be {(p, n)} beside duv {duv.shape}, got {score.shape} and {status.shape}")
    if not 1 <= p <= MAX_PAIRS:
        raise ValueError(f"1 .. {MAX_PAIRS} pairs, got {p}")
    if status.dtype != np.uint8:
        if status.dtype.kind not in "iub":
            raise ValueError(f"status must be integers, got {status.dtype}")
        status = np.clip(status, 0, 255).astype(np.uint8)  # (below 0: a candidate as 0 is; above 255: none, as 255)
    if np.size(grid) != 2:
        raise ValueError(f"grid is (rows, cols), got {grid}")
    rows, cols = (int(v) for v in grid)
    if rows < 0 or cols < 0 or rows * cols != n:
        raise ValueError(f"a grid of {rows} x {cols} nodes for {n} points")
    if threshold is None:
        radius, threshold = 0, 2.0
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError(f"a radius of 0 .. {MAX_RADIUS} nodes, got {radius}")
    most = (2 * radius + 1) ** 2 - 1
    if radius > 0 and not 1 <= int(min_neighbors) <= most:
        raise ValueError(f"min_neighbors of 1 .. {most} at radius {radius}, got {min_neighbors}")
    for name, value in (("threshold", threshold), ("epsilon", epsilon)):
        if not (np.isfinite(value) and value > 0):
            raise ValueError(f"{name} must be finite and positive, got {value}")
    if int(min_count) < 1:
        raise ValueError(f"min_count must be at least 1, got {min_count}")
    dt = seconds(dt, p)
    if np.shape(scale) != (2,) or not np.all(np.isfinite(np.asarray(scale, dtype=np.float64))):
        raise ValueError(f"scale must be two finite numbers, got {scale}")
    return duv, score, status, (rows, cols), dt, (float(scale[0]), float(scale[1])), radius, float(threshold)


def velocity_field(duv, score, status, grid, dt=1.0, scale=(1.0, 1.0), min_score=0.0, accept_edge=True, radius=1,
                   min_neighbors=3, threshold=2.0, epsilon=0.1, min_count=1, return_kept=False):
    """The velocity field of the displacements `duv` (P, n, 2), `score` (P, n), `status` (P, n) -- what
    `Observer.displacements` returns for P image pairs; (n, 2), (n,), (n,) mean one pair -- at the nodes of a regular
    grid, `grid` = (rows, cols) with rows * cols == n, in row-major order: (v (n, 2) float64, sigma (n, 2) float64,
    count (n,) int32), and with `return_kept` also kept (P, n) bool.

    A vector is a candidate when its status is "matched" (or "peak on the edge", with `accept_edge`), its score is at
    least `min_score` and both components are finite.  Per pair, a candidate is kept when at least `min_neighbors` of
    the nodes within `radius` (0, 1 or 2) rows and columns of it are candidates and, on both components,
    |x - med| / (res + epsilon) <= threshold, where med is the median of the neighbours' values and res the median of
    their absolute deviations from it; `epsilon` is the measurement noise in pixels.  `radius` 0 or `threshold` None
    keeps every candidate.  Per node and component, the kept vectors of all pairs become x = duv * scale / dt --
    `scale` a pair, for example a DEM's cell size `dem.d`; `dt` a number, or P numbers or datetime.timedeltas (seconds)
    -- and v is their median, sigma 1.4826 times the median of |x - v| (0 from a single pair), count their number; a
    node with fewer than `min_count` has NaN in v and sigma.  The rule is INPUTS.md, "Velocity field: the rule"."""
    duv, score, status, grid, dt, scale, radius, threshold = check_arguments(
        duv, score, status, grid, dt, scale, radius, min_neighbors, threshold, epsilon, min_count)
    p, n = duv.shape[:2]
    if n == 0:
        out = (np.empty((0, 2)), np.empty((0, 2)), np.empty(0, dtype=np.int32))
        return (*out, np.empty((p, 0), dtype=bool)) if return_kept else out
    *out, kept = _lib.stage_velocity_field(duv, score, status, grid, dt, scale, min_score, accept_edge, radius,
                                           min_neighbors if radius else 1, threshold, epsilon, min_count)
    return (*out, kept) if return_kept else tuple(out)
