"""The rule of `glimpse_amd.velocity_field` (INPUTS.md, "Velocity field: the rule") restated in NumPy: the candidates, the
neighbour test per pair and the stack over the pairs.  Every operation is a float64 operation of NumPy's, one at a time;
the selections are `np.sort` over arrays padded with +inf, so that 10^5 node-pairs take seconds.  The device equals what
this module returns in every bit (tests/test_gpu_velocity_field.py)."""
import datetime

import numpy as np

SIGMA_OF_MAD = 1.4826
CHUNK = 1 << 17  # node-pairs of one slab of the neighbour test


def median_padded(s, m, axis=-1):
    """The median of the first `m` values along `axis` of `s`, sorted ascending along it and padded with +inf:
    s[m // 2] for odd m, (s[m // 2 - 1] + s[m // 2]) / 2 for even m; NaN where m is 0."""
    s = np.moveaxis(s, axis, -1)
    m = np.asarray(m)
    h = (m // 2)[..., None]
    hi = np.take_along_axis(s, np.minimum(h, s.shape[-1] - 1), axis=-1)[..., 0]
    lo = np.take_along_axis(s, np.maximum(h - 1, 0), axis=-1)[..., 0]
    with np.errstate(all="ignore"):
        med = np.where(m % 2 == 1, hi, (lo + hi) / 2.0)
    return np.where(m > 0, med, np.nan)


def candidates(duv, score, status, min_score=0.0, accept_edge=True):
    """cand (P, n): the status is at most 1 (0 without `accept_edge`), the score at least `min_score` (false for NaN), both
    components finite."""
    with np.errstate(invalid="ignore"):
        return (status <= (1 if accept_edge else 0)) & (score >= min_score) & np.isfinite(duv).all(axis=-1)


def neighbour_test(duv, cand, grid, radius=1, min_neighbors=3, threshold=2.0, epsilon=0.1):
    """kept (P, n) of `duv` (P, n, 2) and `cand` (P, n) on a grid of `grid` = (rows, cols) nodes; also the number of
    neighbours of every node (P, n), for the tests to look at."""
    rows, cols = grid
    p = len(duv)
    if radius == 0:
        return cand.copy(), np.zeros(cand.shape, dtype=np.int64)
    r = radius
    values = np.where(cand[..., None], duv + 0.0, np.inf).reshape(p, rows, cols, 2)
    padded = np.full((p, rows + 2 * r, cols + 2 * r, 2), np.inf)
    padded[:, r:r + rows, r:r + cols] = values
    kept, number = np.zeros((p, rows, cols), dtype=bool), np.zeros((p, rows, cols), dtype=np.int64)
    per = max(1, CHUNK // max(1, rows * cols))
    for p0 in range(0, p, per):
        sl = slice(p0, p0 + per)
        nb = np.stack([padded[sl, r + dy:r + dy + rows, r + dx:r + dx + cols] for dy in range(-r, r + 1)
                       for dx in range(-r, r + 1) if (dy, dx) != (0, 0)], axis=-1)  # (p, rows, cols, 2, N)
        s = np.sort(nb, axis=-1)
        m = (s[..., 0, :] < np.inf).sum(axis=-1)  # (the same for both components)
        with np.errstate(all="ignore"):
            med = median_padded(s, m[..., None])
            res = median_padded(np.sort(np.abs(s - med[..., None]) + 0.0, axis=-1), m[..., None])
            ok = np.abs(values[sl] - med) / (res + epsilon) <= threshold
        kept[sl] = cand.reshape(p, rows, cols)[sl] & (m >= min_neighbors) & ok.all(axis=-1)
        number[sl] = m
    return kept.reshape(p, -1), number.reshape(p, -1)


def stack(duv, kept, dt, scale=(1.0, 1.0), min_count=1):
    """(v (n, 2), sigma (n, 2), count (n,) int32) of the kept vectors of `duv` (P, n, 2): per node and component
    x = duv * scale / dt over the kept pairs, their median and 1.4826 times the median of |x - v|."""
    p, n = kept.shape
    dt = np.asarray(dt, dtype=np.float64).reshape(p, 1, 1)
    with np.errstate(all="ignore"):
        x = duv * np.asarray(scale, dtype=np.float64) / dt + 0.0
    s = np.sort(np.where(kept[..., None], x, np.inf), axis=0)
    count = kept.sum(axis=0)
    m = np.broadcast_to(count[:, None], (n, 2))
    v = median_padded(s, m, axis=0)
    inside = np.arange(p).reshape(p, 1, 1) < count.reshape(1, n, 1)
    with np.errstate(all="ignore"):
        dev = np.where(inside, np.abs(s - v) + 0.0, np.inf)
        sigma = SIGMA_OF_MAD * median_padded(np.sort(dev, axis=0), m, axis=0)
    few = count < min_count
    v[few], sigma[few] = np.nan, np.nan
    return v, sigma, count.astype(np.int32)


def seconds(dt, pairs):
    if isinstance(dt, datetime.timedelta) or np.ndim(dt) == 0:
        dt = [dt] * pairs
    return np.array([v.total_seconds() if isinstance(v, datetime.timedelta) else v for v in dt], dtype=np.float64)


def velocity_field(duv, score, status, grid, dt=1.0, scale=(1.0, 1.0), min_score=0.0, accept_edge=True, radius=1,
                   min_neighbors=3, threshold=2.0, epsilon=0.1, min_count=1):
    """(v (n, 2), sigma (n, 2), count (n,) int32, kept (P, n) bool) by the rule."""
    duv, score, status = np.asarray(duv, dtype=np.float64), np.asarray(score, dtype=np.float64), np.asarray(status)
    if duv.ndim == 2:
        duv, score, status = duv[None], score[None], status[None]
    if threshold is None:
        radius = 0
    cand = candidates(duv, score, status, min_score, accept_edge)
    kept, _ = neighbour_test(duv, cand, grid, radius, min_neighbors, threshold, epsilon)
    return (*stack(duv, kept, seconds(dt, len(duv)), scale, min_count), kept)
