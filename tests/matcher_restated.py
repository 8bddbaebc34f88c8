"""NumPy restatement of the descriptor search of glh_match.hip (test-only): the two distance definitions, the best-two
rule, and a brute-force stand-in for a cv2 descriptor matcher built of them.

  integer  d2 = sum_k (q_k - t_k)^2 of uint8 rows, exact; the float32 of that integer (below 2^24 for dim <= 256)
  float    float32, accumulated in element order: s = s + (q_k - t_k) * (q_k - t_k), every operation rounded
  best two for query q the train rows with the smallest keys (d2, index), lexicographic: a stable sort by d2
           (a set of one row has no second: index -1, distance inf)
"""
import collections

import numpy as np

DMatch = collections.namedtuple("DMatch", "queryIdx trainIdx distance")


def d2_integer(q, t):
    q, t = np.asarray(q), np.asarray(t)
    assert q.dtype == np.uint8 and t.dtype == np.uint8 and q.shape[1] == t.shape[1] <= 256
    q, t = q.astype(np.float64), t.astype(np.float64)  # (every term is an integer below 2^53: float64 is exact here)
    d2 = (q * q).sum(1)[:, None] + (t * t).sum(1)[None, :] - 2 * (q @ t.T)
    assert d2.max(initial=0) < 2 ** 24
    return d2.astype(np.float32)


def d2_float(q, t):
    q, t = np.asarray(q, dtype=np.float32), np.asarray(t, dtype=np.float32)
    s = np.zeros((len(q), len(t)), dtype=np.float32)
    for k in range(q.shape[1]):
        u = q[:, k][:, None] - t[:, k][None, :]
        s = s + u * u
    assert s.dtype == np.float32
    return s


def best2(d2):
    """(idx int32 (n_q, 2), d2 float32 (n_q, 2)) of the distances (n_q, n_t)."""
    d2 = np.asarray(d2, dtype=np.float32)
    order = np.argsort(d2, axis=1, kind="stable")[:, :2]
    idx = np.full((len(d2), 2), -1, dtype=np.int32)
    best = np.full((len(d2), 2), np.inf, dtype=np.float32)
    idx[:, : order.shape[1]] = order
    best[:, : order.shape[1]] = np.take_along_axis(d2, order, axis=1)
    return idx, best


def best2_by_minima(d2):
    """`best2` without the sort, for the large cases (finite distances only): np.argmin gives the first, so the lowest,
    index of the minimum; the second is the minimum of the row with that entry taken out (set to inf)."""
    d2 = np.array(d2, dtype=np.float32)
    assert np.isfinite(d2).all()
    rows = np.arange(len(d2))
    idx = np.full((len(d2), 2), -1, dtype=np.int32)
    best = np.full((len(d2), 2), np.inf, dtype=np.float32)
    idx[:, 0] = d2.argmin(axis=1)
    best[:, 0] = d2[rows, idx[:, 0]]
    if d2.shape[1] > 1:
        d2[rows, idx[:, 0]] = np.inf
        idx[:, 1] = d2.argmin(axis=1)
        best[:, 1] = d2[rows, idx[:, 1]]
    return idx, best


def knn2_large(q, t, block=8192):
    """`knn2` of uint8 sets, `block` queries at a time."""
    parts = [best2_by_minima(d2_integer(q[a:a + block], t)) for a in range(0, len(q), block)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def knn2(q, t, path=None):
    """What _lib.Matcher.knn2 returns for the sets q and t (`path` as _lib.Matcher.put's)."""
    q, t = np.asarray(q), np.asarray(t)
    if path is None and q.dtype == np.uint8 and t.dtype == np.uint8:
        return best2(d2_integer(q, t))
    return best2(d2_float(q, t))


class BruteForceMatcher:
    """The stand-in for a cv2.DescriptorMatcher: knnMatch by the rule above, the distance np.sqrt of the float32 squared
    distance as a Python float."""

    def __init__(self, path=None):
        self.path = path

    def knnMatch(self, query, train, k=1, mask=None):
        assert mask is None
        idx, d2 = knn2(query, train, self.path)
        distance = np.sqrt(d2).tolist()
        idx = idx.tolist()
        return [[DMatch(q, idx[q][r], distance[q][r]) for r in range(k)] for q in range(len(idx))]
