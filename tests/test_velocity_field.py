"""`glimpse_amd.velocity_field` on the CPU: the NumPy restatement of the rule (tests/velocity_field_rule.py) -- its medians,
every branch of the rule from an input built for it, and that it does what it is for on a synthetic field --, the
refusals of the public function, made before the library is loaded, and the sorting networks of the neighbour test
(glimpse_amd/csrc/glh_sort_networks.h), proven with the 0/1 principle.  The device against the restatement is
tests/test_gpu_velocity_field.py."""
import datetime
import os
import re

import numpy as np
import pytest

from tests import velocity_field_rule as rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the medians ---------------------------------------------------------------------------------------------------------

def test_medians_equal_numpy_median_in_every_bit():
    rng = np.random.default_rng(3)
    for m in range(1, 26):
        for trial in range(40):
            x = rng.normal(size=m) if trial % 2 else rng.integers(-3, 4, size=m) * 0.25  # (duplicates)
            for width in (m, 32):
                s = np.sort(np.concatenate([x, np.full(width - m, np.inf)]))
                assert rule.median_padded(s, m).tobytes() == np.float64(np.median(x)).tobytes()
    s = np.sort(rng.normal(size=(5, 7, 25)), axis=0)
    got = rule.median_padded(s, np.full((7, 25), 5), axis=0)
    assert got.tobytes() == np.median(s, axis=0).tobytes()
    assert np.isnan(rule.median_padded(np.full(8, np.inf), 0))


# ---- statuses and branches -----------------------------------------------------------------------------------------------

def uniform(p, rows, cols, value=(1.0, -2.0)):
    n = rows * cols
    duv = np.tile(np.array(value, dtype=np.float64), (p, n, 1))
    return duv, np.full((p, n), 0.9), np.zeros((p, n), dtype=np.uint8)


def test_each_status():
    duv, score, status = uniform(1, 3, 5)
    status[0, :5] = [0, 1, 2, 3, 4]
    duv[0, 2:5] = np.nan  # (what displacements writes with the statuses 2 .. 4)
    assert rule.candidates(duv, score, status)[0, :6].tolist() == [True, True, False, False, False, True]
    assert rule.candidates(duv, score, status, accept_edge=False)[0, :6].tolist() == [True, False, False, False, False, True]
    *_, kept = rule.velocity_field(duv, score, status, (3, 5), radius=0)
    assert kept[0, :6].tolist() == [True, True, False, False, False, True]
    duv[0, 2:5] = 1.0  # (the status alone refuses them)
    assert rule.candidates(duv, score, status)[0, :6].tolist() == [True, True, False, False, False, True]


def test_min_score_and_nan():
    duv, score, status = uniform(1, 3, 5)
    score[0, :4] = [0.5, 0.49, np.nan, -1.0]
    duv[0, 6, 1], duv[0, 7, 0] = np.nan, np.inf
    cand = rule.candidates(duv, score, status, min_score=0.5)
    assert cand[0, :4].tolist() == [True, False, False, False] and not cand[0, 6] and not cand[0, 7] and cand[0, 8:].all()
    assert rule.candidates(duv, score, status, min_score=-1.0)[0, :4].tolist() == [True, True, False, True]
    v, sigma, count, kept = rule.velocity_field(duv, score, status, (3, 5), min_score=0.5, threshold=None)
    assert np.array_equal(kept, cand) and np.array_equal(count, cand[0].astype(np.int32))
    assert np.isnan(v[~cand[0]]).all() and np.isnan(sigma[~cand[0]]).all() and (sigma[cand[0]] == 0).all()


def test_min_neighbors_and_borders():
    """A 3 x 3 grid where every node is a candidate: a corner has 3 neighbours, an edge 5, the centre 8 -- no wrap, no
    reflection."""
    duv, score, status = uniform(1, 3, 3)
    cand = rule.candidates(duv, score, status)
    _, number = rule.neighbour_test(duv, cand, (3, 3))
    assert number.reshape(3, 3).tolist() == [[3, 5, 3], [5, 8, 5], [3, 5, 3]]
    for least, want in ((3, 9), (4, 5), (6, 1), (8, 1)):
        kept, _ = rule.neighbour_test(duv, cand, (3, 3), min_neighbors=least)
        assert kept.sum() == want
    _, number = rule.neighbour_test(duv, cand, (3, 3), radius=2)
    assert (number == 8).all()
    # an isolated vector cannot be vouched for
    status[0, [1, 3, 4]] = 4
    kept, number = rule.neighbour_test(duv, rule.candidates(duv, score, status), (3, 3), min_neighbors=1)
    assert number[0, 0] == 0 and not kept[0, 0] and kept[0, 8]


def test_threshold_epsilon_and_none():
    duv, score, status = uniform(1, 5, 5)
    duv[0, 12] = [1.0 + 0.25, -2.0]  # res is exactly 0: |x - med| / epsilon
    cand = rule.candidates(duv, score, status)
    assert not rule.neighbour_test(duv, cand, (5, 5))[0][0, 12]                 # 0.25 / 0.1 > 2
    assert rule.neighbour_test(duv, cand, (5, 5), epsilon=0.125)[0][0, 12]      # 0.25 / 0.125 <= 2
    assert rule.neighbour_test(duv, cand, (5, 5), threshold=2.5)[0][0, 12]
    duv[0, 12] = [1.0, -2.0 - 0.25]  # the other component refuses as well
    assert not rule.neighbour_test(duv, cand, (5, 5))[0][0, 12]
    *_, kept = rule.velocity_field(duv, score, status, (5, 5), threshold=None)
    assert kept.all()
    *_, kept = rule.velocity_field(duv, score, status, (5, 5), radius=0)
    assert kept.all()


def test_stack_min_count_scale_and_dt():
    duv = np.array([[[2.0, 4.0]], [[4.0, -8.0]], [[9.0, 1.0]], [[100.0, 100.0]]])  # (4 pairs, 1 node)
    kept = np.array([[True], [True], [True], [False]])
    v, sigma, count = rule.stack(duv, kept, [1.0, 2.0, 3.0, 1.0], scale=(1.0, -0.5))
    assert count.tolist() == [3] and count.dtype == np.int32
    assert v.tolist() == [[2.0, -0.5 / 3.0]]  # x = (2, 2, 3) and (-2, 2, -1/6)
    assert sigma[0, 0] == 0.0 and sigma[0, 1] == 1.4826 * np.abs(-2.0 - -0.5 / 3.0)
    v, sigma, count = rule.stack(duv, kept, [1.0] * 4, min_count=4)
    assert count.tolist() == [3] and np.isnan(v).all() and np.isnan(sigma).all()
    v, sigma, count = rule.stack(duv[:2], kept[:2], [1.0, 1.0])  # an even count: the mean of the middle two
    assert v.tolist() == [[3.0, -2.0]] and sigma.tolist() == [[1.4826 * 1.0, 1.4826 * 6.0]]
    v, sigma, count = rule.stack(duv[:1], kept[:1], [1.0])  # one pair: no spread
    assert v.tolist() == [[2.0, 4.0]] and sigma.tolist() == [[0.0, 0.0]]


def test_negative_zero_never_reaches_a_result():
    duv = np.array([[[-0.0, 0.0]], [[0.0, -0.0]], [[-0.0, -0.0]]])
    v, sigma, _ = rule.stack(duv, np.ones((3, 1), dtype=bool), [1.0, -1.0, 1.0])
    assert not np.signbit(v).any() and not np.signbit(sigma).any() and (v == 0).all() and (sigma == 0).all()


def test_timedeltas_equal_their_seconds():
    duv, score, status = sense_field()[:3]
    dt = [datetime.timedelta(days=1 + k, seconds=17 * k, microseconds=250000 * k) for k in range(len(duv))]
    a = rule.velocity_field(duv, score, status, SENSE_GRID, dt=dt)
    b = rule.velocity_field(duv, score, status, SENSE_GRID, dt=[v.total_seconds() for v in dt])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    one = rule.velocity_field(duv, score, status, SENSE_GRID, dt=datetime.timedelta(hours=6))
    assert one[0].tobytes() == rule.velocity_field(duv, score, status, SENSE_GRID, dt=21600.0)[0].tobytes()
    from glimpse_amd import velocity

    assert velocity.seconds(dt, len(dt)).tobytes() == rule.seconds(dt, len(dt)).tobytes()
    assert velocity.seconds(datetime.timedelta(hours=6), 3).tolist() == [21600.0] * 3


# ---- refusals ------------------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_library(monkeypatch):
    import glimpse_amd
    from glimpse_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    duv, score, status = uniform(2, 3, 4)
    good = dict(grid=(3, 4))
    bad = [
        dict(grid=(3, 5)), dict(grid=(4, 4)), dict(grid=(12,)),
        dict(radius=3), dict(radius=-1),
        dict(min_neighbors=0), dict(min_neighbors=9), dict(radius=2, min_neighbors=25),
        dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.inf), dict(threshold=np.nan),
        dict(epsilon=0.0), dict(epsilon=-0.1), dict(epsilon=np.inf), dict(epsilon=np.nan),
        dict(min_count=0),
        dict(dt=0.0), dict(dt=np.inf), dict(dt=np.nan), dict(dt=[1.0, 0.0]), dict(dt=[1.0, 2.0, 3.0]),
        dict(dt=datetime.timedelta(0)),
        dict(scale=(1.0,)), dict(scale=(1.0, np.nan)), dict(scale=(np.inf, 1.0)), dict(scale=2.0),
    ]
    for kwargs in bad:
        with pytest.raises(ValueError):
            glimpse_amd.velocity_field(duv, score, status, **{**good, **kwargs})
    for d, s, t in ((duv[:, :11], score, status), (duv, score[:, :11], status), (duv, score, status[:1]),
                    (duv[..., :1], score, status), (duv[0], score, status), (duv, score, status.astype(np.float64))):
        with pytest.raises(ValueError):
            glimpse_amd.velocity_field(d, s, t, (3, 4))
    many = uniform(1025, 1, 1)
    with pytest.raises(ValueError):
        glimpse_amd.velocity_field(*many, (1, 1))
    with pytest.raises(ValueError):
        glimpse_amd.velocity_field(duv[:0], score[:0], status[:0], (3, 4))
    # an empty n returns empty arrays without a library call
    v, sigma, count, kept = glimpse_amd.velocity_field(duv[:, :0], score[:, :0], status[:, :0], (0, 7), return_kept=True)
    assert v.shape == (0, 2) and sigma.shape == (0, 2) and count.shape == (0,) and count.dtype == np.int32
    assert kept.shape == (2, 0) and kept.dtype == bool
    assert len(glimpse_amd.velocity_field(duv[0, :0], score[0, :0], status[0, :0], (0, 0))) == 3
    # what is accepted reaches the library
    for kwargs in (dict(), dict(threshold=None, min_neighbors=99), dict(radius=0, min_neighbors=0), dict(radius=2, min_neighbors=24),
                   dict(dt=[datetime.timedelta(seconds=1), 2.0]), dict(scale=(2.0, -2.0))):
        with pytest.raises(AssertionError, match="the library was loaded"):
            glimpse_amd.velocity_field(duv, score, status, **{**good, **kwargs})
    with pytest.raises(AssertionError, match="the library was loaded"):
        glimpse_amd.velocity_field(duv[0], score[0], status[0], (3, 4))


# ---- sense ---------------------------------------------------------------------------------------------------------------

SENSE_GRID = (9, 12)


def sense_field():
    """(duv (7, 108, 2), score, status, truth (108, 2), moved (7, 108) bool, off (7, 108) bool): a smooth field with noise
    of 0.05 px; per pair 8 nodes are no candidates and 10 others are moved by +-(4 .. 12) px on both components."""
    rng = np.random.default_rng(5)
    rows, cols = SENSE_GRID
    n, pairs = rows * cols, 7
    r, c = np.divmod(np.arange(n), cols)
    truth = np.column_stack([3 + 0.15 * c + 0.05 * r, -2 + 0.1 * r - 0.02 * c])
    duv = truth + rng.normal(0.0, 0.05, size=(pairs, n, 2))
    score, status = np.full((pairs, n), 0.9), np.zeros((pairs, n), dtype=np.uint8)
    moved, off = np.zeros((pairs, n), dtype=bool), np.zeros((pairs, n), dtype=bool)
    for p in range(pairs):
        pick = rng.permutation(n)[:18]
        off[p, pick[:8]], moved[p, pick[8:]] = True, True
        status[p, pick[:4]], score[p, pick[4:8]] = 4, -0.5
        duv[p, pick[:4]] = np.nan
        duv[p, pick[8:]] += rng.choice([-1.0, 1.0], size=(10, 2)) * rng.uniform(4.0, 12.0, size=(10, 2))
    return duv, score, status, truth, moved, off


def test_sense():
    """With the defaults every one of the 70 moved vectors is rejected and at least 95 % of the other candidates are kept:
    this restatement keeps 621 of the 630 (SENSE_KEPT, asserted, so that a change of the restatement shows); the
    stacked v lies within 0.1 px of the noise-free field at every node with a count of 4 or more."""
    duv, score, status, truth, moved, off = sense_field()
    v, sigma, count, kept = rule.velocity_field(duv, score, status, SENSE_GRID)
    assert moved.sum() == 70 and off.sum() == 56 and not kept[moved].any() and not kept[off].any()
    others = ~moved & ~off
    print("kept", kept[others].sum(), "of", others.sum())
    assert others.sum() == 630 and kept[others].sum() >= 0.95 * 630
    assert kept[others].sum() == SENSE_KEPT
    well = count >= 4
    assert well.sum() > 100 and np.abs(v[well] - truth[well]).max() < 0.1
    assert (sigma[well] < 0.2).all() and np.array_equal(count, kept.sum(axis=0))


SENSE_KEPT = 621


# ---- the networks --------------------------------------------------------------------------------------------------------

def network(name):
    src = open(os.path.join(ROOT, "glimpse_amd", "csrc", "glh_sort_networks.h")).read()
    body = src[src.index("#define " + name + "(X)"):]
    end = re.search(r"[^\\]\n", body).end()  # the macro ends at the first line without a continuation
    return [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),(\d+)\)", body[:end])]


@pytest.mark.parametrize("wires", [8, 24])
def test_networks_sort_every_binary_input(wires):
    """0/1 principle: a comparator network sorts every input iff it sorts every binary input.  All 2^wires of them run
    bit-parallel, 64 to a word, in chunks of 2^20 inputs."""
    pairs = network(f"GLH_SORT{wires}_NETWORK")
    assert pairs and all(0 <= a < b < wires for a, b in pairs)
    assert {w for pair in pairs for w in pair} == set(range(wires))
    total, chunk = 1 << wires, 1 << min(wires, 20)
    for start in range(0, total, chunk):
        idx = np.arange(start, start + chunk, dtype=np.uint32)
        w = [np.packbits(((idx >> k) & 1).astype(np.uint8), bitorder="little") for k in range(wires)]
        ones = sum(((idx >> k) & 1).astype(np.uint8) for k in range(wires))
        for a, b in pairs:
            w[a], w[b] = w[a] & w[b], w[a] | w[b]
        # sorted ascending with as many ones as went in: wire k is 1 exactly when k >= wires - ones
        for k in range(wires):
            want = np.packbits((ones >= wires - k).astype(np.uint8), bitorder="little")
            assert np.array_equal(w[k], want), (wires, k, start)
