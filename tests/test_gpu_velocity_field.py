"""glimpse_amd.velocity_field on the device against the NumPy restatement of the rule (tests/velocity_field_rule.py): v,
sigma, count and kept, bit for bit (tobytes(), the NaN pattern included).  The shapes are small ones at which the kernels
can still go wrong: grids of one node, one row, one column and past a workgroup's tile (32 x 8 nodes) on each axis; every
number of neighbours of both radii; pair counts on both sides of every length of list and of the steps of the stack's
plan (256 / 257, 512 / 513 pairs); ties, signed zeros, magnitudes 1e300 beside 1e-300, negative scale, dt over six decades."""
import datetime

import numpy as np
import pytest

from tests import displacement_rule
from tests import velocity_field_rule as rule

pytestmark = pytest.mark.gpu

NAMES = ("v", "sigma", "count", "kept")


def field(pairs, rows, cols, seed, density=0.9, quantum=None):
    """(duv (pairs, n, 2), score, status): a smooth field with noise of 0.3 px (in steps of `quantum`, if given), of which a
    part of 1 - density is no candidate: by its status (2 .. 4, duv NaN as displacements writes them), by a score below 0
    or by a NaN score; a tenth of the rest has the status "peak on the edge", a twentieth is moved by some pixels."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    r, c = np.divmod(np.arange(n), cols)
    duv = np.column_stack([3 + 0.15 * c + 0.05 * r, -2 + 0.1 * r - 0.02 * c]) + rng.normal(0.0, 0.3, size=(pairs, n, 2))
    duv[rng.random((pairs, n)) < 0.05] += rng.uniform(-9.0, 9.0, size=2)
    if quantum:
        duv = np.rint(duv / quantum) * quantum
    score = rng.uniform(0.2, 1.0, size=(pairs, n))
    status = (rng.random((pairs, n)) < 0.1).astype(np.uint8)
    how = rng.integers(0, 5, size=(pairs, n))
    out = rng.random((pairs, n)) >= density
    for k in (2, 3, 4):
        status[out & (how == k)] = k
        duv[out & (how == k)] = np.nan
    score[out & (how == 0)] = -0.25
    score[out & (how == 1)] = np.nan
    return duv, score, status


def check(duv, score, status, grid, **kwargs):
    import glimpse_amd

    got = glimpse_amd.velocity_field(duv, score, status, grid, return_kept=True, **kwargs)
    want = rule.velocity_field(duv, score, status, grid, **kwargs)
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            rows = [np.ascontiguousarray(a).reshape(-1, a.shape[-1] if name != "count" else 1).view(np.uint8) for a in (g, w)]
            where = np.flatnonzero((rows[0] != rows[1]).any(axis=1))
            raise AssertionError(f"{name} differs at {len(where)} rows, the first {where[:10]}: "
                                 f"{g.reshape(len(rows[0]), -1)[where[:3]]} for {w.reshape(len(rows[0]), -1)[where[:3]]}")
    assert len(glimpse_amd.velocity_field(duv, score, status, grid, **kwargs)) == 3
    return want


# ---- grids ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("grid", [(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (9, 12), (5, 300), (70, 70)])
def test_grids(grid, radius):
    duv, score, status = field(3, *grid, seed=grid[0] + grid[1])
    v, sigma, count, kept = check(duv, score, status, grid, radius=radius, min_neighbors=1, dt=[1.0, 2.0, 0.5])
    if grid[0] * grid[1] > 1:
        assert kept.any()
    if min(grid) == 1 and radius == 1:
        assert rule.neighbour_test(duv, rule.candidates(duv, score, status), grid, 1)[1].max() <= 2


def test_launch_arithmetic_of_70000_nodes():
    grid = (250, 280)
    duv, score, status = field(3, *grid, seed=9)
    v, sigma, count, kept = check(duv, score, status, grid, scale=(2.0, -2.0), dt=[3600.0, 7200.0, 1800.0])
    assert set(np.unique(count)) == {0, 1, 2, 3} and kept.mean() > 0.5


# ---- neighbour counts ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2])
def test_every_number_of_neighbours(radius):
    """Candidate densities of 0.1, 0.5 and 0.9 on a 30 x 31 grid: over the cases a candidate meets every number of
    neighbours there is, 0 .. 8 or 0 .. 24, so every select of the median's pick is taken."""
    grid, seen = (30, 31), set()
    for density in (0.1, 0.5, 0.9):
        duv, score, status = field(4, *grid, seed=int(10 * density) + radius, density=density)
        cand = rule.candidates(duv, score, status)
        seen |= set(rule.neighbour_test(duv, cand, grid, radius)[1][cand].tolist())
        check(duv, score, status, grid, radius=radius, min_neighbors=1)
    assert seen == set(range((2 * radius + 1) ** 2))


@pytest.mark.parametrize("radius,min_neighbors", [(1, 1), (1, 3), (1, 8), (2, 1), (2, 3), (2, 8), (2, 24)])
def test_min_neighbors(radius, min_neighbors):
    grid, below, kept_some = (11, 13), False, False
    for density in (0.05, 0.35, 0.97):
        duv, score, status = field(3, *grid, seed=17, density=density)
        cand = rule.candidates(duv, score, status)
        number = rule.neighbour_test(duv, cand, grid, radius)[1][cand]
        *_, kept = check(duv, score, status, grid, radius=radius, min_neighbors=min_neighbors, threshold=3.0)
        below, kept_some = below or (number < min_neighbors).any(), kept_some or kept.any()
    assert below and kept_some  # (the bound refuses some candidates and lets others through)


def test_candidates_options():
    grid = (9, 12)
    duv, score, status = field(5, *grid, seed=23, density=0.7)
    for kwargs in (dict(accept_edge=False), dict(min_score=0.6), dict(threshold=None), dict(radius=0),
                   dict(epsilon=0.5, threshold=1.0), dict(min_count=3)):
        check(duv, score, status, grid, **kwargs)
    one = check(duv[0], score[0], status[0], grid)  # a single pair without the leading axis
    assert one[3].shape == (1, 108) and (one[1][one[2] == 1] == 0).all()
    check(duv, score, status.astype(np.int64), grid)


# ---- pair counts ---------------------------------------------------------------------------------------------------------

def pairs_case(pairs, seed):
    """A 5 x 7 grid of which node 0 keeps no pair, node 1 one, node 2 two (of two or more) and node 3 all; the others keep
    each pair with a probability of their own."""
    rng = np.random.default_rng(seed)
    duv, score, status = field(pairs, 5, 7, seed=seed, density=1.0)
    keep = rng.random((pairs, 35)) < rng.random(35)
    keep[:, 0], keep[:, 1], keep[:, 2], keep[:, 3] = False, False, False, True
    keep[rng.integers(pairs), 1] = True
    keep[rng.permutation(pairs)[:2], 2] = True
    status[~keep] = 4
    duv[~keep] = np.nan
    return duv, score, status


@pytest.mark.parametrize("pairs", [1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024])
def test_pair_counts(pairs):
    duv, score, status = pairs_case(pairs, seed=pairs)
    dt = np.logspace(0.0, 6.0, pairs) * np.where(np.arange(pairs) % 5 == 4, -1.0, 1.0)  # 1 s .. 10^6 s, some backwards
    v, sigma, count, kept = check(duv, score, status, (5, 7), radius=0, dt=dt, scale=(0.5, -0.5))
    counts = set(count.tolist())
    assert {0, 1, min(2, pairs), pairs} <= counts
    if pairs > 4:
        assert any(c > 2 and c % 2 for c in counts) and any(c > 2 and c % 2 == 0 for c in counts)
    assert np.isnan(v[0]).all() and np.isnan(sigma[0]).all() and (sigma[1] == 0).all() and not np.isnan(v[1:4]).any()


@pytest.mark.parametrize("pairs", [512, 513])
def test_pair_counts_where_the_run_of_nodes_halves(pairs):
    """Beside 256 / 257 above: the other number of pairs from which a workgroup takes half as many nodes."""
    test_pair_counts(pairs)


def test_every_pair_kept_at_1024():
    duv, score, status = field(1024, 5, 7, seed=3, density=1.0)
    v, sigma, count, kept = check(duv, score, status, (5, 7), radius=0)
    assert (count == 1024).all() and kept.all() and (sigma > 0).all()


def test_min_count_above_some_counts():
    duv, score, status = pairs_case(33, seed=5)
    v, sigma, count, kept = check(duv, score, status, (5, 7), radius=0, min_count=12)
    few = count < 12
    assert few.any() and (~few).any() and np.isnan(v[few]).all() and not np.isnan(v[~few]).any()


# ---- values --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2])
def test_ties(radius):
    """duv in steps of 0.25 px: the medians meet ties, and the residual is exactly 0 at some nodes."""
    grid = (12, 14)
    duv, score, status = field(6, *grid, seed=31, quantum=0.25)
    duv[:, :, 1] = np.rint(duv[:, :, 1])  # (whole pixels: most neighbours agree)
    cand = rule.candidates(duv, score, status)
    padded = np.where(cand[..., None], duv, np.inf).reshape(6, *grid, 2)
    flat = padded[:, :, 1:] == padded[:, :, :-1]
    assert flat[np.isfinite(padded[:, :, 1:])].mean() > 0.2
    check(duv, score, status, grid, radius=radius)
    check(np.rint(duv), score, status, grid, radius=radius, epsilon=0.01)


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_signed_zeros(radius):
    """Fields of -0.0 and +0.0 mixed with a few small values: the median of many nodes is a zero, of either sign going
    in, and +0.0 coming out."""
    rng = np.random.default_rng(37)
    grid, pairs = (9, 10), 5
    duv = rng.choice([-0.0, 0.0, 0.0, -0.0, 0.25, -0.25], size=(pairs, 90, 2))
    score, status = np.full((pairs, 90), 0.9), np.zeros((pairs, 90), dtype=np.uint8)
    assert np.signbit(duv[duv == 0]).any() and not np.signbit(duv[duv == 0]).all()
    v, sigma, count, kept = check(duv, score, status, grid, radius=radius, dt=[1.0, -1.0, 2.0, -2.0, 1.0], scale=(1.0, -1.0))
    assert (v == 0).any() and not np.signbit(v[v == 0]).any() and not np.signbit(sigma[sigma == 0]).any()


def test_magnitudes():
    """1e300 beside 1e-300: the sum of an even median must not overflow where NumPy's does not, and the small values must
    not be lost."""
    rng = np.random.default_rng(41)
    grid, pairs = (8, 9), 4
    duv = rng.choice([1e300, 1e-300, -1e300, -1e-300], size=(pairs, 72, 2)) * rng.uniform(1.0, 2.0, size=(pairs, 72, 2))
    score, status = np.full((pairs, 72), 0.9), np.zeros((pairs, 72), dtype=np.uint8)
    for radius in (0, 1, 2):
        v, sigma, count, kept = check(duv, score, status, grid, radius=radius, threshold=1e3)
        assert np.isfinite(v[count > 0]).all()
    assert (np.abs(v) > 1e299).any() and (np.abs(v) < 1e-299).any()


def test_scale_and_dt():
    grid = (9, 12)
    duv, score, status = field(6, *grid, seed=43)
    dt = [1.0, 1e6, 33.0, 86400.0, 1e3, 7.0]
    check(duv, score, status, grid, dt=dt, scale=(10.0, -10.0))
    check(duv, score, status, grid, dt=[datetime.timedelta(seconds=s) for s in dt], scale=(0.1, -3.0))
    check(duv, score, status, grid, dt=datetime.timedelta(days=2))


def test_times():
    from glimpse_amd import _lib

    duv, score, status = field(3, 9, 12, seed=47)
    *out, times = _lib.stage_velocity_field(duv, score, status, (9, 12), np.ones(3), (1.0, 1.0), 0.0, True, 1, 3, 2.0, 0.1, 1,
                                            return_times=True)
    assert tuple(times) == _lib.VELOCITY_FIELD_TIMES and all(t >= 0 for t in times.values())
    want = rule.velocity_field(duv, score, status, (9, 12))
    assert all(g.tobytes() == w.tobytes() for g, w in zip(out, want))


def test_library_refusals():
    from glimpse_amd import _lib

    duv, score, status = field(2, 3, 4, seed=1)
    args = dict(grid=(3, 4), dt=np.ones(2), scale=(1.0, 1.0), min_score=0.0, accept_edge=True, radius=1, min_neighbors=3,
                threshold=2.0, epsilon=0.1, min_count=1)
    # (-1: GLH_E_INVALID, -5: GLH_E_UNSUPPORTED)
    for change, code in ((dict(grid=(3, 5)), -1), (dict(radius=3), -5), (dict(min_neighbors=9), -1), (dict(threshold=0.0), -1),
                         (dict(epsilon=np.inf), -1), (dict(min_count=0), -1), (dict(dt=np.array([1.0, 0.0])), -1),
                         (dict(scale=(np.nan, 1.0)), -1)):
        with pytest.raises(_lib.GlhError) as error:
            _lib.stage_velocity_field(duv, score, status, **{**args, **change})
        assert error.value.code == code, change


# ---- the chain -----------------------------------------------------------------------------------------------------------

def test_observer_velocity_field():
    """Four noise frames of 97 x 61 pixels a day apart, a 6 x 9 grid of points: Observer.velocity_field equals the rule's
    velocity field of the rule's displacements of the same frames."""
    from glimpse_amd import Image, Observer

    a = displacement_rule.noise_u8((61, 97), seed=11)
    arrays = [a, displacement_rule.shifted(a, 1, 0, seed=31), displacement_rule.shifted(a, 1, 2, seed=32),
              displacement_rule.shifted(a, -1, 3, seed=33)]
    t0 = datetime.datetime(2020, 1, 1)
    obs = Observer([Image(cam={"imgsz": (97, 61), "f": (100, 100)}, array=f, datetime=t0 + datetime.timedelta(days=k))
                    for k, f in enumerate(arrays)])
    grid = (6, 9)
    u, v = np.meshgrid(np.linspace(8.0, 88.0, 9), np.linspace(7.0, 53.0, 6))
    uv = np.column_stack([u.ravel(), v.ravel()])
    match = dict(size=(9, 9), reach=(4, 3))
    for step, kwargs in ((1, dict()), (2, dict(radius=2, min_neighbors=4)), (1, dict(scale=(2.0, -2.0), min_count=2))):
        got = obs.velocity_field(uv, grid, step=step, displacements=match, return_kept=True, **kwargs)
        pairs = [displacement_rule.displacements(arrays[k], arrays[k + step], uv, **match)[:3] for k in range(4 - step)]
        duv, score, status = (np.stack(x) for x in zip(*pairs))
        want = rule.velocity_field(duv, score, status, grid, dt=86400.0 * step, **kwargs)
        for name, g, w in zip(NAMES, got, want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name
        assert want[3].any()
