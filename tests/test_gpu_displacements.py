"""glimpse_amd.displacements on the device against the NumPy restatement of the rule (tests/displacement_rule.py): duv,
score, status and the whole score surface, bit for bit (tobytes(), the NaN pattern included), on both paths.  The frame is
97 x 61 pixels (a width that is no multiple of 4); the points put template boxes flush with every edge and corner and
let the left edge of the boxes take all four values modulo 4."""
import datetime

import numpy as np
import pytest

from tests import displacement_rule as rule

pytestmark = pytest.mark.gpu

SMALL = (61, 97)    # rows, cols
LARGE = (130, 160)  # for 63 x 63 templates


def frames_u8(shape):
    a = rule.noise_u8(shape, seed=11)
    b = rule.shifted(a, 2, -1, seed=12)
    b[::7, ::5] ^= 3  # (not an exact copy: scores below 1, surfaces without exact ties)
    return a, b


def points(shape, size):
    uv = rule.edge_points(shape, size)
    lefts = {int(np.floor(u - size[0] / 2 + 0.5)) % 4 for u, _ in uv}
    assert lefts == {0, 1, 2, 3}
    return uv


def same(got, want):
    names = ("duv", "score", "status", "surface")
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            rows = [np.ascontiguousarray(v).view(np.uint8).reshape(len(v), -1) for v in (g, w)]
            raise AssertionError(f"{name} differs at points {np.flatnonzero((rows[0] != rows[1]).any(axis=1))[:20]}")


def check(a, b, uv, size, reach, guess=None, subpixel=True):
    import glimpse_amd

    got = glimpse_amd.displacements(a, b, uv, size=size, reach=reach, guess=guess, subpixel=subpixel, return_surface=True)
    want = rule.displacements(a, b, uv, size=size, reach=reach, guess=guess, subpixel=subpixel)
    same(got, want)
    return got


SHAPES = [((3, 3), (1, 1)), ((5, 4), (2, 5)), ((15, 15), (16, 16)), ((16, 16), (2, 5)), ((31, 31), (16, 16)),
          ((15, 15), (32, 32)), ((31, 31), (1, 1)), ((16, 16), (32, 32))]


@pytest.mark.parametrize("size,reach", SHAPES)
def test_integer_path(size, reach):
    a, b = frames_u8(SMALL)
    uv = points(SMALL, size)
    *_, status, _ = check(a, b, uv, size, reach)
    assert set(status) <= {rule.MATCHED, rule.EDGE}


@pytest.mark.parametrize("reach", [(1, 1), (16, 16), (32, 32)])
def test_integer_path_63(reach):
    a, b = frames_u8(LARGE)
    uv = points(LARGE, (63, 63))
    check(a, b, uv if reach[0] < 32 else uv[::3], (63, 63), reach)  # (the restatement of the full reach takes its time)


def guesses(n):
    """Guesses that keep the range inside, push part of it out, and push all of it out of the frame."""
    g = np.zeros((n, 2))
    g[0::4] = (2.4, -1.0)
    g[1::4] = (-30.0, 20.6)
    g[2::4] = (70.0, 3.0)
    g[3::4] = (-200.5, 150.0)
    return g


@pytest.mark.parametrize("size,reach", [((5, 4), (2, 5)), ((15, 15), (16, 16))])
def test_integer_path_with_guess(size, reach):
    a, b = frames_u8(SMALL)
    uv = points(SMALL, size)
    *_, status, _ = check(a, b, uv, size, reach, guess=guesses(len(uv)))
    assert rule.NO_OFFSET in status and (status < rule.NO_OFFSET).any()


def float_frames(kind, shape=SMALL):
    a, b = frames_u8(shape)
    rng = np.random.default_rng(21)
    if kind == "float32":
        return (a + rng.random(shape)).astype(np.float32), (b + rng.random(shape)).astype(np.float32)
    if kind == "uint16":
        return a.astype(np.uint16) * 256 + 3, b.astype(np.uint16) * 255 + 9
    if kind == "rgb":
        return (np.stack([a, np.roll(a, 1, 0) // 2, a[::-1] // 3], axis=2),
                np.stack([b, np.roll(b, 1, 0) // 2, b[::-1] // 3], axis=2))
    if kind == "float64":
        return a * 1.0 + rng.random(shape) * 1e-3, b * 1.0
    assert kind == "nan"
    a, b = (a + rng.random(shape)).astype(np.float32), (b + rng.random(shape)).astype(np.float32)
    a[rng.random(shape) < 0.002] = np.nan
    b[rng.random(shape) < 0.004] = np.nan
    b[5, 50] = np.inf
    return a, b


@pytest.mark.parametrize("size,reach", [((3, 3), (1, 1)), ((5, 4), (2, 5)), ((15, 15), (16, 16)), ((16, 16), (32, 32)),
                                        ((31, 31), (16, 16))])
def test_float_path(size, reach):
    a, b = float_frames("float32")
    check(a, b, points(SMALL, size), size, reach)


@pytest.mark.parametrize("kind", ["uint16", "rgb", "float64"])
def test_float_path_types(kind):
    a, b = float_frames(kind)
    n = len(points(SMALL, (9, 7)))
    check(a, b, points(SMALL, (9, 7)), (9, 7), (4, 3), guess=guesses(n))
    check(a, b, points(SMALL, (9, 7)), (9, 7), (4, 3))


def test_float_path_nan_cells():
    a, b = float_frames("nan")
    u, v = np.meshgrid(np.arange(6, 92, 6) + 0.5, np.arange(6, 56, 6) + 0.5)
    uv = np.column_stack([u.ravel(), v.ravel()])
    *_, status, surface = check(a, b, uv, (7, 7), (3, 3))
    assert rule.FLAT in status  # (templates that hold a NaN)
    valid = status < rule.NO_OFFSET
    assert (np.isnan(surface[valid]).any(axis=(1, 2)) & np.isfinite(surface[valid]).any(axis=(1, 2))).any()


def test_float_path_63_at_full_reach():
    a, b = float_frames("float32", LARGE)
    uv = np.array([[80.0, 65.0], [31.5, 31.5], [160 - 31.5, 130 - 31.5], [70.3, 60.8]])
    check(a, b, uv, (63, 63), (32, 32))


@pytest.mark.parametrize("n", [1, 2, 300])
def test_counts(n):
    a, b = frames_u8(SMALL)
    rng = np.random.default_rng(n)
    uv = np.column_stack([rng.uniform(-2, 99, n), rng.uniform(-2, 63, n)])
    uv[0] = (48.0, 30.0)
    *_, status, _ = check(a, b, uv, (9, 9), (3, 3))
    assert n < 300 or (rule.OUTSIDE in status and rule.MATCHED in status)
    fa, fb = float_frames("float32")
    check(fa, fb, uv, (9, 9), (3, 3))


@pytest.mark.parametrize("as_float", [False, True])
def test_statuses_and_subpixel_false(as_float):
    """Every status on the device; subpixel=False equals the whole-pixel part of the default call and never reports
    "peak on the edge"."""
    import glimpse_amd

    a, b = frames_u8(SMALL)
    a = a.copy()
    a[40:55, 10:25] = 9  # (a constant patch: flat templates)
    if as_float:
        a, b = a.astype(np.float32), b.astype(np.float32)
    uv = np.vstack([points(SMALL, (9, 9)), [[17.0, 47.0], [np.nan, 3.0], [96.0, 30.0]]])
    guess = np.zeros((len(uv), 2))
    guess[1] = (500.0, 0.0)  # no window inside
    guess[9] = (-1.0, 0.0)   # an interior point: the shift of 2 is found at offset 3, the border of the range
    fine = check(a, b, uv, (9, 9), (3, 3), guess=guess)
    coarse = check(a, b, uv, (9, 9), (3, 3), guess=guess, subpixel=False)
    assert set(fine[2]) == set(range(5))
    assert rule.EDGE not in coarse[2]
    ok = fine[2] < rule.NO_OFFSET
    assert (coarse[2][ok] == rule.MATCHED).all() and (coarse[2][~ok] == fine[2][~ok]).all()
    assert (coarse[0][ok] == np.rint(coarse[0][ok])).all() and (np.abs(fine[0][ok] - coarse[0][ok]) <= 0.5).all()
    assert coarse[1].tobytes() == fine[1].tobytes() and coarse[3].tobytes() == fine[3].tobytes()
    no_surface = glimpse_amd.displacements(a, b, uv, size=(9, 9), reach=(3, 3), guess=guess)
    assert len(no_surface) == 3
    same(no_surface, fine[:3])


def observer(arrays):
    from glimpse_amd import Image, Observer

    t0 = datetime.datetime(2020, 1, 1)
    rows, cols = arrays[0].shape[:2]
    return Observer([Image(cam={"imgsz": (cols, rows), "f": (100, 100)}, array=f, datetime=t0 + datetime.timedelta(days=k))
                     for k, f in enumerate(arrays)])


@pytest.mark.parametrize("as_float", [False, True])
def test_observer_and_image(as_float):
    """Three pairs over four frames (step 1), two pairs (step 2): every pair equals the two-frame call bit for bit, with
    one guess for all pairs and with one per pair; Image.displacements equals the module function."""
    import glimpse_amd

    a, _ = frames_u8(SMALL)
    arrays = [a, rule.shifted(a, 1, 0, seed=31), rule.shifted(a, 1, 2, seed=32), rule.shifted(a, -1, 3, seed=33)]
    if as_float:
        arrays = [f.astype(np.float32) for f in arrays]
    obs = observer(arrays)
    uv = points(SMALL, (9, 9))
    kwargs = dict(size=(9, 9), reach=(4, 3))
    for step in (1, 2):
        pairs = len(arrays) - step
        per_pair = np.stack([guesses(len(uv)) * (k - 1) for k in range(pairs)])
        for guess in (None, guesses(len(uv)), per_pair):
            got = obs.displacements(uv, step=step, guess=guess, return_surface=True, **kwargs)
            assert got[0].shape == (pairs, len(uv), 2) and got[3].shape == (pairs, len(uv), 7, 9)
            for k in range(pairs):
                g = guess if guess is None or np.ndim(guess) == 2 else guess[k]
                two = glimpse_amd.displacements(arrays[k], arrays[k + step], uv, guess=g, return_surface=True, **kwargs)
                same(tuple(v[k] for v in got), two)
    got = obs.displacements(uv, index=[0, 2, 3], **kwargs)
    same(tuple(v[1] for v in got), glimpse_amd.displacements(arrays[2], arrays[3], uv, **kwargs))
    same(obs.images[0].displacements(obs.images[2], uv, **kwargs), glimpse_amd.displacements(arrays[0], arrays[2], uv, **kwargs))
    truth = glimpse_amd.displacements(arrays[0], arrays[1], np.array([[48.0, 30.0]]), **kwargs)
    assert np.allclose(truth[0], [[1.0, 0.0]], atol=0.5) and truth[1][0] > 0.99
