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


# ---- ties, every width, height and reach, pixel-value extremes, launch limits ------------------------------------------
# The scenes are tests/displacement_rule.py's; tests/test_displacements.py asserts on the CPU what makes each meaningful.

def periodic_guess(n):
    from tests.test_displacements import periodic_guess as guess

    return guess(n)


@pytest.mark.parametrize("with_guess", [False, True])
@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("scene", ["periodic_u8", "half_striped_u8"])
def test_ties_go_to_the_first_offset(scene, as_float, subpixel, with_guess):
    """A periodic frame against itself: 12 to 35 offsets of every point share the largest score, across the waves and
    the strides of a workgroup; a half striped one: the peak's neighbour is among them, and the sub-pixel term is formed
    from it.  Beside the restatement's bytes: the peak's score is exactly 1, and without the sub-pixel term duv is the
    smallest tied offset of the surface the device itself returned."""
    frame = getattr(rule, scene)(SMALL)
    frame = frame.astype(np.float32) if as_float else frame
    uv = points(SMALL, (9, 9))
    guess = periodic_guess(len(uv)) if with_guess else None
    duv, score, status, surface = check(frame, frame, uv, (9, 9), (16, 16), guess=guess, subpixel=subpixel)
    assert (score == 1.0).all()
    ties = rule.tied(surface)
    assert all(len(t) >= 2 for t in ties)
    if not subpixel:
        first = np.array([[int(t[0]) % 33 - 16, int(t[0]) // 33 - 16] for t in ties], dtype=np.float64)
        assert (duv == first + (guess if with_guess else 0.0)).all()
    elif not with_guess:
        assert rule.MATCHED in status and rule.EDGE in status


def test_exact_copy_scores_one():
    a = rule.noise_u8(SMALL, seed=11)
    b = rule.shifted(a, 3, -2, seed=12)
    uv = points(SMALL, (15, 15))
    duv, score, status, _ = check(a, b, uv, (15, 15), (4, 4))
    inner = slice(8, 13)  # (edge_points: the five points inside)
    assert (score[inner] == 1.0).all() and (status[inner] == rule.MATCHED).all()
    assert (np.rint(duv[inner]) == (3.0, -2.0)).all()
    coarse, *_ = check(a, b, uv, (15, 15), (4, 4), subpixel=False)
    assert (coarse[inner] == (3.0, -2.0)).all()


ALL_SIDES, ALL_REACHES = range(3, 64), range(1, 33)
SWEEP_REACHES = [1, 5, 7, 8, 15, 16, 17, 31, 32]
SWEEP_WIDTHS = [3, 16, 17, 32, 33, 48, 49, 63]  # either side of the steps of the template's pitch
TALL = (97, 61)


def sweep(a, b, sizes_and_reaches):
    for size, reach in sizes_and_reaches:
        try:
            *_, status, _ = check(a, b, points(a.shape, size), size, reach)
        except AssertionError as error:
            raise AssertionError(f"size {size}, reach {reach}: {error}") from None
        assert (status < rule.NO_OFFSET).all(), (size, reach)


@pytest.mark.parametrize("rx", SWEEP_REACHES)
def test_integer_path_every_width(rx):
    """h = 3, ry = 1: every template width against reaches either side of the window pitch's classes."""
    sweep(*frames_u8(SMALL), [((w, 3), (rx, 1)) for w in ALL_SIDES])


@pytest.mark.parametrize("w", SWEEP_WIDTHS)
def test_integer_path_every_reach(w):
    sweep(*frames_u8(SMALL), [((w, 3), (rx, 1)) for rx in ALL_REACHES])


@pytest.mark.parametrize("ry", [1, 5, 16, 32])
def test_integer_path_every_height(ry):
    """w = 4, rx = 1: every segment length of the running sums along the rows and down the columns."""
    sweep(*frames_u8(TALL), [((4, h), (1, ry)) for h in ALL_SIDES])


@pytest.mark.parametrize("h", [3, 31, 63])
def test_integer_path_every_vertical_reach(h):
    sweep(*frames_u8(TALL), [((4, h), (1, ry)) for ry in ALL_REACHES])


@pytest.mark.parametrize("rx", SWEEP_REACHES)
def test_float_path_every_width(rx):
    sweep(*float_frames("float32"), [((w, 3), (rx, 1)) for w in ALL_SIDES])


@pytest.mark.parametrize("w", SWEEP_WIDTHS)
def test_float_path_every_reach(w):
    sweep(*float_frames("float32"), [((w, 3), (rx, 1)) for rx in ALL_REACHES])


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("size,reach", [((63, 3), (1, 32)), ((3, 63), (32, 1))])
def test_long_thin_templates(size, reach, as_float):
    """195 offsets in one long row or column of them: a workgroup's threads, and the float path's 1024 offsets a pass,
    stride exactly once (test_float_path_63_at_full_reach: more than once)."""
    shape = TALL if size[1] == 63 else SMALL
    sweep(*(float_frames("float32", shape) if as_float else frames_u8(shape)), [(size, reach)])


SATURATED_POINTS = np.array([[80.0, 65.0], [31.5, 31.5], [160 - 31.5, 130 - 31.5], [70.3, 60.8]])


@pytest.mark.parametrize("scene", ["saturated_u8", "holes_u8"])
def test_integer_path_at_the_largest_sums(scene):
    """63 x 63 templates of 254 / 255, and of 255 with single pixels of 0, at the full reach: sum(S^2) of 2^27.9 in the
    32-bit sums, and variances that are a small part of them."""
    a, b = getattr(rule, scene)(LARGE)
    duv, score, status, _ = check(a, b, SATURATED_POINTS, (63, 63), (32, 32))
    assert (status < rule.NO_OFFSET).all()
    assert status[0] == rule.MATCHED and tuple(np.rint(duv[0])) == rule.SATURATED_SHIFT and score[0] == 1.0


@pytest.mark.parametrize("scene", ["subnormal_f32", "huge_f32"])
def test_float_path_at_the_ends_of_float32(scene):
    """Frames of float32 subnormals (a flushed conversion would report "flat template") and of pixels up to 2.4e38."""
    a, b = getattr(rule, scene)(SMALL)
    duv, score, status, _ = check(a, b, points(SMALL, (9, 9)), (9, 9), (3, 3))
    assert set(status) == {rule.MATCHED, rule.EDGE}
    assert status[8] == rule.MATCHED and tuple(np.rint(duv[8])) == rule.SUBNORMAL_SHIFT


@pytest.mark.parametrize("as_float", [False, True])
def test_more_points_than_65535(as_float):
    """70 000 points, the 13 of edge_points over and over: every block of 13 is the restatement of the first."""
    import glimpse_amd

    a, b = float_frames("float32") if as_float else frames_u8(SMALL)
    uv = points(SMALL, (9, 9))
    copies = -(-70000 // len(uv))
    many = np.tile(uv, (copies, 1))[:70000]
    got = glimpse_amd.displacements(a, b, many, size=(9, 9), reach=(3, 3))
    want = rule.displacements(a, b, uv, size=(9, 9), reach=(3, 3))[:3]
    same(got, tuple(np.concatenate([v] * copies)[:70000] for v in want))


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("wide", [True, False])
def test_frames_at_the_largest_side(wide, as_float):
    """9 x 32768 and 32768 x 9 pixels: boxes flush with the far edge and corner, a far fractional position, and a guess
    that pushes a far point's range out of the frame."""
    shape = (9, 32768) if wide else (32768, 9)
    rng = np.random.default_rng(41)
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    b = rule.moved(a, *((3, 1) if wide else (1, 3)), rng.integers(0, 256, size=shape, dtype=np.uint8))
    if as_float:
        a, b = a.astype(np.float32) + np.float32(0.25), b.astype(np.float32)
    size, reach = ((9, 7), (4, 1)) if wide else ((7, 9), (1, 4))
    far = 32768.0
    along = [far - 4.5, far - 20.3, far - 40.0, far - 9.0, 16000.5, 4.5]  # (the side of 9 lies along the frame)
    across = [3.5, 4.6, 4.5, 5.5, 4.5, 5.5]
    uv = np.column_stack([along, across] if wide else [across, along])
    guess = np.zeros((len(uv), 2))
    guess[2, 0 if wide else 1] = 33.0   # the last two offsets of the range leave the frame
    guess[3, 0 if wide else 1] = 200.0  # all of them
    *_, status, _ = check(a, b, uv, size, reach, guess=guess)
    assert status[3] == rule.NO_OFFSET and (np.delete(status, 3) < rule.NO_OFFSET).all()
    check(a, b, uv, size, reach)


@pytest.mark.parametrize("as_float", [False, True])
def test_arbitrary_pairs(as_float):
    """Pairs in any order through _lib.stage_displacements -- descending, a frame with itself, one pair twice -- with
    guesses of their own: every pair equals the two-frame call, and the self-pair scores exactly 1 at offset 0."""
    import glimpse_amd
    from glimpse_amd import _lib
    from glimpse_amd.displacements import template_boxes

    a, _ = frames_u8(SMALL)
    arrays = [a, rule.shifted(a, 1, 0, seed=31), rule.shifted(a, 1, 2, seed=32)]
    if as_float:
        arrays = [f.astype(np.float32) for f in arrays]
    uv = points(SMALL, (9, 9))
    pairs = np.array([[2, 0], [1, 1], [0, 2], [2, 0]], dtype=np.int32)
    guess = np.stack([guesses(len(uv)) * s for s in (-1, 0, 1, -1)]).astype(np.int32)
    corners, inside = template_boxes(uv, (9, 9), SMALL)
    got = _lib.stage_displacements(np.stack(arrays), pairs, corners, inside.astype(np.uint8), guess, (9, 9), (4, 3),
                                   return_surface=True)
    for k, (first, second) in enumerate(pairs):
        two = glimpse_amd.displacements(arrays[first], arrays[second], uv, size=(9, 9), reach=(4, 3),
                                        guess=guess[k].astype(np.float64), return_surface=True)
        same(tuple(v[k] for v in got), two)
        same(two, rule.displacements(arrays[first], arrays[second], uv, size=(9, 9), reach=(4, 3), guess=guess[k]))
    same(tuple(v[0] for v in got), tuple(v[3] for v in got))
    duv, score, status, surface = (v[1] for v in got)
    assert (status < rule.NO_OFFSET).all()
    assert (np.rint(duv) == 0.0).all() and all(int(t[0]) == 3 * 9 + 4 for t in rule.tied(surface))
    assert as_float or (score == 1.0).all()
