"""glimpse_amd.displacements on the CPU: the NumPy restatement of the rule (tests/displacement_rule.py) recovers known
shifts, the host side of the package (template boxes, refusals) does what the rule says, and every status arises from
the input the rule names for it.  No GPU: the device is pinned to the restatement in tests/test_gpu_displacements.py."""
import datetime

import numpy as np
import pytest

from tests import displacement_rule as rule

ONE = np.float64(1.0)
TWO_ULP = 2 * np.spacing(ONE)


def grid_points(shape, margin, step):
    rows, cols = shape
    u, v = np.meshgrid(np.arange(margin, cols - margin, step) + 0.5, np.arange(margin, rows - margin, step) + 0.5)
    return np.column_stack([u.ravel(), v.ravel()])


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("shift", [(3, -2), (-4, 1), (5, 5), (-5, 0), (0, 0)])
def test_restatement_recovers_whole_pixel_shifts(shift, as_float):
    """White noise and its copy moved by whole pixels, both signs, up to a shift equal to the reach (5): every point's
    peak is the shift, with a score within 2 ulp of 1."""
    a = rule.noise_u8()
    a = a.astype(np.float32) if as_float else a
    b = rule.shifted(a, *shift)
    uv = grid_points(a.shape, margin=14, step=11)
    assert len(uv) >= 12
    duv, score, status, _ = rule.displacements(a, b, uv, size=(9, 9), reach=(5, 5), subpixel=False)
    assert (status == rule.MATCHED).all()
    assert (duv == np.asarray(shift, dtype=float)).all()
    assert (np.abs(score - ONE) <= TWO_ULP).all(), np.abs(score - ONE).max()


def test_subpixel_term_beats_whole_pixels_on_a_band_limited_texture():
    """A texture of seed rule.TEXTURE_SEED without energy above rule.TEXTURE_BANDWIDTH cycles per pixel, moved by a
    fraction of a pixel in the Fourier domain: for every point the sub-pixel estimate is nearer the truth than the
    whole-pixel one.  (Recorded, not asserted: with 15 x 15 templates the error of the sub-pixel estimate over the 40
    points had a median of 0.05 to 0.06 px and a maximum of 0.14 to 0.21 px for these three shifts, against 0.43 to 0.68 px
    for whole pixels.)"""
    a = rule.texture().astype(np.float32)
    uv = grid_points(a.shape, margin=16, step=13)
    for truth in [(0.3, -0.4), (1.35, 0.75), (-2.6, 1.45)]:
        b = rule.texture(shift=truth).astype(np.float32)
        fine, _, status, _ = rule.displacements(a, b, uv, size=(15, 15), reach=(4, 4))
        coarse, _, _, _ = rule.displacements(a, b, uv, size=(15, 15), reach=(4, 4), subpixel=False)
        assert (status == rule.MATCHED).all()
        error_fine, error_coarse = (np.hypot(*(d - truth).T) for d in (fine, coarse))
        print(f"shift {truth}: sub-pixel error up to {error_fine.max():.4f} px, whole-pixel {error_coarse.max():.4f} px")
        assert (error_fine < error_coarse).all()
        assert (np.abs(fine - coarse) <= 0.5).all()


def test_template_boxes_equal_tile_box():
    """template_boxes is Observer.tile_box point by point where that does not raise, and flags exactly where it does."""
    from glimpse_amd import Image, Observer
    from glimpse_amd.displacements import template_boxes

    rows, cols = 40, 57
    t0 = datetime.datetime(2020, 1, 1)
    cam = {"imgsz": (cols, rows), "f": (50, 50)}
    images = [Image(cam=dict(cam), array=np.zeros((rows, cols), dtype=np.uint8), datetime=t0 + datetime.timedelta(days=k))
              for k in range(2)]
    observer = Observer(images)
    rng = np.random.default_rng(3)
    uv = np.column_stack([rng.uniform(-3, cols + 3, 400), rng.uniform(-3, rows + 3, 400)])
    uv[:40] = np.round(uv[:40] * 2) / 2  # (halves: the ties of floor(x + 0.5), and boxes flush with an edge)
    uv = np.vstack([uv, [[2.5, 2.0], [cols - 2.5, rows - 2.0], [2.5 - 1e-9, 2.0], [np.nan, 5.0], [5.0, np.inf]]])
    for size in [(5, 4), (4, 5), (15, 15)]:
        corners, inside = template_boxes(uv, size, (rows, cols))
        raised = 0
        for k, point in enumerate(uv):
            try:
                box = observer.tile_box(point, size, 0)
            except (IndexError, ValueError):
                raised += 1
                assert not inside[k], (point, size)
                continue
            assert inside[k], (point, size)
            assert tuple(corners[k]) == (box[0], box[1]), (point, size)
            assert (box[2] - box[0], box[3] - box[1]) == size
        assert 0 < raised < len(uv)


def test_refusals_come_before_the_library_is_loaded(monkeypatch):
    import glimpse_amd
    from glimpse_amd import _lib

    def no_load():
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(_lib, "load", no_load)
    a = rule.noise_u8()
    uv = np.array([[40.0, 30.0]])
    for kwargs in [dict(size=(2, 9)), dict(size=(9, 64)), dict(size=(65, 9)), dict(reach=(0, 4)), dict(reach=(4, 33))]:
        with pytest.raises(ValueError):
            glimpse_amd.displacements(a, a, uv, **kwargs)
    with pytest.raises(ValueError):
        glimpse_amd.displacements(a, a[:-1], uv)
    for bad in [np.zeros(2), np.zeros((3, 3)), np.zeros((2, 2, 2))]:
        with pytest.raises(ValueError):
            glimpse_amd.displacements(a, a, bad)
    for frame in [a.astype(np.int16), a.astype(np.int32), a.astype(bool), a.astype(np.float16)]:
        with pytest.raises(NotImplementedError):
            glimpse_amd.displacements(frame, frame, uv)
    with pytest.raises(NotImplementedError):
        glimpse_amd.displacements(np.zeros((8, 8, 2), dtype=np.uint8), np.zeros((8, 8, 2), dtype=np.uint8), uv)
    duv, score, status = glimpse_amd.displacements(a, a, np.empty((0, 2)))
    assert duv.shape == (0, 2) and score.shape == (0,) and status.shape == (0,) and status.dtype == np.uint8
    *_, surface = glimpse_amd.displacements(a, a, np.empty((0, 2)), reach=(2, 3), return_surface=True)
    assert surface.shape == (0, 7, 5)


def test_status_names():
    from glimpse_amd import _lib

    assert _lib.DISPLACEMENT_STATUS == rule.STATUS
    assert _lib.DISPLACEMENT_GUESS_LIMIT == rule.GUESS_LIMIT


@pytest.mark.parametrize("as_float", [False, True])
def test_each_status_arises_from_its_input(as_float):
    a = rule.noise_u8()
    a = a.astype(np.float32) if as_float else a
    b = rule.shifted(a, 2, 0)
    uv = np.array([[40.0, 30.0]])
    kwargs = dict(size=(9, 9), reach=(3, 3))
    assert rule.displacements(a, b, uv, **kwargs)[2][0] == rule.MATCHED
    # a constant template
    flat = a.copy()
    flat[20:41, 30:51] = 7
    duv, score, status, surface = rule.displacements(flat, b, uv, **kwargs)
    assert status[0] == rule.FLAT and np.isnan(duv).all() and np.isnan(score).all() and np.isnan(surface).all()
    # a box that leaves the frame, a uv that is not finite
    for point in ([[2.0, 30.0]], [[40.0, 58.0]], [[np.nan, 30.0]]):
        duv, score, status, _ = rule.displacements(a, b, np.array(point), **kwargs)
        assert status[0] == rule.OUTSIDE and np.isnan(duv).all() and np.isnan(score).all()
    # a guess that puts every window outside b (also one that is not finite)
    for guess in ([[200.0, 0.0]], [[0.0, -90.0]], [[np.inf, 0.0]], [[1e30, 0.0]]):
        duv, score, status, surface = rule.displacements(a, b, uv, guess=np.array(guess), **kwargs)
        assert status[0] == rule.NO_OFFSET and np.isnan(duv).all() and np.isnan(score).all() and np.isnan(surface).all()
    # a peak on the border of the range: the shift equals the reach
    duv, score, status, _ = rule.displacements(a, rule.shifted(a, 3, 0), uv, **kwargs)
    assert status[0] == rule.EDGE and abs(score[0] - 1) <= TWO_ULP
    assert duv[0, 0] == 3.0 and abs(duv[0, 1]) < 0.5  # (no term on the axis of the border, one on the other)
    # ... which subpixel=False never reports
    assert rule.displacements(a, rule.shifted(a, 3, 0), uv, subpixel=False, **kwargs)[2][0] == rule.MATCHED
    # a peak beside an invalid offset: the frame's edge cuts the range
    duv, _, status, surface = rule.displacements(a, a, np.array([[4.5, 30.0]]), **kwargs)
    assert status[0] == rule.EDGE and duv[0, 0] == 0.0 and abs(duv[0, 1]) < 0.5 and np.isnan(surface[0, :, :3]).all()


def test_nan_pixels_on_the_float_path():
    """A NaN inside the template gives "flat template"; a NaN inside some windows of a valid template skips them."""
    a = rule.noise_u8().astype(np.float32)
    b = rule.shifted(a, 1, 1)
    uv = np.array([[40.0, 30.0]])
    kwargs = dict(size=(9, 9), reach=(3, 3))
    holed = a.copy()
    holed[30, 40] = np.nan
    assert rule.displacements(holed, b, uv, **kwargs)[2][0] == rule.FLAT
    holed = b.copy()
    holed[23, 40] = np.nan  # (the template's rows are 26 .. 34: row 23 is the top row of the windows of j = 0 alone)
    duv, score, status, surface = rule.displacements(a, holed, uv, **kwargs)
    assert status[0] == rule.MATCHED and np.allclose(duv[0], (1, 1), atol=0.5)
    assert np.isnan(surface[0, 0]).all() and np.isfinite(surface[0, 1:]).all()
    holed = b.copy()
    holed[31, 41] = np.inf  # (the centre of the matching window: every window holds it)
    assert rule.displacements(a, holed, uv, **kwargs)[2][0] == rule.NO_OFFSET


@pytest.mark.parametrize("as_float", [False, True])
def test_tie_goes_to_the_first_in_row_major_order(as_float):
    """Two identical features inside the reach: the first in row-major order of (j, i) wins."""
    a = rule.noise_u8(seed=5)
    b = np.full(a.shape, 128, dtype=np.uint8)
    b[::2, ::2] += 1  # (windows that vary, so that they are valid, and that correlate little with noise)
    feature = a[26:35, 36:45]  # the 9 x 9 template of (40.5, 30.5)
    b[26 - 5:35 - 5, 36 + 5:45 + 5] = feature  # offset (+5, -5): row 0 of the surface, its last column
    b[26 + 5:35 + 5, 36 - 5:45 - 5] = feature  # offset (-5, +5): the last row, its first column
    if as_float:
        a, b = a.astype(np.float32), b.astype(np.float32)
    duv, score, status, surface = rule.displacements(a, b, np.array([[40.5, 30.5]]), size=(9, 9), reach=(5, 5),
                                                     subpixel=False)
    assert surface[0, 0, 10] == surface[0, 10, 0] == score[0]
    assert tuple(duv[0]) == (5.0, -5.0) and status[0] == rule.MATCHED


def test_mean_rule_and_uint16():
    """Three channels are averaged in float64 and cast to float32; uint16 widens exactly."""
    from glimpse_amd.displacements import frame_plane

    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, size=(9, 11, 3), dtype=np.uint8)
    assert frame_plane(rgb).dtype == np.float32
    assert (frame_plane(rgb) == rgb.mean(axis=2).astype(np.float32)).all()
    assert (frame_plane(rgb) == rule.plane(rgb)).all()
    gray = rgb[:, :, 0]
    assert frame_plane(gray) is gray or (frame_plane(gray).dtype == np.uint8 and (frame_plane(gray) == gray).all())
    wide = rng.integers(0, 65536, size=(9, 11), dtype=np.uint16)
    assert frame_plane(wide).dtype == np.float32 and (frame_plane(wide).astype(np.uint16) == wide).all()
    assert frame_plane(wide.astype(np.float64)).dtype == np.float32


def test_whole_guess():
    from glimpse_amd.displacements import whole_guess

    g = whole_guess([[0.5, 1.5], [-0.5, 2.4999], [np.nan, -np.inf], [1e30, -1e30]])
    assert g.dtype == np.int32
    assert g.tolist() == [[0, 2], [0, 2], [rule.GUESS_LIMIT, rule.GUESS_LIMIT], [rule.GUESS_LIMIT, -rule.GUESS_LIMIT]]
    assert [[rule.whole(v) for v in row] for row in [[0.5, 1.5], [-0.5, 2.4999], [np.nan, -np.inf], [1e30, -1e30]]] == g.tolist()


# ---- the scenes of tests/test_gpu_displacements.py: the condition that makes each device test meaningful ---------------

PERIODIC_GUESS = np.array([(3.0, 2.0), (-5.0, 7.0), (0.0, -3.0), (9.0, 4.0)])  # one per point, in turn


def periodic_guess(n):
    return PERIODIC_GUESS[np.arange(n) % len(PERIODIC_GUESS)]


@pytest.mark.parametrize("as_float", [False, True])
def test_periodic_scene_ties_every_point(as_float):
    """rule.periodic_u8 matched against itself with 9 x 9 templates and a reach of (16, 16): every point's largest score
    is shared by offsets in different waves and strides of a 256-thread workgroup, the first of them wins, and for some
    points the first positions of the tied lattice are invalid."""
    frame = rule.periodic_u8()
    px, py = 7, 5
    frame = frame.astype(np.float32) if as_float else frame
    uv = rule.edge_points(frame.shape, (9, 9))
    rx = ry = 16
    nxo = 2 * rx + 1
    duv, score, status, surface = rule.displacements(frame, frame, uv, size=(9, 9), reach=(rx, ry))
    coarse, _, coarse_status, _ = rule.displacements(frame, frame, uv, size=(9, 9), reach=(rx, ry), subpixel=False)
    ties = rule.tied(surface)
    print("tied offsets per point:", [len(t) for t in ties], "status:", status.tolist())
    assert all(len(t) >= 2 for t in ties)
    assert (score == 1.0).all()
    assert rule.MATCHED in status and rule.EDGE in status and set(status) <= {rule.MATCHED, rule.EDGE}
    assert (coarse_status == rule.MATCHED).all()
    assert any(len({(o % 256) // 64 for o in t}) > 1 for t in ties)  # the same score in two waves
    assert any(len({o // 256 for o in t}) > 1 for t in ties)         # ... and in two strides of the workgroup
    skipped = 0
    for k, t in enumerate(ties):
        first = int(t[0])
        assert tuple(coarse[k]) == (first % nxo - rx, first // nxo - ry)  # the winner is the smallest tied offset
        # the lattice of offsets a whole number of periods from 0, where the windows are equal; those before the winner
        # are not on the surface: their windows leave the frame
        lattice = [j * nxo + i for j in range(2 * ry + 1) for i in range(nxo) if (i - rx) % px == 0 and (j - ry) % py == 0]
        assert set(t) <= set(lattice)
        before = [o for o in lattice if o < first]
        assert np.isnan(surface[k].ravel()[before]).all()
        skipped += bool(before)
    assert 0 < skipped < len(uv)
    # with the guesses the lattice moves: the first tied offset lies in the second row of offsets or later
    guess = periodic_guess(len(uv))
    coarse, score, status, surface = rule.displacements(frame, frame, uv, size=(9, 9), reach=(rx, ry), guess=guess,
                                                        subpixel=False)
    ties = rule.tied(surface)
    assert (score == 1.0).all() and all(len(t) >= 2 for t in ties)
    rows = {int(t[0]) // nxo for t in ties}
    assert min(rows) >= 1 and len(rows) > 2
    for k, t in enumerate(ties):
        assert tuple(coarse[k]) == (guess[k, 0] + int(t[0]) % nxo - rx, guess[k, 1] + int(t[0]) // nxo - ry)


@pytest.mark.parametrize("as_float", [False, True])
def test_half_striped_scene_ties_the_peak_with_its_neighbour(as_float):
    """rule.half_striped_u8 against itself: for the points inside, the peak is the first window that lies in the striped
    part; the offset before it scores less, the offset after it the same in every bit, and the sub-pixel term of that
    axis is computed from them: den = (a_ - 2) + 1 < 0 and a term of (a_ - 1) / (2 den), which is 0.5 but for the rounding
    of a_ - 2 (0.5000000000000002 here: the rule's |term| <= 0.5 holds in exact arithmetic, not to the last bit).  Some of
    the tied offsets are a multiple of 256 apart, so one thread of the workgroup meets the same score twice; the lattice of
    the periodic scene has no such pair (165 a + 7 b is no multiple of 256 for |b| <= 4, a <= 6)."""
    frame = rule.half_striped_u8()
    frame = frame.astype(np.float32) if as_float else frame
    uv = rule.edge_points(frame.shape, (9, 9))
    duv, score, status, surface = rule.displacements(frame, frame, uv, size=(9, 9), reach=(16, 16))
    assert (score == 1.0).all() and all(len(t) >= 2 for t in rule.tied(surface))
    assert any(len({int(o) % 256 for o in t}) < len(t) for t in rule.tied(surface))
    for k in range(8, 13):
        l, _ = rule.box(*uv[k], 9, 9, frame.shape)
        assert l >= 40 + 2 and status[k] == rule.MATCHED
        j, i = divmod(int(rule.tied(surface)[k][0]), 33)
        assert l + i - 16 == 40
        assert surface[k, j, i - 1] < surface[k, j, i] == surface[k, j, i + 1] == 1.0
        term = rule.vertex(surface[k, j, i - 1], 1.0, 1.0)
        assert duv[k, 0] == (i - 16) + term and abs(term - 0.5) < 1e-12


SATURATED_POINTS = np.array([[80.0, 65.0], [31.5, 31.5], [160 - 31.5, 130 - 31.5], [70.3, 60.8]])


def window_sums(b, l, t, w, h, rx, ry):
    """(sum(S), sum(S^2)) as Python integers for every offset whose window lies in `b`."""
    out = []
    for j in range(-ry, ry + 1):
        for i in range(-rx, rx + 1):
            x, y = l + i, t + j
            if 0 <= x and x + w <= b.shape[1] and 0 <= y and y + h <= b.shape[0]:
                S = b[y:y + h, x:x + w].astype(np.int64)
                out.append((int(S.sum()), int((S * S).sum())))
    return out


def test_saturated_scene_fills_the_32_bit_sums():
    """rule.saturated_u8 with 63 x 63 templates: sum(S^2) of some window exceeds 2^27 and every sum stays below 2^32 (the
    largest sum a window of uint8 pixels can have, 63 * 63 * 255^2 = 258 084 225, is 2^27.94: a factor of 16.6 below
    2^32).  The interior point is matched at the shift."""
    a, b = rule.saturated_u8()
    duv, score, status, _ = rule.displacements(a, b, SATURATED_POINTS[:1], size=(63, 63), reach=(32, 32), subpixel=False)
    assert status[0] == rule.MATCHED and tuple(duv[0]) == rule.SATURATED_SHIFT and score[0] == 1.0
    l, t = rule.box(*SATURATED_POINTS[0], 63, 63, a.shape)
    sums = window_sums(b, l, t, 63, 63, 32, 32)
    T = a[t:t + 63, l:l + 63].astype(np.int64)
    largest = max(max(q for _, q in sums), int((T * T).sum()), 255 * int(T.sum()))  # (255 sum(T) bounds every sum(T S))
    print(f"largest 32-bit sum {largest} = 2^{np.log2(largest):.3f}: 2^32 is {2 ** 32 / largest:.2f} times that")
    assert 2 ** 27 < largest < 2 ** 32
    assert largest > 0.98 * 63 * 63 * 255 ** 2  # (within 2 % of what uint8 pixels allow)
    assert 2 ** 32 / largest > 16


def test_holes_scene_has_small_variances_under_large_sums():
    """rule.holes_u8: every 63 x 63 window holds k = 1 .. 9 pixels of 0 among 255 (one per cell of 32 x 32), so
    n sum(S^2) - sum(S)^2 = 255^2 k (n - k) is k / n of n sum(S^2), below 2^-8, and the interior point is matched at the
    shift with a score of exactly 1."""
    a, b = rule.holes_u8()
    duv, score, status, surface = rule.displacements(a, b, SATURATED_POINTS[:1], size=(63, 63), reach=(32, 32),
                                                     subpixel=False)
    assert status[0] == rule.MATCHED and tuple(duv[0]) == rule.SATURATED_SHIFT and score[0] == 1.0
    l, t = rule.box(*SATURATED_POINTS[0], 63, 63, a.shape)
    n = 63 * 63
    sums = window_sums(b, l, t, 63, 63, 32, 32)
    assert len(sums) == int(np.isfinite(surface).sum())  # (no window is constant)
    ratios = [(n * q - s * s) / (n * q) for s, q in sums]
    assert 0 < min(ratios) and max(ratios) < 2 ** -8
    assert min(q for _, q in sums) > 2 ** 27


def test_subnormal_scene():
    """rule.subnormal_f32: every pixel is a nonzero float32 subnormal; the rule widens each to float64, where it is an
    ordinary number, so no point is "flat template" and an interior point is matched at the shift."""
    a, b = rule.subnormal_f32()
    tiny = np.finfo(np.float32).tiny
    for f in (a, b):
        assert f.dtype == np.float32 and (f > 0).all() and (f < tiny).all()
    assert len(np.unique(a)) == 256
    uv = rule.edge_points(a.shape, (9, 9))
    duv, score, status, _ = rule.displacements(a, b, uv, size=(9, 9), reach=(3, 3))
    assert set(status) == {rule.MATCHED, rule.EDGE}
    assert status[8] == rule.MATCHED and tuple(np.rint(duv[8])) == rule.SUBNORMAL_SHIFT and abs(score[8] - 1) <= TWO_ULP


def test_huge_scene():
    """rule.huge_f32: pixels up to 2.4e38, finite in float32, whose sums of products stay finite in float64."""
    a, b = rule.huge_f32()
    for f in (a, b):
        assert f.dtype == np.float32 and np.isfinite(f).all() and f.max() > 2e38
    uv = rule.edge_points(a.shape, (9, 9))
    duv, score, status, surface = rule.displacements(a, b, uv, size=(9, 9), reach=(3, 3))
    assert set(status) == {rule.MATCHED, rule.EDGE}
    assert status[8] == rule.MATCHED and tuple(np.rint(duv[8])) == rule.SUBNORMAL_SHIFT and abs(score[8] - 1) <= TWO_ULP


# ---- the restatement against exact arithmetic ---------------------------------------------------------------------------

def exact_scores(a, b, l, t, w, h, rx, ry):
    """{(j, i): score} of every offset whose window lies in `b` and varies: num, vt and vs as Python integers,
    num / sqrt(vt vs) with 60 decimal digits, rounded once to float64."""
    import decimal

    context = decimal.Context(prec=60)
    n = w * h
    T = [int(v) for v in a[t:t + h, l:l + w].ravel()]
    st, stt = sum(T), sum(v * v for v in T)
    vt = n * stt - st * st
    out = {}
    for j in range(2 * ry + 1):
        for i in range(2 * rx + 1):
            x, y = l + i - rx, t + j - ry
            if not (0 <= x and x + w <= b.shape[1] and 0 <= y and y + h <= b.shape[0]):
                continue
            S = [int(v) for v in b[y:y + h, x:x + w].ravel()]
            ss, sq, sx = sum(S), sum(v * v for v in S), sum(p * q for p, q in zip(T, S))
            vs, num = n * sq - ss * ss, n * sx - st * ss
            if vs > 0:
                root = context.sqrt(decimal.Decimal(vt * vs))
                out[(j, i)] = float(context.divide(decimal.Decimal(num), root))
    return out


def noise_pair():
    a = rule.noise_u8(seed=11)
    b = rule.shifted(a, 2, -1, seed=12)
    b[::7, ::5] ^= 3
    return a, b


EXACT_CASES = [(noise_pair, (9, 9), (3, 3), np.array([[48.0, 30.0], [30.0, 20.0], [4.5, 4.5], [92.5, 56.5]])),
               (rule.saturated_u8, (63, 63), (3, 3), SATURATED_POINTS[:2]),
               (rule.holes_u8, (63, 63), (2, 2), SATURATED_POINTS[:1])]


@pytest.mark.parametrize("as_float", [False, True])
@pytest.mark.parametrize("case", range(len(EXACT_CASES)))
def test_restatement_against_exact_arithmetic(case, as_float):
    """The surface of the restatement lies within 2 ulp of num / sqrt(vt vs) formed exactly.  The bound is derived: the
    rule rounds three times on exact inputs -- the product vt vs, the square root, the quotient -- each by half an ulp at
    most, and the root halves the relative error of the product: 0.25 + 0.5 + 0.5 ulp, and the ulp of the exact value
    may be half that of its neighbour across a power of two.  On the float path the frames hold whole numbers, every sum
    is exact below 2^53, and the same bound holds.  (About 200 offsets over white noise, the saturated scene and the scene
    of 255 with holes.)"""
    scene, size, reach, uv = EXACT_CASES[case]
    a, b = scene()
    fa, fb = (a.astype(np.float32), b.astype(np.float32)) if as_float else (a, b)
    *_, status, surface = rule.displacements(fa, fb, uv, size=size, reach=reach)
    checked, worst = 0, 0.0
    for k, (u, v) in enumerate(uv):
        assert status[k] < rule.NO_OFFSET
        l, t = rule.box(u, v, *size, a.shape)
        exact = exact_scores(a, b, l, t, *size, *reach)
        assert len(exact) == int(np.isfinite(surface[k]).sum())
        for (j, i), want in exact.items():
            got = surface[k, j, i]
            ulp = np.spacing(abs(np.float64(want))) if want != 0 else np.spacing(np.float64(0))
            worst = max(worst, abs(got - want) / ulp)
            assert abs(got - want) <= 2 * ulp, (k, j, i, got, want)
            checked += 1
    print(f"{checked} offsets, the largest difference {worst} ulp")
    assert checked >= 25
