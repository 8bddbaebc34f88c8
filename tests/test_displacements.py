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
