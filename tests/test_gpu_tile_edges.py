"""The tile, SSD and sampling stages at their edges, against oracle.tiles / oracle.ssd / SciPy directly (whole tracks can hide
a tile error behind the resampling): the stage hooks on uint8 frames for every median window and boundary mode -- boxes
flush with the frame's corners, templates smaller than the window, two-level and saturated content, RGB triplets that share a
channel sum, a constant box --, the template and likelihood stages of a staged context for every frame type on cases of
tests/option_cases.py, and the surface sampling against scipy.interpolate.RectBivariateSpline at the sizes where the fit
changes its method."""
import warnings

import numpy as np
import pytest

from oracle import spline as ospline
from oracle import tiles as otiles
from tests import option_cases as oc

pytestmark = pytest.mark.gpu

WINDOWS = [(r, c) for r in oc.WINDOWS for c in oc.WINDOWS if (r, c) != (1, 1)]
W, H = 96, 80


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


# (template box, search box): flush with each of the four corners of the frame; templates smaller than a 7 x 7 window
# (3 x 3 and 2 wide x 5 high: 'mirror' and 'wrap' fold more than once), in a corner and inside
BOXES = [((0, 0, 15, 11), (0, 0, 30, 27)), ((W - 15, 0, W, 11), (W - 30, 0, W, 27)),
         ((0, H - 11, 15, H), (0, H - 27, 30, H)), ((W - 15, H - 11, W, H), (W - 30, H - 27, W, H)),
         ((40, 30, 43, 33), (38, 28, 44, 35)), ((W - 2, H - 5, W, H), (W - 5, H - 9, W, H)), ((0, 0, 3, 3), (0, 0, 4, 4)),
         ((20, 20, 36, 34), (10, 12, 47, 45))]


def _frames():
    """name -> (template frame, search frame), uint8."""
    rng = np.random.default_rng(21)
    out = {}
    out["gray"] = tuple(rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(2))
    out["rgb"] = tuple(rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
    out["two-level"] = tuple(np.where(rng.random((H, W)) < 0.5, 10, 200).astype(np.uint8) for _ in range(2))
    sat = []
    for _ in range(2):  # saturated: mostly 255, a few 254 and 0
        r = rng.random((H, W))
        sat.append(np.where(r < 0.7, 255, np.where(r < 0.85, 254, 0)).astype(np.uint8))
    out["saturated"] = tuple(sat)
    same = []
    for _ in range(2):  # triplets that differ but share one of three channel sums: ties between unequal pixels
        s = rng.choice([300, 301, 420], (H, W))
        r = rng.integers(np.maximum(0, s - 510), np.minimum(255, s) + 1)
        g = rng.integers(np.maximum(0, s - r - 255), np.minimum(255, s - r) + 1)
        same.append(np.stack((r, g, s - r - g), axis=2).astype(np.uint8))
        assert (same[-1].astype(int).sum(axis=2) == s).all()
    out["same-sum"] = tuple(same)
    for name, (lo, hi) in (("two-level", (10, 200)), ("saturated", (0, 255))):  # (no template box of one value)
        for (x0, y0, x1, y1), _ in BOXES:
            out[name][0][y0, x0], out[name][0][y1 - 1, x1 - 1] = lo, hi
    return out


FRAMES = _frames()


@pytest.mark.parametrize("mode", oc.MODES)
def test_stage_tiles_at_the_edges_for_every_window(lib, mode):
    """_lib.stage_template / stage_search_tile against oracle.tiles.extract_tile (scipy.ndimage.median_filter): hist_q
    exact, tile and hist_v at 1e-12 / 1e-13, the search tile exact as float32 given the oracle's histogram."""
    n = 0
    for name, (f0, f1) in FRAMES.items():
        for tbox, sbox in BOXES:
            raw = otiles.read_box(f0, tbox).astype(int)
            assert np.ptp(raw if raw.ndim == 2 else raw.sum(axis=2)) > 0, (name, tbox)  # (not a constant box: see below)
            for size in WINDOWS:
                want, hist = otiles.extract_tile(f0, np.array(tbox), return_histogram=True, highpass_size=size,
                                                 highpass_mode=mode)
                tile, (hv, hq) = lib.stage_template(f0, tbox, highpass=size, mode=mode)
                where = f"{name} {tbox} window {size} {mode}"
                np.testing.assert_array_equal(hq, hist[1], err_msg=where)
                np.testing.assert_allclose(hv, hist[0], rtol=1e-12, atol=1e-13, err_msg=where)
                np.testing.assert_allclose(tile, want, rtol=1e-12, atol=1e-13, err_msg=where)
                want_s = otiles.extract_tile(f1, np.array(sbox), histogram=hist, highpass_size=size, highpass_mode=mode)
                search = lib.stage_search_tile(f1, sbox, hist, highpass=size, mode=mode)
                np.testing.assert_array_equal(search, want_s.astype(np.float32), err_msg=where)
                n += 1
    assert n == len(FRAMES) * len(BOXES) * len(WINDOWS)


def test_stage_template_of_a_constant_box(lib):
    """A box of one value has zero variance: the reference divides by it and carries NaNs on (helpers.py:344), and so does the
    hook -- an all-NaN tile and a one-entry histogram (NaN, 1.0).  That is the condition `!(var > 0)` under which a context
    flags the point GLH_PT_CONST_TILE (the Tracker's ValueError "Template tile has zero variance")."""
    for frame in (np.full((H, W), 77, np.uint8), np.full((H, W, 3), (3, 250, 99), np.uint8)):
        box = (10, 12, 25, 23)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want, hist = otiles.extract_tile(frame, np.array(box), return_histogram=True)
        assert np.isnan(want).all() and len(hist[0]) == 1 and np.isnan(hist[0][0]) and hist[1][0] == 1.0
        tile, (hv, hq) = lib.stage_template(frame, box)
        assert np.isnan(tile).all() and tile.shape == want.shape
        assert len(hv) == 1 and np.isnan(hv[0]) and list(hq) == [1.0]
    # ... and in a context
    cam = oc.case(oc.SEEDS[0])["cams"][0]
    w, h = int(cam[6]), int(cam[7])
    with lib.Context(1, 64, 1, max_frames=2) as ctx:
        ctx.observer_init(0, 2, w, h, 1, 0.3)
        ctx.observer_set_cameras(0, np.tile(cam, (2, 1)))
        for t in range(2):
            ctx.observer_upload_frame(0, t, np.full((h, w), 77, np.uint8))
        ctx.begin_sequence(1, 64, (15, 15))
        params = np.zeros((1, lib.MOTION_LEN))
        params[0, 0:2] = oc.case(oc.SEEDS[0])["params"][0, 0:2]
        params[0, 2:4] = 0.1
        ctx.set_motion_cartesian(params)
        ctx.set_frame(0)
        ctx.init_particles(seed=1)
        ctx.init_templates(0, 0)
        assert ctx.point_status()[0] & lib.PT_CONST_TILE


# two cases of every frame type from the generator (between them one channel and three, full and squeezed / quantised
# levels, several windows, modes and template shapes)
STAGED = tuple(s for t in oc.FRAME_TYPES for s in [s for s in oc.SEEDS if oc.options(s)["ftype"] == t][:3])


@pytest.mark.parametrize("seed", STAGED)
def test_template_and_likelihood_stages_for_every_frame_type(lib, seed):
    """One step of a staged context (set_fused(0), set_debug(1)) on a generator case: ctx.get_template against the
    oracle's template (box exact, duv, tile and hist_v at 1e-12 / 1e-13, hist_q exact), ctx.likelihood_debug against the
    oracle's trace (the search box exact, the search tile at rtol 1e-5 / atol 1e-6, the SSE surface at 1e-5)."""
    cs = oc.case(seed)
    run = oc.oracle_run(cs, "row_f32", n_frames=2)
    P, N, O, d = cs["P"], cs["N"], len(cs["cams"]), cs["draws"]
    with lib.Context(P, N, O, max_tile=cs["max_tile"], max_search_dim=cs["max_search_dim"], max_frames=2) as ctx:
        for o in range(O):
            ctx.observer_init(o, 2, cs["imgsz"][0], cs["imgsz"][1], cs["channels"], cs["sigmas"][o])
            ctx.observer_set_depth(o, cs["dtype"])
            ctx.observer_set_cameras(o, np.tile(cs["cams"][o], (2, 1)))
            for t in range(2):
                ctx.observer_upload_frame(o, t, cs["frames"][o][t])
        ctx.begin_sequence(P, N, cs["tile"])
        ctx.set_highpass(cs["window"], cs["mode"])
        ctx.set_interpolation(*cs["interp"])
        ctx.set_motion(cs["params"])
        ctx.set_fused(0)
        ctx.set_debug(1)
        ctx.set_frame(0)
        ctx.init_particles(normals=d["init"])
        for o in range(O):
            ctx.init_templates(o, 0)
        ctx.step(1, cs["taus"][0], cs["matching"][1], normals=d["evolve"][0], u=d["u"][0])
        assert (ctx.point_status() == 0).all() and (ctx.observer_status() == lib.OBS_OK).all()
        worst = dict(tile=0.0, hist_v=0.0, search=0.0, sse=0.0)
        for p in range(P):
            _, trace = run[p]
            for o in range(O):
                want, got = trace[0]["templates"][o], ctx.get_template(o, p)
                np.testing.assert_array_equal(got["box"], want["box"])
                np.testing.assert_allclose(got["duv"], want["duv"], rtol=0, atol=1e-9)
                np.testing.assert_array_equal(got["histogram"][1], want["histogram"][1])
                worst["tile"] = max(worst["tile"], float(np.abs(got["tile"] - want["tile"]).max()))
                worst["hist_v"] = max(worst["hist_v"], float(np.abs(got["histogram"][0] - want["histogram"][0]).max()))
                ot, dbg = trace[1]["obs"][o], ctx.likelihood_debug(o, p)
                np.testing.assert_array_equal(dbg["box"], ot["box"])
                worst["search"] = max(worst["search"], float(np.abs(dbg["search"] - ot["search_tile"]).max()))
                worst["sse"] = max(worst["sse"], float(np.abs(dbg["sse"] / ot["sse"] - 1).max()))
                print(f"seed {seed} point {p} observer {o}: largest differences so far {worst}")
                np.testing.assert_allclose(got["tile"], want["tile"], rtol=1e-12, atol=1e-13)
                np.testing.assert_allclose(got["histogram"][0], want["histogram"][0], rtol=1e-12, atol=1e-13)
                np.testing.assert_allclose(dbg["search"], ot["search_tile"].astype(np.float32), rtol=1e-5, atol=1e-6)
                np.testing.assert_allclose(dbg["sse"], ot["sse"], rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("orders", [None, (3, 3), (1, 1), (2, 4), (5, 5)])
def test_stage_sample_against_scipy_at_the_sizes_where_the_fit_changes(lib, orders):
    """_lib.stage_sample against scipy.interpolate.RectBivariateSpline itself (the call of Observer.sample_tile,
    observer.py:201-214) on surfaces of 4, 5, 39, 40, 41 and 64 cells a side, square and not -- around the 40 coefficients
    at which the dense fit gives way to the banded one --, and of 128, 255, 256 and 300 cells a side and 1100 x 40 (what a
    wide prior asks of the banded fit: the surfaces of tests/wide_cases.py), sampled on the first and the last data site,
    on interior knots (data sites), between the box's edge and the outermost sites, and at random points; atol 5e-12.
    The bowl keeps the depth it has at 64 cells on the larger surfaces, so that the bound means the same there (an SSE of
    normalised tiles does not grow with the surface)."""
    rng = np.random.default_rng(9)
    kx, ky = orders or (3, 3)
    sides = (4, 5, 39, 40, 41, 64)
    shapes = [(s, s) for s in sides] + [(4, 64), (64, 5), (39, 41), (41, 40), (40, 39), (5, 40)]
    shapes += [(128, 128), (255, 255), (256, 256), (300, 300), (40, 1100)]
    for ho, wo in shapes:
        if ho < kx + 1 or wo < ky + 1:
            continue
        # an SSE-like surface: a bowl with texture, as float32
        yy, xx = np.mgrid[0:ho, 0:wo]
        curv = 0.002 * min(1.0, (64.0 / max(ho, wo)) ** 2)
        sse = (0.3 + curv * ((xx - 0.4 * wo) ** 2 + (yy - 0.6 * ho) ** 2) + 0.2 * rng.random((ho, wo))).astype(np.float32)
        box = np.array([100.5, 200.5, 100.5 + wo, 200.5 + ho])
        cu, cv = ospline.cell_centres(box, sse.shape)
        sites = np.array([(cu[0], cv[0]), (cu[-1], cv[-1]), (cu[0], cv[-1]), (cu[-1], cv[0]), (cu[1], cv[2]),
                          (cu[2], cv[1]), (cu[wo // 2], cv[ho // 2]), (cu[-3], cv[-2]), (cu[wo // 2], cv[0] + 0.37)])
        edge = np.array([(box[0], box[1]), (box[2], box[3]), (box[0] + 0.2, cv[1]), (cu[1] + 0.1, box[3] - 0.1)])
        inside = np.column_stack((rng.uniform(box[0], box[2], 300), rng.uniform(box[1], box[3], 300)))
        uv = np.concatenate((sites, edge, inside))
        want = ospline.sample_tile(uv, sse.astype(np.float64), box, kx=kx, ky=ky)
        got, outside = lib.stage_sample(sse, box, uv, orders=orders)
        assert not outside.any()
        print(f"orders {orders} surface {ho} x {wo}: largest difference {np.abs(got - want).max():.2e}")
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-12, err_msg=f"surface {ho} x {wo}")
