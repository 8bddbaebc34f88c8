"""The admitted cases of tests/surface_cases.py through the frame step (glh_step, C ABI) with the context's dem, dem_sigma
and viewshed rasters set, against the oracle's whole-track restatement over the same surfaces (oracle/raster.py: SciPy's
RegularGridInterpolator; oracle/motion.py; oracle/tracker.py, viewshed=) on the same host-fed draws, index for index: the
raster instantiation of the fused kernel (k_point_step, SURF = 2) with its LDS windows, and the staged kernels, in both
arithmetics.  The reference is the oracle's run with the SSD accumulated like the kernels do (Observer(ssd="row_f32")); the
admission rule (surface_cases.admit) has made sure that its indices do not hinge on that choice, that no particle sits on
an outer limit or a viewshed cell border unless the case pins it there, and that the designed failures happen where the
case says.

The sweep's coverage (which code serves which share of the samples) and its device figures: INPUTS.md, "The surface sweep"."""
import numpy as np
import pytest

from tests import option_cases as oc
from tests import surface_cases as sc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-7, 1e-8  # those of tests/test_gpu_option_sweep.py
# Particles after the first step against the oracle's evolved[idx].  Exact arithmetic: what tests/test_oracle_golden.py grants
# the oracle's own motion step against the reference.  Fast arithmetic: ten times the largest |device - oracle| / (1 + |oracle|)
# measured over the sweep on an MI355X (INPUTS.md, "The surface sweep") -- a handful of roundings per sample.
EXACT_RTOL, EXACT_ATOL = 1e-13, 1e-14
FAST_MEASURED = 1.96e-16  # (exact arithmetic: 1.82e-16 on the staged kernels, 4.4e-17 on the fused kernel)
FAST_BOUND = 10 * FAST_MEASURED

# What the kernels raise in the SAME frame downstream of a track's error, where the reference has already left the track: the
# status word of the failing frame is the bit of the error plus these, and the library reports the first bit in the order of
# glimpse_amd/tracker.py: _ERRORS (the order in which the reference would meet them), which is the error itself.
#   * a Cartesian point beyond the outer limit of `dem`: the particles out there get a NaN DEM term, hence NaN weights, and the
#     cumulative sum the resampling searches falls short of 1 -- PT_RESAMPLE_CLAMP, the reference's IndexError on such weights;
#   * a point out of bounds when its particles are drawn: their heights are NaN, so is the mean the template is cut around --
#     PT_TEMPLATE_OOB, the reference's IndexError on a box that is no box.
def downstream(name, point):
    from glimpse_amd import _lib

    return {("leaves_the_raster", 0): _lib.PT_RESAMPLE_CLAMP, ("on_the_limit", 1): _lib.PT_TEMPLATE_OOB}.get((name, point), 0)


_RUNS = {}      # (name, math) -> what the launch-path count needs
_RASTERS = {}   # name -> the case's glimpse_amd.Rasters


def rasters(cs):
    import glimpse_amd

    if cs["name"] not in _RASTERS:
        _RASTERS.clear()  # (one case's rasters at a time: some have a third of a million nodes)
        _RASTERS[cs["name"]] = {k: None if v is None else glimpse_amd.Raster(v[0], x=v[1], y=v[2])
                                for k, v in cs["surfaces"].items()}
    return _RASTERS[cs["name"]]


def run_case(cs, math, fused=1):
    from glimpse_amd import _lib

    P, N, T, O = cs["P"], cs["N"], cs["T"], len(cs["cams"])
    d, sf = cs["draws"], rasters(cs)
    with _lib.Context(P, N, O, max_tile=cs["max_tile"], max_search_dim=cs["max_search_dim"], max_frames=T) as ctx:
        for o in range(O):
            ctx.observer_init(o, T, cs["imgsz"][0], cs["imgsz"][1], cs["channels"], cs["sigmas"][o])
            ctx.observer_set_depth(o, cs["dtype"])
            ctx.observer_set_cameras(o, np.tile(cs["cams"][o], (T, 1)))
            for t in range(T):
                ctx.observer_upload_frame(o, t, cs["frames"][o][t])
        ctx.begin_sequence(P, N, cs["tile"])
        ctx.set_highpass(cs["window"], cs["mode"])
        ctx.set_interpolation(*cs["interp"])
        for slot, key in ((_lib.RASTER_DEM, "dem"), (_lib.RASTER_DEM_SIGMA, "dem_sigma"), (_lib.RASTER_VIEWSHED, "viewshed")):
            ctx.set_raster(slot, sf[key])
        ctx.set_motion(cs["params"])
        ctx.set_math(math)
        ctx.set_fused(fused)
        ctx.set_frame(0)
        ctx.init_particles(normals=d["init"])
        for o in range(O):
            ctx.init_templates(o, 0)
        ctx.record_moments(0)
        ctx.set_debug(2)  # resample indices
        idx, variants, status, first = [], [], [ctx.point_status()], None
        for i in range(1, T):
            ctx.step(i, cs["taus"][i - 1], cs["matching"][i], normals=d["evolve"][i - 1], u=d["u"][i - 1])
            idx.append(ctx.resample_indices())
            variants.append(ctx.last_variant())
            status.append(ctx.point_status())
            if i == 1:
                first = ctx.get_particles()
        return dict(idx=np.stack(idx), moments=ctx.get_moments(0, T), status=np.stack(status),
                    error_frame=ctx.point_error_frame(), obs_status=ctx.observer_status_frames(1, T - 1),
                    variants=variants, first=first)


def deviation(got, want):
    with np.errstate(invalid="ignore"):
        return float(np.nanmax(np.abs(got - want) / (1.0 + np.abs(want)), initial=0.0))


def compare(cs, ref, got, math):
    """Indices, moments, statuses and the particles after the first step of one run against the oracle's; returns the number
    of differing indices and the first step's deviation (asserted by the caller's rule, printed first)."""
    from glimpse_amd import _lib
    from glimpse_amd.tracker import _failures

    bits = {sc.OOB: _lib.PT_RASTER_OOB, sc.HIDDEN: _lib.PT_NOT_VISIBLE, sc.MISSING: _lib.PT_NAN}
    T, P = cs["T"], cs["P"]
    errs = ref["errors"]
    clean = [p for p in range(P) if errs[p] is None]
    n_bad = 0
    for p in range(P):
        steps = T - 1 if errs[p] is None else max(errs[p][0] - 1, 0)  # the steps the oracle's track completed
        n_bad += int((got["idx"][:steps, p] != ref["idx"][:steps, p]).sum())
    # a failed track ends where it failed: the library's own rule (glimpse_amd/tracker.py: _failures) on the device's words
    means, sigmas = got["moments"][:, :, 0:6].copy(), got["moments"][:, :, 6:12].copy()
    for p in np.nonzero(got["status"][-1])[0]:
        means[int(got["error_frame"][p]):, p] = sigmas[int(got["error_frame"][p]):, p] = np.nan
    want_first = np.stack([ref["evolved"][1, p][ref["idx"][0, p]] for p in clean])
    dev = deviation(got["first"][clean], want_first)
    print(f"{cs['name']} {math}: variant {got['variants'][-1]}, {n_bad} indices differ, first step deviates by {dev:.2e}, "
          f"status {got['status'].tolist()}, error frames {got['error_frame'].tolist()}")
    assert n_bad == 0, f"{n_bad} resample indices differ from the oracle"
    np.testing.assert_allclose(means, ref["means"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sigmas, ref["sigmas"], rtol=RTOL, atol=ATOL)
    for p in range(P):
        if errs[p] is None:
            assert (got["status"][:, p] == 0).all(), (p, got["status"][:, p])
            continue
        frame, message = errs[p]
        # nothing before the oracle's failing frame; at it exactly the bit of its error (and what follows from it in that
        # frame: downstream); the word stays as it is; the library's reading of it is the oracle's error, its frame too
        assert (got["status"][:frame, p] == 0).all(), (p, got["status"][:, p])
        assert got["status"][frame, p] == bits[message] | downstream(cs["name"], p), (p, message, got["status"][:, p])
        assert (got["status"][frame:, p] == got["status"][frame, p]).all(), (p, got["status"][:, p])  # later frames add none
        error = _failures(got["status"][-1, p:p + 1], np.array([frame]), ())[0]
        assert isinstance(error, ValueError) and str(error) == message, (p, got["status"][-1, p], error)
        assert got["error_frame"][p] == frame, (p, got["error_frame"][p], frame)
    want = np.where(cs["matching"][1:] >= 0, _lib.OBS_OK, _lib.OBS_SKIPPED)  # (T - 1, O)
    np.testing.assert_array_equal(got["obs_status"][:, :, clean],
                                  np.broadcast_to(want[:, :, None], got["obs_status"][:, :, clean].shape))
    if math == "exact":
        np.testing.assert_allclose(got["first"][clean], want_first, rtol=EXACT_RTOL, atol=EXACT_ATOL)
    else:
        assert dev <= FAST_BOUND, (dev, FAST_BOUND)
    # one launch path per case, on the raster instantiation where it is the fused kernel, in the arithmetic asked for
    assert len({v[0] > 0 for v in got["variants"]}) == 1
    if got["variants"][-1][0] > 0:
        assert all(v[3] & 8 for v in got["variants"]), got["variants"]
        assert all((v[3] & 1) == (math == "fast") for v in got["variants"])
    return n_bad, dev


def check_case(name, math, fused=1):
    admission = sc.admit(name)
    assert admission["ok"], admission["why"]
    cs, ref = sc.case(name), admission["ref"]
    got = run_case(cs, math, fused)
    n_bad, dev = compare(cs, ref, got, math)
    is_fused = got["variants"][-1][0] > 0
    if fused == 1:
        _RUNS[name, math] = dict(fused=is_fused, flags=got["variants"][-1][3], n_bad=n_bad, dev=dev)
        assert is_fused == (cs["interp"] in oc.FUSED_ORDERS and max(cs["tile"]) <= 63)
    else:
        assert is_fused == (fused == 2)
    return got


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("name", sc.SEEDS + ("glacier",))
def test_frame_step_over_gridded_surfaces_matches_the_oracle(name, math):
    """0 resample indices differ from the oracle's at every step of every point (no allowance); means and sigmas at the option
    sweep's rtol 1e-7 / atol 1e-8; every status word clean, every image used but the missing one; the raster instantiation
    on every fused step; the particles after the first step are the oracle's evolved[idx] -- to rtol 1e-13 / atol 1e-14 in
    exact arithmetic, to ten times the measured deviation in fast arithmetic.  Eight of the fused cases once more on the
    staged kernels and (exact arithmetic) with the tiles forced into the HBM workspaces: equal indices, moments to
    1e-11 / 1e-12."""
    got = check_case(name, math)
    if name in sc.AGAIN:
        for mode in (0, 2) if math == "exact" else (0,):
            other = check_case(name, math, fused=mode)
            np.testing.assert_array_equal(other["idx"], got["idx"])
            np.testing.assert_allclose(other["moments"], got["moments"], rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("name", ["border_tie_ascending", "border_tie_descending"])
def test_a_particle_on_a_viewshed_cell_border_takes_the_oracle_s_cell(name, math):
    """Every particle of four points exactly on the border between a visible and a hidden viewshed cell (y0 == 0.5): the
    status word of each is what the oracle's nearest-neighbour lookup implies -- clean, or PT_NOT_VISIBLE from frame 0 --
    with the axes ascending and descending."""
    got = check_case(name, math)
    assert sorted(np.nonzero(got["status"][0])[0]) == [0, 2]


@pytest.mark.parametrize("math", ["exact", "fast"])
def test_a_point_on_the_outer_limit_is_inside_and_one_ulp_beyond_is_not(math):
    """x pinned exactly to dem.max[0]: tracked, extrapolated, indices equal to the oracle's; its twin one ulp beyond carries
    PT_RASTER_OOB from frame 0 (and PT_TEMPLATE_OOB: no template around a NaN mean) and only NaN rows."""
    from glimpse_amd import _lib

    got = check_case("on_the_limit", math)
    assert got["status"][0, 1] & _lib.PT_RASTER_OOB and got["status"][0, 0] == got["status"][0, 2] == 0
    assert got["error_frame"][1] == 0 and np.isnan(sc.admit("on_the_limit")["ref"]["means"][:, 1]).all()


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("fused", [1, 0])
def test_tracks_that_fail_mid_sequence_fail_at_the_oracle_s_frame(fused, math):
    """A cloud that crosses the outer limit of `dem`, one that walks onto hidden viewshed cells, one that runs into NaN nodes:
    each point carries exactly the bit of its error at the oracle's failing frame and none before (the point beyond `dem`
    also PT_RESAMPLE_CLAMP, raised by the NaN weights of that very frame: `downstream`), point_error_frame() names that
    frame, its moments are the oracle's up to it and NaN from it on; the clean point matches index for index -- on the
    fused kernel and on the staged kernels."""
    got = check_case("leaves_the_raster", math, fused)
    assert (got["variants"][-1][0] > 0) == (fused == 1)
    assert (got["status"][-1][:3] != 0).all() and got["status"][-1][3] == 0


def test_both_launch_paths_take_their_share_of_the_surface_sweep():
    """Per arithmetic: how many cases ran on the raster instantiation of the fused kernel and how many on the staged kernels
    -- neither is empty -- and 0 differing indices over all of them."""
    for math in ("exact", "fast"):
        names = sc.SEEDS + ("glacier",)
        for name in names:
            if (name, math) not in _RUNS:
                check_case(name, math)
        runs = [_RUNS[name, math] for name in names]
        raster = sum(r["fused"] and bool(r["flags"] & 8) for r in runs)
        staged = sum(not r["fused"] for r in runs)
        print(f"{math}: raster instantiation {raster}, staged kernels {staged} of {len(runs)}; differing indices "
              f"{sum(r['n_bad'] for r in runs)}; largest first-step deviation {max(r['dev'] for r in runs):.2e}")
        assert raster > 0 and staged > 0 and raster + staged == len(runs)
        assert sum(r["n_bad"] for r in runs) == 0
