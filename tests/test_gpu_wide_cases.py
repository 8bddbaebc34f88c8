"""The designed cases of tests/wide_cases.py through the frame step (glh_step, C ABI) against the oracle: search tiles of
93 .. 1110 pixels a side for every frame type, and particle counts either side of the last one the fused kernel takes up
to the last one glh_create takes -- sizes an ordinary caller reaches (Tracker(max_search_dim=None) grows the workspaces
with the prior) and the seeded sweeps do not.

  * whole tracks: both arithmetics on the path the plan picks (asserted from the profile and from last_variant), against
    the admitted row_f32 run of the oracle, 0 differing resample indices; the cases the fused kernel takes once more on
    the staged kernels and, in exact arithmetic, with the tiles forced into the HBM workspaces;
  * stages: template, search box, search tile and SSE surface of one staged step against the oracle's trace (a whole
    track can hide a tile error behind the resampling);
  * device draws: 12 000 and 14 950 particles in fast arithmetic on the Philox streams, the draws read back and handed
    to the oracle.
The cases, their sizes and the device figures: INPUTS.md, "The wide-tile cases"; without a GPU: tests/test_wide_cases.py."""
import numpy as np
import pytest

from tests import option_cases as oc
from tests import test_gpu_option_sweep as sweep
from tests import wide_cases as wc

pytestmark = pytest.mark.gpu

RTOL, ATOL = sweep.RTOL, sweep.ATOL  # 1e-7, 1e-8: the sweep's
SEED = 20261021


def _rtol_needed(got, want):
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(0.0, float(np.nanmax(np.where(np.abs(want) > 0, (np.abs(got - want) - ATOL) / np.abs(want), 0.0))))


def _compare(cs, got, ref, where):
    """Indices, moments and statuses of a device run against the oracle's; returns (differing indices, rtol needed)."""
    from glimpse_amd import _lib

    n_bad = int((got["idx"] != ref["idx"]).sum())
    means, sigmas = got["moments"][:, :, 0:6], got["moments"][:, :, 6:12]
    need = max(_rtol_needed(means, ref["means"]), _rtol_needed(sigmas, ref["sigmas"]))
    largest = max(float(np.abs(means - ref["means"]).max()), float(np.abs(sigmas - ref["sigmas"]).max()))
    print(f"{where}: variants {sorted(set(got['variants']))}, stages {got['stages']}, {n_bad} indices differ, moments "
          f"need rtol {need:.2e} beside atol {ATOL} (largest absolute difference {largest:.2e})")
    assert n_bad == 0, f"{where}: {n_bad} resample indices differ from the oracle"
    np.testing.assert_allclose(means, ref["means"], rtol=RTOL, atol=ATOL, err_msg=where)
    np.testing.assert_allclose(sigmas, ref["sigmas"], rtol=RTOL, atol=ATOL, err_msg=where)
    assert (got["status"] == 0).all(), got["status"]
    assert (got["obs_status"] == _lib.OBS_OK).all(), got["obs_status"]
    return n_bad, need


def _assert_path(name, got, fused, math):
    """The launch path of every step, from the profile and from the record of the fused instantiation."""
    stages, variants = got["stages"], got["variants"]
    assert len(variants) == wc.T - 1
    if fused:
        assert "point_step" in stages and "resample" not in stages, (name, stages)
        assert all(v[0] > 0 and v[2] == len(wc.case(name)["cams"]) for v in variants), (name, variants)
        assert all((v[3] & 1) == (math == "fast") for v in variants), (name, variants)
        if name == "n10976":
            assert all(v[:3] == (1024, 0, 1) for v in variants), variants
    else:
        assert "point_step" not in stages and "resample" in stages and "ssd" in stages, (name, stages)
        assert all(v[0] == 0 for v in variants), (name, variants)


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("name", wc.NAMES)
def test_whole_tracks_match_the_oracle(name, math):
    """0 resample indices differ from the admitted row_f32 run at any step of either point; means and sigmas at the
    sweep's rtol 1e-7 / atol 1e-8; point and observer statuses clean; the path is the one pt_plan picks.  A case the fused
    kernel takes runs again with set_fused(0) and, in exact arithmetic, with set_fused(2): index for index the first run."""
    admission = wc.admit(name)
    assert admission["ok"], admission["why"]
    cs, ref = wc.case(name), admission["ref"]
    w, h = wc.largest_tile(admission["run"])
    fused = name in wc.FUSED
    got = sweep.run_case(cs, math)
    where = (f"{name} {math}: {cs['ftype']} x{cs['channels']}, N {cs['N']}, largest search tile {w} x {h}, "
             f"{'fused' if fused else 'staged'}")
    _assert_path(name, got, fused, math)
    _compare(cs, got, ref, where)
    if fused:
        for mode in (0, 2) if math == "exact" else (0,):
            other = sweep.run_case(cs, math, fused=mode)
            _assert_path(name, other, mode == 2, math)
            _compare(cs, other, ref, f"{where}, set_fused({mode})")
            np.testing.assert_array_equal(other["idx"], got["idx"])
            np.testing.assert_allclose(other["moments"], got["moments"], rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("name", tuple(wc.TILE_CASES))
def test_stages_of_one_step_match_the_oracle(name):
    """One step of a staged context (set_fused(0), set_debug(1)), as tests/test_gpu_tile_edges.py does it, at the wide
    sizes: get_template against the oracle's template (box and hist_q exact, duv at 1e-9, tile and hist_v at 1e-12 /
    1e-13), likelihood_debug against the oracle's trace (the search box exact, the search tile at rtol 1e-5 / atol 1e-6,
    the SSE surface at rtol 1e-5 / atol 1e-7: that file's tolerances)."""
    from glimpse_amd import _lib as lib

    cs, run = wc.case(name), wc.admit(name)["run"]
    P, N, d = cs["P"], cs["N"], cs["draws"]
    with lib.Context(P, N, 1, max_tile=cs["max_tile"], max_search_dim=cs["max_search_dim"], max_frames=2) as ctx:
        ctx.observer_init(0, 2, cs["imgsz"][0], cs["imgsz"][1], cs["channels"], cs["sigmas"][0])
        ctx.observer_set_depth(0, cs["dtype"])
        ctx.observer_set_cameras(0, np.tile(cs["cams"][0], (2, 1)))
        for t in range(2):
            ctx.observer_upload_frame(0, t, cs["frames"][0][t])
        ctx.begin_sequence(P, N, cs["tile"])
        ctx.set_highpass(cs["window"], cs["mode"])
        ctx.set_interpolation(*cs["interp"])
        ctx.set_motion(cs["params"])
        ctx.set_fused(0)
        ctx.set_debug(1)
        ctx.set_frame(0)
        ctx.init_particles(normals=d["init"])
        ctx.init_templates(0, 0)
        ctx.step(1, cs["taus"][0], cs["matching"][1], normals=d["evolve"][0], u=d["u"][0])
        assert (ctx.point_status() == 0).all() and (ctx.observer_status() == lib.OBS_OK).all()
        reached = False
        for p in range(P):
            _, trace = run[p]
            want, got = trace[0]["templates"][0], ctx.get_template(0, p)
            ot, dbg = trace[1]["obs"][0], ctx.likelihood_debug(0, p)
            assert dbg["box"] is not None
            ws, hs = int(dbg["box"][2] - dbg["box"][0]), int(dbg["box"][3] - dbg["box"][1])
            reached |= wc.in_class(name, ws, hs)
            search_want = ot["search_tile"].astype(np.float32)
            same_shape = dbg["search"].shape == search_want.shape and dbg["sse"].shape == ot["sse"].shape
            worst = dict(tile=float(np.abs(got["tile"] - want["tile"]).max()),
                         hist_v=float(np.abs(got["histogram"][0] - want["histogram"][0]).max())
                         if len(got["histogram"][0]) == len(want["histogram"][0]) else np.inf,
                         search=float(np.abs(dbg["search"] - search_want).max()) if same_shape else np.inf,
                         sse=float(np.abs(dbg["sse"] / ot["sse"] - 1).max()) if same_shape else np.inf,
                         search_cells_differing=int((dbg["search"] != search_want).sum()) if same_shape else -1)
            print(f"{name} point {p}: search tile {ws} x {hs}, surface {dbg['sse'].shape[1]} x {dbg['sse'].shape[0]}, "
                  f"largest differences {worst}")
            np.testing.assert_array_equal(got["box"], want["box"])
            np.testing.assert_allclose(got["duv"], want["duv"], rtol=0, atol=1e-9)
            np.testing.assert_array_equal(got["histogram"][1], want["histogram"][1])
            np.testing.assert_allclose(got["tile"], want["tile"], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(got["histogram"][0], want["histogram"][0], rtol=1e-12, atol=1e-13)
            np.testing.assert_array_equal(dbg["box"], ot["box"])
            np.testing.assert_allclose(dbg["search"], search_want, rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(dbg["sse"], ot["sse"], rtol=1e-5, atol=1e-7)
        assert reached, f"{name}: no point's first search tile lies in the size class"


@pytest.mark.parametrize("name", ["n12000", "n14950"])
def test_staged_counts_on_the_device_streams_match_the_oracle(name):
    """Fast arithmetic on the Philox streams at counts only the staged kernels take: the draws are read back with
    debug_draws and handed to the oracle (as tests/test_gpu_pinned.py: _device_run does it on the fused kernel); 0
    differing indices against its row_f32 run, moments at rtol 1e-7 / atol 1e-8, and no step ran the fused kernel."""
    from glimpse_amd import _lib

    cs = wc.case(name)
    P, N, T = cs["P"], cs["N"], cs["T"]
    with _lib.Context(P, N, 1, max_tile=cs["max_tile"], max_search_dim=cs["max_search_dim"], max_frames=T) as ctx:
        ctx.observer_init(0, T, cs["imgsz"][0], cs["imgsz"][1], cs["channels"], cs["sigmas"][0])
        ctx.observer_set_cameras(0, np.tile(cs["cams"][0], (T, 1)))
        for t in range(T):
            ctx.observer_upload_frame(0, t, cs["frames"][0][t])
        ctx.begin_sequence(P, N, cs["tile"])
        ctx.set_motion(cs["params"])
        ctx.set_math("fast")
        ctx.set_debug(2)
        ctx.set_frame(0)
        ctx.init_particles(seed=SEED)
        draws = dict(init=ctx.debug_draws("init", SEED),
                     evolve=np.stack([ctx.debug_draws("evolve", SEED, step=i) for i in range(1, T)]),
                     u=np.stack([ctx.debug_draws("u", SEED, step=i) for i in range(1, T)]))
        ctx.init_templates(0, 0)
        ctx.record_moments(0)
        idx, variants = [], []
        for i in range(1, T):
            ctx.step(i, cs["taus"][i - 1], cs["matching"][i], seed=SEED)
            idx.append(ctx.resample_indices())
            variants.append(ctx.last_variant())
        got = dict(idx=np.stack(idx), moments=ctx.get_moments(0, T), status=ctx.point_status(),
                   obs_status=ctx.observer_status_frames(1, T - 1), variants=variants,
                   stages={k: v[1] for k, v in ctx.profile_get().items() if v[1] > 0})
    init = draws["init"]
    assert init.shape == (P, N, 6) and np.abs(init).max() < 6.7 and abs(init.std() - 1) < 0.02
    assert ((0 <= draws["u"]) & (draws["u"] < 1)).all()
    run = oc.oracle_run(dict(cs, draws=draws), "row_f32")
    assert oc._clean(cs, run)
    ref = dict(idx=np.stack([[tr["idx"] for tr in trace if "idx" in tr] for _, trace in run], axis=1),
               means=np.stack([res["means"] for res, _ in run], axis=1),
               sigmas=np.stack([res["sigmas"] for res, _ in run], axis=1))
    _assert_path(name, got, False, "fast")
    _compare(cs, got, ref, f"{name} fast, device Philox draws, N {N}, staged")


def test_glh_create_refuses_the_count_after_the_last():
    """wide_cases.CREATE_LAST is the last count a context takes: the next one is refused at creation."""
    from glimpse_amd import _lib

    with _lib.Context(1, wc.CREATE_LAST, 1, max_frames=2):
        pass
    with pytest.raises(_lib.GlhError):
        _lib.Context(1, wc.CREATE_LAST + 1, 1, max_frames=2)
