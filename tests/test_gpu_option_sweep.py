"""The admitted cases of tests/option_cases.py through the frame step (glh_step, C ABI) against the oracle's whole-track
restatement on the same host-fed draws, index for index: every frame type, median window, boundary mode, spline order
and motion model the library serves, where they meet -- on the fused kernel's general instantiations and on the staged
kernels, in both arithmetics.  The reference is the oracle's run with the SSD accumulated like the kernels do
(Observer(ssd="row_f32"), which tests/test_gpu_parity.py: test_stage_ssd_matches_oracle holds the kernels to bit for bit);
the admission rule (option_cases.admit) has made sure that its indices do not hinge on that choice.

The sweep's coverage and its device figures: INPUTS.md, "The option sweep"."""
import numpy as np
import pytest

from tests import option_cases as oc

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-7, 1e-8  # those of tests/test_gpu_random_sweep.py

# ten of the cases the fused kernel takes: run again on the staged kernels and with the tiles forced into the workspaces
AGAIN = tuple(s for s in oc.SEEDS if oc.options(s)["interp"] in oc.FUSED_ORDERS and max(oc.options(s)["tile"]) <= 63)[:10]

_RUNS = {}  # (seed, math) -> what the launch-path count needs


def run_case(cs, math, fused=1):
    from glimpse_amd import _lib

    P, N, T, O = cs["P"], cs["N"], cs["T"], len(cs["cams"])
    d = cs["draws"]
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
        ctx.set_motion(cs["params"])
        ctx.set_math(math)
        ctx.set_fused(fused)
        ctx.set_frame(0)
        ctx.init_particles(normals=d["init"])
        for o in range(O):
            ctx.init_templates(o, 0)
        ctx.record_moments(0)
        ctx.set_debug(2)  # resample indices
        idx, variants = [], []
        for i in range(1, T):
            ctx.step(i, cs["taus"][i - 1], cs["matching"][i], normals=d["evolve"][i - 1], u=d["u"][i - 1])
            idx.append(ctx.resample_indices())
            variants.append(ctx.last_variant())
        stages = {k: v[1] for k, v in ctx.profile_get().items() if v[1] > 0}  # stage -> launches
        return dict(idx=np.stack(idx), moments=ctx.get_moments(0, T), status=ctx.point_status(),
                    obs_status=ctx.observer_status_frames(1, T - 1), variants=variants, stages=stages)


def check_case(seed, math):
    from glimpse_amd import _lib

    admission = oc.admit(seed)
    assert admission["ok"], admission["why"]
    cs, ref = oc.case(seed), admission["ref"]
    got = run_case(cs, math)
    n_bad = int((got["idx"] != ref["idx"]).sum())
    means, sigmas = got["moments"][:, :, 0:6], got["moments"][:, :, 6:12]
    with np.errstate(divide="ignore", invalid="ignore"):
        err = max(float(np.nanmax(np.where(np.abs(b) > 0, (np.abs(a - b) - ATOL) / np.abs(b), 0.0)))
                  for a, b in ((means, ref["means"]), (sigmas, ref["sigmas"])))
    fused = got["variants"][-1][0] > 0  # (the staged kernels leave the record of the fused instantiation empty)
    _RUNS[seed, math] = dict(fused=fused, flags=got["variants"][-1][3], n_bad=n_bad, ftype=cs["ftype"])
    print(f"seed {seed} {math}: {cs['ftype']} x{cs['channels']} {cs['levels']}, window {cs['window']} {cs['mode']}, "
          f"orders {cs['interp']}, {oc.KINDS[cs['kind']]}, template {cs['tile']}, N {cs['N']}: variant "
          f"{got['variants'][-1]}, {n_bad} indices differ, moments need rtol {max(err, 0.0):.2e}")
    assert n_bad == 0, f"{n_bad} resample indices differ from the oracle"
    np.testing.assert_allclose(means, ref["means"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(sigmas, ref["sigmas"], rtol=RTOL, atol=ATOL)
    # statuses as the oracle's run implies: every track clean, every image used but the missing one
    assert (got["status"] == 0).all(), got["status"]
    want = np.where(cs["matching"][1:] >= 0, _lib.OBS_OK, _lib.OBS_SKIPPED)  # (T - 1, O)
    np.testing.assert_array_equal(got["obs_status"], np.broadcast_to(want[:, :, None], got["obs_status"].shape))
    # one launch path per case, in the arithmetic asked for
    assert len({v[0] > 0 for v in got["variants"]}) == 1
    if fused:
        assert all((v[3] & 1) == (math == "fast") for v in got["variants"])
    else:
        assert cs["interp"] not in oc.FUSED_ORDERS or max(cs["tile"]) > 63
    if seed in AGAIN:
        assert fused
        for mode in (0, 2) if math == "exact" else (0,):  # (mode 2 has its own bound on the per-cell sampling form of the
            other = run_case(cs, math, fused=mode)       # fast arithmetic, tests/test_gpu_fused.py: compared in exact)
            assert (other["variants"][-1][0] > 0) == (mode == 2)
            np.testing.assert_array_equal(other["idx"], got["idx"])
            np.testing.assert_allclose(other["moments"], got["moments"], rtol=1e-11, atol=1e-12)
    return _RUNS[seed, math]


@pytest.mark.parametrize("math", ["exact", "fast"])
@pytest.mark.parametrize("seed", oc.SEEDS)
def test_frame_step_matches_the_oracle_over_the_option_space(seed, math):
    """0 resample indices differ from the oracle's at every step of every point (no allowance: the admission rule is what
    makes 0 the right number); means and sigmas at the random sweep's rtol 1e-7 / atol 1e-8; point and observer statuses as
    the oracle's run implies; ten of the fused cases once more on the staged kernels and with the tiles in the HBM
    workspaces, index for index."""
    check_case(seed, math)


def test_both_launch_paths_take_their_share_of_the_sweep():
    """Over the admitted cases, in either arithmetic: the fused kernel's general instantiation took the steps of at least
    half of them, the staged kernels those of at least a quarter (other spline orders, templates above 63 pixels)."""
    for math in ("exact", "fast"):
        runs = [_RUNS.get((seed, math)) or check_case(seed, math) for seed in oc.SEEDS]
        general = sum(r["fused"] and bool(r["flags"] & 2) for r in runs)
        staged = sum(not r["fused"] for r in runs)
        plain = len(runs) - general - staged
        bad = {t: sum(r["n_bad"] for r in runs if r["ftype"] == t) for t in oc.FRAME_TYPES}
        print(f"{math}: fused general {general}, fused plain {plain}, staged {staged} of {len(runs)}; differing indices {bad}")
        assert 2 * general >= len(runs), (general, len(runs))
        assert 4 * staged >= len(runs), (staged, len(runs))
        assert sum(bad.values()) == 0
