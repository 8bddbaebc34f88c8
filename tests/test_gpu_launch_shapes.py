"""Every instantiation of the fused frame step the library carries (glh_point_variants.h: 11 launch shapes x 8 codes), run.

pt_shape (glh_point_plan.h) picks the launch shape from the particle count and the observer count; the other GPU tests stop at
counts and observer numbers that reach six of the eleven shapes, and few codes on most of those.  Here, from the recipe
table of tests/launch_shape_cases.py:

* every shape at the particle counts where its own edges show (2048 / 2049, 5120 / 5121, 10240 / 10241, 10500), in three
  configurations (plain / general / rasters) and both arithmetics on the device's Philox draws -- all eight codes --
  against the staged kernels BIT FOR BIT: particles, weights and resample indices after every step, the moments history
  to 1e-12, clean statuses, and last_variant() naming the expected instantiation at every step; in exact arithmetic also
  with every tile forced through the HBM workspaces (set_fused(2));
* `test_every_carried_instantiation_ran`: the instantiations seen, against glimpse_amd.build.variants() -- the header
  parsed the way the build parses it, so an instantiation added without a case fails here;
* the five 1024-thread shapes no other test launches -- (1024, 0, 1 .. 4): observer 0's coordinates parked in c[] and the uv
  scratch; (1024, 10, 2) -- against the oracle directly: resample indices equal at every step, posteriors to 1e-7, in
  exact arithmetic on host-fed draws (code 000) and in fast arithmetic on the device streams read back through
  debug_draws (codes 110, then 011), as tests/test_gpu_pinned.py does for the benched shapes.

The oracle is a NumPy loop.  Measured on the CPU, one run of P = 2 points x T = 3 frames: 0.06 .. 0.19 s at N = 10 500 with one
observer, 0.10 s with two (N = 10 241, 10 240), 0.11 .. 0.13 s with three, 0.16 s with four (N = 10 500) -- P = 2 is kept for
every shape.  The existing N = 10 000, P = 2, T = 3 benched-instantiation case: 0.08 s for its oracle and 10.5 s to render its
2048^2 frames; here a station's 512 x 512 frames render in 1.2 s, once per station and scene seed."""
import numpy as np
import pytest

from tests import launch_shape_cases as lc

pytestmark = pytest.mark.gpu

SEEN = set()   # (tb, ppt, O, S, F, C) launched by the shape tests of this session
DONE = set()   # table entries (shape, N) that ran


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _images(step, n_obs):
    return [step] * (n_obs - 1) + [-1] if lc.missing_image(step, n_obs) else [step] * n_obs


def _run(lib, cs, config, math, mode):
    """T - 1 steps from init_particles(seed=...) on the device's draws; the state is read after EVERY step -- reading it
    expands the compact state, which the next step's choice of code depends on, so the sequence is started again for every
    stop (the Philox streams are keyed on seed, frame, point and particle: the same numbers each time)."""
    import glimpse_amd

    n_obs, n_frames = len(cs["cams"]), cs["T"]
    cfg = lc.configuration(cs, config)
    out = dict(particles=[], weights=[], idx=[], variants=[])
    with lib.Context(cs["P"], cs["N"], n_obs, max_tile=31, max_search_dim=160, max_frames=n_frames) as ctx:
        for o in range(n_obs):
            ctx.observer_init(o, n_frames, cs["imgsz"][0], cs["imgsz"][1], 1, cs["sigmas"][o])
            ctx.observer_set_cameras(o, np.tile(cs["cams"][o], (n_frames, 1)))
            for t in range(n_frames):
                ctx.observer_upload_frame(o, t, cs["frames"][o][t])
        ctx.begin_sequence(cs["P"], cs["N"], lc.TILE)
        if cfg["rasters"]:
            x, y, dem, dem_sigma = cfg["rasters"]
            ctx.set_raster(lib.RASTER_DEM, glimpse_amd.Raster(dem, x=x, y=y))
            ctx.set_raster(lib.RASTER_DEM_SIGMA, glimpse_amd.Raster(dem_sigma, x=x, y=y))
        if config == "plain":
            ctx.set_motion_cartesian(cfg["motion"])
        else:
            ctx.set_motion(cfg["motion"])
        ctx.set_math(math)
        ctx.set_fused(mode)
        ctx.set_debug(2)  # keeps the resample indices; the step stays on the fused kernel
        for stop in range(1, n_frames):
            ctx.set_frame(0)
            ctx.init_particles(seed=lc.SEED)
            for o in range(n_obs):
                ctx.init_templates(o, 0)
            ctx.record_moments(0)
            for i in range(1, stop + 1):
                ctx.step(i, 1.0, _images(i, n_obs), seed=lc.SEED)
                if stop == n_frames - 1:
                    out["idx"].append(ctx.resample_indices())
                    out["variants"].append(ctx.last_variant())
            out["particles"].append(ctx.get_particles())
            out["weights"].append(ctx.get_weights())
        out["moments"] = ctx.get_moments(0, n_frames)
        out["status"] = ctx.point_status()
        out["obs"] = ctx.observer_status_frames(1, n_frames - 1)  # (T - 1, O, P)
    return out


def _check_entry(lib, shape, N):
    """One table entry: every configuration and arithmetic, fused against staged (and, exact, against the HBM-tile hook)."""
    n_obs = shape[2]
    cs = lc.multi_observer_case(n_obs, T=lc.T, P=lc.P, N=N)
    for config in lc.CONFIGS:
        for math in lc.MATHS:
            # (mode 2 has its own LDS plan and with it its own bound on the surfaces the fast arithmetic samples in per-cell
            # form: comparable bit for bit in exact arithmetic only)
            modes = (1, 0, 2) if math == "exact" else (1, 0)
            res = {mode: _run(lib, cs, config, math, mode) for mode in modes}
            what = f"{shape} N={N} {config} {math}"
            want = [tuple(shape) + lc.expected_code(config, math, s, n_obs) for s in range(1, lc.T)]
            for mode in modes:
                r = res[mode]
                got = [tuple(v[:3]) + lc.flags_to_code(v[3]) if v[0] else tuple(v) for v in r["variants"]]
                assert got == (want if mode else [(0, 0, 0, 0)] * (lc.T - 1)), (what, mode, got)
                assert (r["status"] == 0).all(), (what, mode, r["status"])
                ok = np.full(r["obs"].shape, lib.OBS_OK)
                if n_obs > 1:
                    ok[1, n_obs - 1] = lib.OBS_SKIPPED
                np.testing.assert_array_equal(r["obs"], ok, err_msg=f"{what} mode {mode}")
            for other in modes[1:]:
                for s in range(lc.T - 1):
                    msg = f"{what}: fused against mode {other}, step {s + 1}"
                    np.testing.assert_array_equal(res[1]["idx"][s], res[other]["idx"][s], err_msg=msg)
                    np.testing.assert_array_equal(res[1]["particles"][s], res[other]["particles"][s], err_msg=msg)
                    np.testing.assert_array_equal(res[1]["weights"][s], res[other]["weights"][s], err_msg=msg)
                np.testing.assert_allclose(res[1]["moments"], res[other]["moments"], rtol=1e-12, atol=1e-13, err_msg=what)
            assert np.isfinite(res[1]["moments"]).all(), what
            SEEN.update(want)
    DONE.add((tuple(shape), N))


@pytest.mark.parametrize("shape,N", lc.entries(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"N{v}")
def test_every_code_of_a_shape_equals_the_staged_kernels(lib, shape, N):
    _check_entry(lib, shape, N)


def test_every_carried_instantiation_ran(lib):
    """The instantiations the shape tests launched (by last_variant(), step for step) against the build's own list.  Shapes
    a -k selection left out are run here first."""
    from glimpse_amd import build

    for shape, counts in lc.SHAPES:
        if not any((tuple(shape), n) in DONE for n in counts):
            _check_entry(lib, shape, counts[-1])
    carried = set(build.variants())
    unreachable = set(lc.UNREACHABLE)
    missing = carried - SEEN - unreachable
    print(f"{len(carried)} instantiations carried: {len(SEEN & carried)} ran, {len(unreachable)} documented unreachable")
    assert not missing, f"carried instantiations no case launched: {sorted(missing)}"
    assert not SEEN - carried, sorted(SEEN - carried)
    assert len(SEEN & carried) + len(unreachable) == len(carried) == 88


# ---- the five shapes no other test launches, against the oracle ---------------------------------------------------------
RTOL = 1e-7


def _device_run(lib, cs, math, rng):
    """The frame loop, one glh_step per frame (as tests/test_gpu_pinned.py: _device_run).  rng == "philox": the device
    streams, returned as the draws the oracle needs; rng == "host": the case's host-fed draws."""
    n_obs, n_frames = len(cs["cams"]), cs["T"]
    with lib.Context(cs["P"], cs["N"], n_obs, max_tile=31, max_search_dim=160, max_frames=n_frames) as ctx:
        for o in range(n_obs):
            ctx.observer_init(o, n_frames, cs["imgsz"][0], cs["imgsz"][1], 1, cs["sigmas"][o])
            ctx.observer_set_cameras(o, np.tile(cs["cams"][o], (n_frames, 1)))
            for t in range(n_frames):
                ctx.observer_upload_frame(o, t, cs["frames"][o][t])
        ctx.begin_sequence(cs["P"], cs["N"], lc.TILE)
        ctx.set_motion_cartesian(cs["params"])
        ctx.set_math(math)
        ctx.set_debug(2)
        ctx.set_frame(0)
        if rng == "philox":
            ctx.init_particles(seed=lc.SEED)
            init = ctx.debug_draws("init", lc.SEED)
            ev = np.stack([ctx.debug_draws("evolve", lc.SEED, step=i) for i in range(1, n_frames)])
            us = np.stack([ctx.debug_draws("u", lc.SEED, step=i) for i in range(1, n_frames)])
        else:
            init, ev, us = cs["draws"]
            ctx.init_particles(normals=init)
        for o in range(n_obs):
            ctx.init_templates(o, 0)
        ctx.record_moments(0)
        idx, variants = [], []
        for i in range(1, n_frames):
            if rng == "philox":
                ctx.step(i, 1.0, [i] * n_obs, seed=lc.SEED)
            else:
                ctx.step(i, 1.0, [i] * n_obs, normals=ev[i - 1], u=us[i - 1])
            idx.append(ctx.resample_indices())
            variants.append(ctx.last_variant())
        moments = ctx.get_moments(0, n_frames)
        assert (ctx.point_status() == 0).all()
        assert (ctx.observer_status_frames(1, n_frames - 1) == lib.OBS_OK).all()
    return dict(moments=moments, idx=np.stack(idx), variants=variants, draws=(init, ev, us))


@pytest.mark.parametrize("shape", sorted(lc.ORACLE_CASES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["exact-host", "fast-philox"])
def test_never_run_shapes_match_the_oracle(lib, shape, mode):
    """oracle.tracker.track_one with the kernels' SSD accumulation (ssd="row_f32") on the same draws: resample indices
    equal at every step of every point, means and sigmas to 1e-7.  The host-fed cases are admitted by the oracle alone
    (tests/test_launch_shape_cases.py: both accumulations of the SSD give the same indices)."""
    cs = lc.oracle_case(shape)
    n_frames = cs["T"]
    if mode == "exact-host":
        dev = _device_run(lib, cs, "exact", "host")
        want = [(0, 0, 0)] * (n_frames - 1)
    else:
        dev = _device_run(lib, cs, "fast", "philox")
        want = [(1, 1, 0)] + [(0, 1, 1)] * (n_frames - 2)  # the first update reads the expanded prior
        init, _, us = dev["draws"]
        assert np.abs(init).max() < 6.7 and abs(init.std() - 1) < 0.02 and ((0 <= us) & (us < 1)).all()
    got = [(tuple(v[:3]), lc.flags_to_code(v[3])) for v in dev["variants"]]
    assert got == [(tuple(shape), c) for c in want], got
    ref = lc.oracle_tracks(cs, dev["draws"], "row_f32")
    assert ref["clean"]
    bad = [(s, int((dev["idx"][s] != ref["idx"][s]).sum())) for s in range(n_frames - 1)
           if (dev["idx"][s] != ref["idx"][s]).any()]
    assert not bad, f"resample indices differ from the oracle at (step, count): {bad}"
    np.testing.assert_allclose(dev["moments"][..., 0:6], ref["means"], rtol=RTOL, atol=1e-8)
    np.testing.assert_allclose(dev["moments"][..., 6:12], ref["sigmas"], rtol=RTOL, atol=1e-8)
