"""The fused frame step at the particle counts where its per-wave and per-workgroup glue shows, against the staged kernels
bit for bit and -- its random streams -- against the oracle.

Phase A's bounding-box reduction (four extrema of a wave in one butterfly, glh_math.h: wave_max4_joint) and the particle
tests of the unrolled loops (i < N) meet their edges at small counts: N = 70 (one wave full, one partial, six idle), 513
(a second pass with one particle), 1000 (a partial last wave of the second pass) and 5000 (ten passes, the benched
shape), with one point and with three, at two Philox seeds and a non-zero point offset.  Small 512 x 512 scenes, T = 3
frames: from the second update on the fast arithmetic runs the contract code bench.py times.

* fused == staged: particles, weights and resample indices after every step, statuses; moments to 1e-12 (their sums are
  grouped differently); also with two observers, and with particles ABOVE the camera, which project to NaN: the flag and
  the extrema of the remaining particles are both in play, the observer is out of bounds at every step;
* the streams: glh_debug_draws (the generic Philox code) fed to the oracle's whole-track restatement reproduces the fused
  run's resample indices at every step, as tests/test_gpu_pinned.py does at size."""
import numpy as np
import pytest

from tests import launch_shape_cases as lc

pytestmark = pytest.mark.gpu

T = 3
OFFSET = 37          # global index of point 0 (glh_set_point_offset): part of every Philox counter
SEEDS = (7, 20261004)
COUNTS = (70, 513, 1000, 5000)


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _context(lib, cs, params):
    n_obs = len(cs["cams"])
    ctx = lib.Context(cs["P"], cs["N"], n_obs, max_tile=31, max_search_dim=160, max_frames=T)
    for o in range(n_obs):
        ctx.observer_init(o, T, cs["imgsz"][0], cs["imgsz"][1], 1, cs["sigmas"][o])
        ctx.observer_set_cameras(o, np.tile(cs["cams"][o], (T, 1)))
        for t in range(T):
            ctx.observer_upload_frame(o, t, cs["frames"][o][t])
    ctx.begin_sequence(cs["P"], cs["N"], lc.TILE)
    ctx.set_motion_cartesian(params)
    ctx.set_point_offset(OFFSET)
    ctx.set_math("fast")
    ctx.set_debug(2)  # keeps the resample indices; the step stays on the fused kernel
    return ctx


def _run(lib, cs, seed, mode, params=None, lift=None):
    """T - 1 steps on the device's draws, the state read after every step (reading expands the compact state, so the
    sequence is started again for every stop; the streams are keyed on seed, frame, point and particle).
    lift: (point, particles, z) -- those particles of the prior are placed at height z."""
    n_obs = len(cs["cams"])
    out = dict(particles=[], weights=[], idx=[], variants=[])
    with _context(lib, cs, cs["params"] if params is None else params) as ctx:
        ctx.set_fused(mode)
        for stop in range(1, T):
            ctx.set_frame(0)
            ctx.init_particles(seed=seed)
            if lift:
                p0 = ctx.get_particles()
                p0[lift[0], lift[1], 2] = lift[2]
                p0[lift[0], lift[1], 5] = 0.0
                ctx.set_particles(p0)
            for o in range(n_obs):
                ctx.init_templates(o, 0)
            ctx.record_moments(0)
            for i in range(1, stop + 1):
                ctx.step(i, 1.0, [i] * n_obs, seed=seed)
                if stop == T - 1:
                    out["idx"].append(ctx.resample_indices())
                    out["variants"].append(ctx.last_variant())
            out["particles"].append(ctx.get_particles())
            out["weights"].append(ctx.get_weights())
        out["moments"] = ctx.get_moments(0, T)
        out["status"] = ctx.point_status()
        out["obs"] = ctx.observer_status_frames(1, T - 1)  # (T - 1, O, P)
    return out


def _assert_equal_runs(fused, staged, what):
    # the fused kernel took every step: the general fast code on the expanded prior, then the contract code
    codes = [lc.flags_to_code(v[3]) for v in fused["variants"]]
    assert codes == [(1, 1, 0)] + [(0, 1, 1)] * (T - 2), (what, fused["variants"])
    assert all(tuple(v) == (0, 0, 0, 0) for v in staged["variants"]), (what, staged["variants"])
    np.testing.assert_array_equal(fused["status"], staged["status"], err_msg=what)
    np.testing.assert_array_equal(fused["obs"], staged["obs"], err_msg=what)
    for s in range(T - 1):
        msg = f"{what}: step {s + 1}"
        np.testing.assert_array_equal(fused["idx"][s], staged["idx"][s], err_msg=msg)
        np.testing.assert_array_equal(fused["particles"][s], staged["particles"][s], err_msg=msg)
        np.testing.assert_array_equal(fused["weights"][s], staged["weights"][s], err_msg=msg)
    np.testing.assert_allclose(fused["moments"], staged["moments"], rtol=1e-12, atol=1e-13, err_msg=what)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("P", (1, 3))
def test_fused_equals_staged_at_the_wave_edges(lib, P, N, seed):
    cs = lc.multi_observer_case(1, T=T, P=P, N=N)
    fused, staged = (_run(lib, cs, seed, mode) for mode in (1, 0))
    what = f"P={P} N={N} seed={seed}"
    _assert_equal_runs(fused, staged, what)
    assert (fused["status"] == 0).all() and (fused["obs"] == lib.OBS_OK).all(), what
    assert np.isfinite(fused["moments"]).all(), what


@pytest.mark.parametrize("N", (513, 5000))
def test_fused_equals_staged_with_two_observers(lib, N):
    cs = lc.multi_observer_case(2, T=T, P=3, N=N)
    fused, staged = (_run(lib, cs, SEEDS[0], mode) for mode in (1, 0))
    _assert_equal_runs(fused, staged, f"two observers, N={N}")
    assert (fused["status"] == 0).all() and (fused["obs"] == lib.OBS_OK).all()


@pytest.mark.parametrize("N", (70, 1000))
def test_fused_equals_staged_with_particles_that_project_to_nan(lib, N):
    """Five particles of point 0 sit above the nadir camera (height 100): they project to NaN at every step, so the point's
    observer is out of bounds while the extrema of its other particles are still reduced; without a DEM term
    (dem_sigma = 0) the weights are then uniform and those particles survive into the contract code's steps.  The other
    points run clean through the code that takes the weight straight from a single observer's likelihood."""
    cs = lc.multi_observer_case(1, T=T, P=3, N=N)
    params = cs["params"].copy()
    params[:, 17] = 0.0
    lifted = np.array([0, 1, 63, 64, N - 1])
    fused, staged = (_run(lib, cs, SEEDS[1], mode, params=params, lift=(0, lifted, 150.0)) for mode in (1, 0))
    _assert_equal_runs(fused, staged, f"NaN projections, N={N}")
    assert (staged["obs"][:, 0, 0] == lib.OBS_OUT_OF_BOUNDS).all(), staged["obs"]
    assert (staged["obs"][:, 0, 1:] == lib.OBS_OK).all(), staged["obs"]
    # the lifted particles are still there after the last step (nothing weighted them down)
    assert (fused["particles"][-1][0, :, 2] > 100.0).any()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("P,N", [(1, 70), (3, 513), (1, 1000), (3, 5000)])
def test_streams_fed_to_the_oracle_reproduce_the_fused_run(lib, P, N, seed):
    """The numbers of the device streams read back through glh_debug_draws -- the generic Philox code, keyed as the kernels key
    them, point offset included -- as the oracle's draws: its resample indices equal the fused run's at every step."""
    cs = lc.multi_observer_case(1, T=T, P=P, N=N)
    with _context(lib, cs, cs["params"]) as ctx:
        ctx.set_frame(0)
        ctx.init_particles(seed=seed)
        init = ctx.debug_draws("init", seed)
        ev = np.stack([ctx.debug_draws("evolve", seed, step=i) for i in range(1, T)])
        us = np.stack([ctx.debug_draws("u", seed, step=i) for i in range(1, T)])
        ctx.init_templates(0, 0)
        ctx.record_moments(0)
        idx, variants = [], []
        for i in range(1, T):
            ctx.step(i, 1.0, [i], seed=seed)
            idx.append(ctx.resample_indices())
            variants.append(ctx.last_variant())
        moments = ctx.get_moments(0, T)
        assert (ctx.point_status() == 0).all()
        assert (ctx.observer_status_frames(1, T - 1) == lib.OBS_OK).all()
    assert [lc.flags_to_code(v[3]) for v in variants] == [(1, 1, 0)] + [(0, 1, 1)] * (T - 2), variants
    assert init.shape == (P, N, 6) and ev.shape == (T - 1, P, N, 3) and ((0 <= us) & (us < 1)).all()
    ref = lc.oracle_tracks(cs, (init, ev, us), "row_f32")
    assert ref["clean"]
    bad = [(s, int((idx[s] != ref["idx"][s]).sum())) for s in range(T - 1) if (idx[s] != ref["idx"][s]).any()]
    assert not bad, f"resample indices differ from the oracle at (step, count): {bad}"
    np.testing.assert_allclose(moments[..., 0:6], ref["means"], rtol=1e-7, atol=1e-8)
    np.testing.assert_allclose(moments[..., 6:12], ref["sigmas"], rtol=1e-7, atol=1e-8)
