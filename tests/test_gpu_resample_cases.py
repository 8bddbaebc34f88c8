"""The resampling kernels and their moments on designed weight sets (tests/resample_cases.py): a lost track (every weight at
the 1e-300 floor), one survivor with N copies at index 0, N - 1, on a wave or thread-segment boundary, two survivors at the
ends, weights over 300 orders of magnitude, NaN weights -- and offsets u that tie positions with cumulative weights.

Staged kernel (k_resample), every method that searches the cumulative weights:
  * exact arithmetic: the indices equal the NumPy restatement of the kernel's own segmented scan bit for bit at EVERY u,
    ties included; PT_RESAMPLE_CLAMP is raised exactly when the restatement clamps; the gathered particles and weights are
    particles[idx], weights[idx].  (The outputs two threads write -- resample_cases.kernel_systematic: `contested` -- are
    held to the reach rule instead: which thread writes last is not the kernel's to say.)
  * fast arithmetic (systematic): no index differs from the exact rational answer at the decided offsets; at u = 0 and
    nextafter(1, 0) it equals it on decided positions and stays within reach elsewhere.
  * the largest particle count a context accepts, and the refusal of one more.
Moments: mean and variance of the gathered set against a two-pass longdouble reference, in units of the error model of the
one-pass shifted form (eps max|x - K| for the mean, eps (sigma^2 + |K - mean|^2) for the variance, K the pivot), at g5's
coordinate scale; a cloud that has collapsed onto one particle has sigma exactly 0, wherever the point's first particle is.
Fused kernel, phases D / E / F: survivors forced through the DEM term, against the staged kernels bit for bit and against
the restatement.

INPUTS.md ("Resampling: designed weight sets") records what these print:
    pytest tests/test_gpu_resample_cases.py -s
"""
import functools

import numpy as np
import pytest

from tests import launch_shape_cases as lc
from tests import resample_cases as rc

pytestmark = pytest.mark.gpu

# glimpse_hip.hip, glh_create: refused when max_particles * 10 + 4096 > 150 * 1024 (c[N], the rank tables and 4 KB of
# tree nodes and scan scratch in one workgroup's LDS)
MAX_PARTICLES = (150 * 1024 - 4096) // 10
SCALE = np.array([1, 1, 0.1, 0.2, 0.2, 0.01])
CENTRE = np.array([5e5, 6.7e6, 400, 0.1, 0, 0])   # g5's coordinates (tools/make_golden.py)
EPS = 2.0 ** -53                                   # unit roundoff


@pytest.fixture(scope="module")
def lib():
    from glimpse_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


@functools.lru_cache(maxsize=None)
def _cases(n):
    return rc.CASES(n)


@functools.lru_cache(maxsize=None)
def _exact_systematic(n, name, u):
    return rc.exact_systematic(dict(_cases(n))[name], u, reach=True)


def _particles(P, n, seed=0):
    return np.random.default_rng(seed + n).standard_normal((P, n, 6)) * SCALE + CENTRE


def _resample(ctx, particles, weights, u, method="systematic", math="exact"):
    P, n = weights.shape
    ctx.begin_sequence(P, n, (15, 15))   # (also clears the point status)
    ctx.set_debug(2)
    ctx.set_math(math)
    ctx.set_particles(particles)
    ctx.set_weights(weights)
    ctx.set_frame(0)
    ctx.resample(u=u, method=method)
    return dict(idx=ctx.resample_indices(), particles=ctx.get_particles(), weights=ctx.get_weights(),
                status=[int(s) for s in ctx.point_status()], moments=ctx.get_moments(0, 1)[0])


def _offsets(names, which):
    """u (P,) of one launch: `which` 0 / 1 -- each case's first / second decided offset; 2 / 3 -- u = 0 / nextafter(1, 0)."""
    return np.array([rc.decided_offsets(name)[which] if which < 2 else rc.U_TIES[which - 2] for name in names])


def _assert_gathered(out, particles, weights, what):
    for p in range(len(weights)):
        idx = out["idx"][p]
        assert ((0 <= idx) & (idx < weights.shape[1])).all(), (what, p)
        np.testing.assert_array_equal(out["particles"][p], particles[p][idx], err_msg=f"{what} point {p}")
        np.testing.assert_array_equal(out["weights"][p], weights[p][idx], err_msg=f"{what} point {p}")


@pytest.mark.parametrize("n", rc.COUNTS)
def test_exact_arithmetic_equals_the_restatement_at_every_offset(lib, n):
    names = [name for name, _ in _cases(n)]
    weights = np.stack([w for _, w in _cases(n)])
    P = len(names)
    particles = _particles(P, n)
    with lib.Context(P, n, 1, max_frames=2) as ctx:
        for which in range(4):
            us = _offsets(names, which)
            out = _resample(ctx, particles, weights, us)
            _assert_gathered(out, particles, weights, f"n={n} systematic u#{which}")
            for p, name in enumerate(names):
                what = f"n={n} {name} u={us[p]!r} systematic"
                want, clamped, contested = rc.kernel_systematic(weights[p], us[p], contested=True)
                got = out["idx"][p]
                np.testing.assert_array_equal(got[~contested], want[~contested], err_msg=what)
                assert bool(out["status"][p] & lib.PT_RESAMPLE_CLAMP) == clamped, (what, out["status"][p])
                assert out["status"][p] & ~lib.PT_RESAMPLE_CLAMP == 0, (what, out["status"][p])
                if contested.any():
                    print(f"{what}: outputs {np.nonzero(contested)[0]} are written by two threads; restated "
                          f"{want[contested]}, device {got[contested]}")
                    rc.check_against_exact(got, _exact_systematic(n, name, float(us[p])), n, what, where=contested)
            for method, restated, uniforms in (("stratified", rc.kernel_stratified, rc.uniforms),
                                               ("choice", rc.kernel_choice, rc.choice_uniforms)):
                uj = np.stack([uniforms(n, u) for u in us])
                out = _resample(ctx, particles, weights, uj, method=method)
                _assert_gathered(out, particles, weights, f"n={n} {method} u#{which}")
                for p, name in enumerate(names):
                    what = f"n={n} {name} u={us[p]!r} {method}"
                    want, clamped = restated(weights[p], uj[p])
                    np.testing.assert_array_equal(out["idx"][p], want, err_msg=what)
                    assert out["status"][p] == (lib.PT_RESAMPLE_CLAMP if clamped else 0), (what, out["status"][p])


@pytest.mark.parametrize("n", rc.COUNTS)
def test_fast_systematic_against_the_exact_answer(lib, n):
    """The fast arithmetic scans the raw weights with the DPP ladder and scales the positions instead (count_le_fast): no
    restatement, the rational answer.  NaN weights: no comparison succeeds, every output is the last source, flagged --
    as test_fused_step_edge_cases_match_staged states for its point 5 (the NaN bit itself is raised where a NaN
    particle is found, by the evolve kernels: nothing here evolves)."""
    names = [name for name, _ in _cases(n)]
    weights = np.stack([w for _, w in _cases(n)])
    P = len(names)
    particles = _particles(P, n)
    with lib.Context(P, n, 1, max_frames=2) as ctx:
        for which in range(4):
            us = _offsets(names, which)
            out = _resample(ctx, particles, weights, us, math="fast")
            _assert_gathered(out, particles, weights, f"n={n} fast u#{which}")
            for p, name in enumerate(names):
                what = f"n={n} {name} u={us[p]!r} fast"
                got, flagged = out["idx"][p], bool(out["status"][p] & lib.PT_RESAMPLE_CLAMP)
                assert out["status"][p] & ~lib.PT_RESAMPLE_CLAMP == 0, (what, out["status"][p])
                if rc.has_nan(weights[p]):
                    assert flagged and (got == n - 1).all(), what
                    continue
                exact = _exact_systematic(n, name, float(us[p]))
                if which < 2:
                    assert rc.decided(exact[1], n).all(), what
                    np.testing.assert_array_equal(got, exact[0], err_msg=what)
                    assert not flagged, what
                else:
                    rc.check_against_exact(got, exact, n, what)
                    if flagged:   # (recorded, not asserted: count_le_fast of the last cumulative weight may fall one short)
                        print(f"{what}: PT_RESAMPLE_CLAMP raised, last index {got[-1]}")


def test_largest_particle_count_and_one_more(lib):
    n = MAX_PARTICLES
    with pytest.raises(lib.GlhError):
        lib.Context(1, n + 1, 1, max_frames=2)
    w = np.full((1, n), rc.FLOOR)
    w[0, n - 1] = rc.SPIKE
    particles = _particles(1, n)
    with lib.Context(1, n, 1, max_frames=2) as ctx:
        for u in rc.U_DECIDED + rc.U_TIES:
            want, clamped = rc.kernel_systematic(w[0], u)
            for math in ("exact", "fast"):
                out = _resample(ctx, particles, w, np.array([u]), math=math)
                _assert_gathered(out, particles, w, f"n={n} u={u!r} {math}")
                if math == "exact":
                    np.testing.assert_array_equal(out["idx"][0], want, err_msg=repr(u))
                    assert bool(out["status"][0] & lib.PT_RESAMPLE_CLAMP) == clamped
                else:
                    rc.check_against_exact(out["idx"][0], rc.exact_systematic(w[0], u, reach=True), n, f"fast {u!r}")
            for method, restated in (("stratified", rc.kernel_stratified), ("choice", rc.kernel_choice)):
                uj = rc.uniforms(n, u)[None]
                out = _resample(ctx, particles, w, uj, method=method)
                np.testing.assert_array_equal(out["idx"][0], restated(w[0], uj[0])[0], err_msg=f"{method} {u!r}")


# ---- moments -----------------------------------------------------------------------------------------------------------
def moment_ceilings(n):
    """What the accumulation allows, in the units below (unit roundoff 2^-53; L = ceil(n / BLK) + log2(BLK): a thread's
    ceil(n / BLK) terms, then the 8 levels of the block sum).

    mean     m1 = S1 / s0, S1 = sum w d with d = x - K: each term carries 2 roundings (d, w d) and the sum L more, s0 another
             L, the division 1: (2 L + 3) eps max|d|.  Adding K rounds the RESULT by half an ulp: that is representation,
             not accumulation, and is taken out before the ratio is formed.
    variance var = m2 - m1^2.  m2 = S2 / s0 with 3 roundings per term: (2 L + 4) eps m2.  m1^2: twice the relative error
             of m1 against sum w |d| / s0, whose square is <= m2: (4 L + 7) eps m2.  The subtraction, the square root and
             the squaring of sigma here: 4 more.  m2 = sigma^2 + |K - mean|^2 exactly: (6 L + 15) eps (sigma^2 + d^2).
    """
    L = rc.segment(n) + 8
    return 2 * L + 3, 6 * L + 15


def _moment_ratios(particles, weights, out, what):
    """max over the points' six coordinates of the errors of mean and variance in the units of the model.  {point: (mean, var)}"""
    ratios = {}
    for p in range(len(weights)):
        idx = out["idx"][p]
        x, w = particles[p][idx], weights[p][idx]
        K = particles[p][idx[0]]                           # the kernels' pivot: the source of output 0
        mean, var = rc.moments_reference(x, w, origin=K)   # (the mean relative to the pivot)
        got_mean, got_sigma = out["moments"][p, 0:6], out["moments"][p, 6:12]
        assert np.isfinite(out["moments"][p]).all(), (what, p)
        span = np.abs(x - K).max(axis=0)
        err = np.abs((got_mean.astype(rc.LD) - K.astype(rc.LD)) - mean).astype(float)
        err = np.maximum(err - 0.5 * np.spacing(np.abs(K + mean.astype(float))), 0.0)   # (K + m1 rounds the result)
        assert (err[span == 0] == 0).all(), (what, p, "the mean of copies of the pivot is the pivot")
        r_mean = np.max(err[span > 0] / (EPS * span[span > 0]), initial=0.0)
        unit = EPS * (var + mean ** 2).astype(float)       # eps (sigma^2 + |K - mean|^2)
        verr = np.abs((got_sigma.astype(rc.LD) ** 2 - var).astype(float))
        assert (verr[unit == 0] == 0).all(), (what, p)
        r_var = np.max(verr[unit > 0] / unit[unit > 0], initial=0.0)
        ratios[p] = (float(r_mean), float(r_var))
    return ratios


# cloud -> (mean, variance): what is asserted, 4 x the maximum measured on an MI355X rounded up to a power of two and never
# above moment_ceilings(n) (INPUTS.md has the measured figures)
MOMENT_BOUNDS = {"cases": (16, 32), "survivor": (0, 0), "tight": (0.5, 16)}


def _assert_moments(cloud, n, ratios, labels):
    c_mean, c_var = moment_ceilings(n)
    b_mean, b_var = MOMENT_BOUNDS[cloud]
    b_mean, b_var = min(b_mean, c_mean), min(b_var, c_var)
    worst = (max(r[0] for r in ratios.values()), max(r[1] for r in ratios.values()))
    print(f"moments, cloud {cloud!r} n={n}: max ratio mean {worst[0]:.3g} (asserted {b_mean}, ceiling {c_mean}), "
          f"variance {worst[1]:.3g} (asserted {b_var}, ceiling {c_var})")
    for p, (rm, rv) in ratios.items():
        assert rm <= b_mean and rv <= b_var, (cloud, n, labels[p], rm, rv)


@pytest.mark.parametrize("n", (257, 1000, 5000))
def test_moments_of_the_designed_cases(lib, n):
    """Cloud (a): every designed weight set (the NaN sets apart: their moments are NaN), each at its first decided offset."""
    cases = [(name, w) for name, w in _cases(n) if not rc.has_nan(w)]
    names = [name for name, _ in cases]
    weights = np.stack([w for _, w in cases])
    particles = _particles(len(cases), n, seed=1)
    with lib.Context(len(cases), n, 1, max_frames=2) as ctx:
        out = _resample(ctx, particles, weights, _offsets(names, 0))
    _assert_moments("cases", n, _moment_ratios(particles, weights, out, f"cases n={n}"), names)


@pytest.mark.parametrize("n", (1000, 5000))
def test_moments_of_collapsed_and_tight_clouds(lib, n):
    """Clouds (b) and (c).  (b): one survivor (N copies: the true sigma is 0) with particle 0 moved 10 m, 1 km and 100 km from
    it in x and in y.  The pivot is the source of output 0 -- the survivor itself -- so every difference is 0: the mean is the
    survivor and sigma is 0, exactly.  (Around particle 0, as the kernels pivoted before, var = m2 - m1^2 left
    sqrt(eps) x distance: up to 1.08e-5 m at 1 km.)  (c): a cloud of spread 1e-3 m whose particle 0 is 100 m off and serves
    output 0: the pivot is 1e5 sigma from the mean, the error scales with that distance squared, not with sigma^2."""
    k = rc.spike_positions(n)["seg_last"]
    distances = (10.0, 1e3, 1e5)
    P = len(distances) + 1
    particles = _particles(P, n, seed=2)
    weights = np.full((P, n), rc.FLOOR)
    for p, dist in enumerate(distances):
        weights[p, k] = rc.SPIKE
        particles[p, 0] = particles[p, k]
        particles[p, 0, 0:2] += dist
    rng = np.random.default_rng(n)
    particles[3] = rng.standard_normal((n, 6)) * 1e-3 + CENTRE
    particles[3, 0, 0:3] += 100.0
    weights[3] = np.exp(-rng.random(n)) + rc.FLOOR
    weights[3, 0] = 1.0   # (the heaviest: it serves output 0 at u = 0.5)
    with lib.Context(P, n, 1, max_frames=2) as ctx:
        out = _resample(ctx, particles, weights, np.full(P, 0.5))
    for p, dist in enumerate(distances):
        assert (out["idx"][p] == k).all()
        print(f"one survivor, n={n}, particle 0 {dist:g} m away: sigma returned (x, y) = "
              f"{out['moments'][p, 6]:.3g}, {out['moments'][p, 7]:.3g} m (truth 0)")
        np.testing.assert_array_equal(out["moments"][p, 6:12], 0.0)
        np.testing.assert_array_equal(out["moments"][p, 0:6], particles[p, k])
    assert out["idx"][3][0] == 0
    ratios = _moment_ratios(particles, weights, out, f"far pivot n={n}")
    labels = [f"survivor {d:g} m" for d in distances] + ["tight"]
    _assert_moments("survivor", n, {p: ratios[p] for p in range(3)}, labels)
    _assert_moments("tight", n, {3: ratios[3]}, labels)


# ---- the fused kernel's phases D / E / F ----------------------------------------------------------------------------------
FT, FP = 3, 4            # frames, points
FSEED = 20261004         # of the device's Philox streams
DEM_SIGMA = 0.05         # s: a particle at z = 60 s has a DEM term of 1800 > 746 -- its weight is the 1e-300 floor in both arithmetics
# particle count -> (threads, particles in registers) by glh_point_plan.h: pt_shape, and what phase D does there
FUSED_COUNTS = {
    70: (512, 4),       # one segment element per thread, 442 idle threads
    1000: (512, 4),     # segments of 2 as 32-bit words, idle tail threads
    1023: (512, 4),     # odd: a last segment of 1, no word path
    1024: (512, 4),     # every thread a whole segment of 2
    2049: (512, 10),    # segments of 5
    5000: (512, 10),    # segments of 10, words, 12 idle threads
    5120: (512, 10),    # the aligned double2 segment path
    5121: (1024, 10),   # 1024 threads, segments of 6, the last of 3
}


def _survivor_sets(N, tb, math):
    """[[survivors (index array) of point p] for p < FP] per launch: one survivor at 0 / N - 1 / the edge of a thread segment
    of the fused kernel / 63 / 64, two at the ends, none (every weight at the floor: uniform), all (the control)."""
    first, last = rc.segment_edges(N, tb)
    edge = first if math == "exact" else last
    return {"a": [np.array([0]), np.array([N - 1]), np.array([edge]), np.arange(N)],
            "b": [np.array([63]), np.array([64]), np.array([0, N - 1]), np.array([], dtype=int)]}


def _fused_context(lib, cs, params, math, mode):
    ctx = lib.Context(cs["P"], cs["N"], 1, max_tile=31, max_search_dim=160, max_frames=FT)
    ctx.observer_init(0, FT, cs["imgsz"][0], cs["imgsz"][1], 1, cs["sigmas"][0])
    ctx.observer_set_cameras(0, np.tile(cs["cams"][0], (FT, 1)))
    for t in range(FT):
        ctx.observer_upload_frame(0, t, cs["frames"][0][t])
    ctx.begin_sequence(cs["P"], cs["N"], lc.TILE)
    ctx.set_motion_cartesian(params)
    ctx.set_math(math)
    ctx.set_fused(mode)
    ctx.set_debug(2)  # keeps the resample indices; the step stays on the fused kernel
    return ctx


def _start(ctx, survivors):
    """The prior with its heights forced: the survivors at z = 0, every other particle at z = 60 s, no vertical velocity."""
    ctx.set_frame(0)
    ctx.init_particles(seed=FSEED)
    p0 = ctx.get_particles()
    p0[:, :, 2] = 60.0 * DEM_SIGMA
    p0[:, :, 5] = 0.0
    for p, keep in enumerate(survivors):
        p0[p, keep, 2] = 0.0
    ctx.set_particles(p0)
    ctx.init_templates(0, 0)
    ctx.record_moments(0)
    return p0


def _fused_run(lib, cs, params, math, mode, survivors):
    """As tests/test_gpu_uniform_work.py: _run -- the state read after every step, the sequence started again for every stop."""
    out = dict(particles=[], weights=[], idx=[], variants=[])
    with _fused_context(lib, cs, params, math, mode) as ctx:
        for stop in range(1, FT):
            _start(ctx, survivors)
            for i in range(1, stop + 1):
                ctx.step(i, 1.0, [i], seed=FSEED)
                if stop == FT - 1:
                    out["idx"].append(ctx.resample_indices())
                    out["variants"].append(ctx.last_variant())
            out["particles"].append(ctx.get_particles())
            out["weights"].append(ctx.get_weights())
        out["moments"] = ctx.get_moments(0, FT)
        out["status"] = ctx.point_status()
        out["obs"] = ctx.observer_status_frames(1, FT - 1)
    return out


def _staged_by_hand(lib, cs, params, math, survivors):
    """The staged kernels stage by stage, to capture what the resampling is given: the weights after update_weights and the
    offset u of the device stream, per step."""
    out = dict(particles=[], weights=[], idx=[], w_in=[], u=[])
    with _fused_context(lib, cs, params, math, 0) as ctx:
        _start(ctx, survivors)
        for i in range(1, FT):
            ctx.set_frame(i)
            ctx.evolve(1.0, seed=FSEED, step=i)
            ctx.update_weights([i])
            out["w_in"].append(ctx.get_weights())
            out["u"].append(ctx.debug_draws("u", FSEED, step=i))
            ctx.resample(seed=FSEED, step=i)
            out["idx"].append(ctx.resample_indices())
            out["particles"].append(ctx.get_particles())
            out["weights"].append(ctx.get_weights())
        out["status"] = ctx.point_status()
    return out


def _check_forced_survivors(lib, N, math, group):
    tb, ppt = FUSED_COUNTS[N]
    survivors = _survivor_sets(N, tb, math)[group]
    cs = lc.multi_observer_case(1, T=FT, P=FP, N=N)
    params = cs["params"].copy()
    params[:, 6] = params[:, 12] = params[:, 15] = 0.0   # no vertical velocity, acceleration or acceleration noise: z stays
    params[:, 16], params[:, 17] = 0.0, DEM_SIGMA
    what = f"N={N} {math} group {group}"
    fused = _fused_run(lib, cs, params, math, 1, survivors)
    staged = _fused_run(lib, cs, params, math, 0, survivors)
    hand = _staged_by_hand(lib, cs, params, math, survivors)

    # the launch shape and the code of every step
    want = [(tb, ppt, 1) + lc.expected_code("plain", math, s, 1) for s in range(1, FT)]
    assert [tuple(v[:3]) + lc.flags_to_code(v[3]) for v in fused["variants"]] == want, (what, fused["variants"])
    assert all(tuple(v) == (0, 0, 0, 0) for v in staged["variants"]), (what, staged["variants"])
    # fused == staged == the staged kernels called one by one, bit for bit after every step
    np.testing.assert_array_equal(fused["status"], staged["status"], err_msg=what)
    np.testing.assert_array_equal(hand["status"], staged["status"], err_msg=what)
    np.testing.assert_array_equal(fused["obs"], staged["obs"], err_msg=what)
    assert (staged["obs"] == lib.OBS_OK).all(), (what, staged["obs"])
    for s in range(FT - 1):
        for other, label in ((fused, "fused"), (hand, "stage by stage")):
            msg = f"{what}: {label} against staged, step {s + 1}"
            np.testing.assert_array_equal(other["idx"][s], staged["idx"][s], err_msg=msg)
            np.testing.assert_array_equal(other["particles"][s], staged["particles"][s], err_msg=msg)
            np.testing.assert_array_equal(other["weights"][s], staged["weights"][s], err_msg=msg)
    np.testing.assert_allclose(fused["moments"], staged["moments"], rtol=1e-12, atol=1e-13, err_msg=what)
    assert np.isfinite(fused["moments"]).all(), what
    # one survivor: frame 1's cloud is N copies of one particle, and the pivot is that particle -- sigma is 0, the mean the
    # particle, exactly, in both kernels
    for p, keep in enumerate(survivors):
        if len(keep) == 1:
            for run, label in ((fused, "fused"), (staged, "staged")):
                np.testing.assert_array_equal(run["moments"][1, p, 6:12], 0.0, err_msg=f"{what} {label} point {p}")
                np.testing.assert_array_equal(run["moments"][1, p, 0:6], run["particles"][0][p][0],
                                              err_msg=f"{what} {label} point {p}")

    # the indices against the restatement (exact) / the rational answer (fast) on the captured weights and offsets
    clamps = False
    for s in range(FT - 1):
        for p in range(FP):
            w, u, got = hand["w_in"][s][p], float(hand["u"][s][p]), fused["idx"][s][p]
            msg = f"{what}: step {s + 1} point {p} u={u!r}"
            assert np.isfinite(w).all() and (w >= rc.FLOOR).all(), msg
            if math == "exact":
                idx, clamped, contested = rc.kernel_systematic(w, u, contested=True)
                np.testing.assert_array_equal(got[~contested], idx[~contested], err_msg=msg)
                clamps |= clamped
            else:
                rc.check_against_exact(got, rc.exact_systematic(w, u, reach=True), N, msg)
    if math == "exact":
        assert bool((fused["status"] & lib.PT_RESAMPLE_CLAMP).any()) == clamps, (what, fused["status"])
    assert ((fused["status"] & ~np.uint32(lib.PT_RESAMPLE_CLAMP)) == 0).all(), (what, fused["status"])

    # the survivors: the forced weights did what they were meant to
    for p, keep in enumerate(survivors):
        w, idx = hand["w_in"][0][p], fused["idx"][0][p]
        lifted = np.setdiff1d(np.arange(N), keep)
        assert (w[lifted] == rc.FLOOR).all(), (what, p)
        if len(keep):
            assert (w[keep] > 1e-250).all(), (what, p, w[keep].min())
            assert np.isin(idx, keep).all(), (what, p)
        if len(keep) == 1:   # N copies of one record
            assert (idx == keep[0]).all(), (what, p)
            assert (fused["particles"][0][p] == fused["particles"][0][p][0]).all(), (what, p)
        elif len(keep) == 2:
            assert set(np.unique(idx)) <= {0, N - 1} and (np.diff(idx) >= 0).all(), (what, p)
        elif len(keep) == 0:  # uniform weights at the floor: every particle once (u is not a tie)
            np.testing.assert_array_equal(idx, np.arange(N), err_msg=f"{what} point {p}")


@pytest.mark.parametrize("group", ("a", "b"))
@pytest.mark.parametrize("math", ("exact", "fast"))
@pytest.mark.parametrize("N", sorted(FUSED_COUNTS))
def test_fused_resampling_with_forced_survivors(lib, N, math, group):
    _check_forced_survivors(lib, N, math, group)
