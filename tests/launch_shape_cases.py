"""The launch shapes of the fused frame step and the recipe that runs every instantiation of each (a plain helper module).

glh_point_variants.h carries 11 launch shapes (threads, particles of observer 0 in registers, observers) with 8 codes
(SURF, FAST, CON) each; glh_point_plan.h: pt_shape picks the shape from the particle count N and the observer count O,
pt_code the code from the context's configuration and what the launch is given, pt_plan whether the fused kernel takes
the count at all (tests/test_hostcheck.py runs the three, compiled for the CPU, against this module).  This module names

  * SHAPES: for every shape the particle counts at which its own edges show (tests/test_gpu_launch_shapes.py runs them;
    tests/test_hostcheck.py pins the same N -> shape map on the host);
  * CONFIGS x MATHS and `expected_code`: three configurations, two arithmetics and T = 4 frames on the device's Philox
    draws reach all eight codes of a shape;
  * `flags_to_code`: the flags of Context.last_variant() as the (SURF, FAST, CON) triple of glh_point_variants.h;
  * `multi_observer_case`: the scene -- one to four stations around one textured surface, 512 x 512 frames, 21 x 21 templates;
  * ORACLE_CASES and `admit`: the five 1024-thread shapes no other test launches, compared with the oracle index for
    index, and the rule that admits their seeds (as tests/option_cases.py: the oracle alone, with both accumulations of
    the SSD, before anything runs on a GPU).
"""
import functools
import warnings

import numpy as np

# ---- the shapes ------------------------------------------------------------------------------------------------------
# (threads, PPT, observers) -> particle counts.  What each count is the edge of:
#   2048 / 2049    the last count with 4 particles per thread in registers / the first with 10
#   5120 / 5121    the last count of the 512-thread kernel (ten full passes) / one particle into a sixth pass of 1 024
#                  lanes, almost every lane idle
#   10240          the 1 024-thread kernel exactly full: the last count with observer 0's coordinates in registers
#   10241          the first count that parks observer 0's coordinates (u in c[], v in the uv scratch)
#   10500          the count tests/test_hostcheck.py pins; c[N] + region 2 within 4 KB of the LDS limit with rasters
# Every count is accepted by pt_plan for every configuration below (21 x 21 templates, one channel: c[N], the pairwise-sum
# plan and the three rank tables of phase D/E take 14 N + ~2 KB of the 152 KB - PT_PATCH_LDS a workgroup may have -- N up to
# ~10 700 with rasters), so no entry had to settle for a smaller count:
# tests/test_hostcheck.py: test_launch_shape_table_counts_are_accepted_by_the_plan asserts it.
SHAPES = (
    ((512, 4, 1), (2048,)),
    ((512, 10, 1), (2049, 5120)),
    ((1024, 10, 1), (5121, 10240)),
    ((1024, 0, 1), (10241, 10500)),
    ((512, 10, 2), (5120,)),
    ((1024, 10, 2), (5121, 10240)),
    ((1024, 0, 2), (10241,)),
    ((512, 0, 3), (5120,)),
    ((512, 0, 4), (5120,)),
    ((1024, 0, 3), (5121, 10500)),
    ((1024, 0, 4), (5121, 10500)),
)
# (shape, code) pairs no particle count reaches, with the line of pt_plan / pt_code that excludes them: none.  The
# coverage assertions count an entry here as accounted for.
UNREACHABLE = {}

T, P = 4, 2          # frames, points of the fused-against-staged runs
TILE = (21, 21)
SEED = 7             # of the device's Philox streams
CONFIGS = ("plain", "general", "rasters")
MATHS = ("exact", "fast")


def entries():
    """[(shape, N)] in the table's order."""
    return [(shape, n) for shape, counts in SHAPES for n in counts]


def flags_to_code(flags):
    """Context.last_variant()[3] (bit 0 fast arithmetic, bit 1 the general code, bit 2 the contract, bit 3 the raster
    samples) as the (SURF, FAST, CON) triple of glh_point_variants.h -- glh_point_plan.h: pt_code returns both, the
    triple as (rast ? 2 : surf ? 1 : 0, fast, surf ? common : fast)."""
    fast, surf, common, rast = (bool(flags & b) for b in (1, 2, 4, 8))
    return (2 if rast else 1 if surf else 0, int(fast), int(common if surf else fast))


def missing_image(step, n_obs):
    """Frame 2 has the last observer without an image when there is more than one."""
    return n_obs > 1 and step == 2


def expected_code(config, math, step, n_obs):
    """The code pt_code selects for frame `step` (1 ..) of a run from init_particles(seed=...) on device draws.

    Fast arithmetic runs under the contract (`common`) when the input is the compact state a fused step left and every
    observer has an image: not on frame 1 (the expanded prior) and not on the frame with the missing image."""
    fast = math == "fast"
    common = fast and step >= 2 and not missing_image(step, n_obs)
    rast = config == "rasters"
    surf = rast or config == "general" or (fast and not common)
    return (2 if rast else 1 if surf else 0, int(fast), int(common if surf else fast))


def instantiations(shape):
    """Every (tb, ppt, O, S, F, C) the recipe runs on a shape."""
    return {tuple(shape) + expected_code(config, math, step, shape[2])
            for config in CONFIGS for math in MATHS for step in range(1, T)}


def covered():
    return set().union(*(instantiations(shape) for shape, _ in SHAPES))


# ---- the scene -------------------------------------------------------------------------------------------------------
IMGSZ = (512, 512)


def _cameras():
    from glimpse_amd import synth

    return [synth.nadir_camera(IMGSZ, f=1000.0, height=100.0, k=(0.05, -0.01, 0.002, 0, 0, 0)),
            synth.pack_camera(imgsz=IMGSZ, f=1200.0, k=(0.03, 0, 0), xyz=(40, -30, 90), viewdir=(-53.13, -60.9, 0)),
            synth.nadir_camera(IMGSZ, f=850.0, height=110.0, k=(0.02, 0, 0, 0, 0, 0), xyz_offset=(4.0, -3.0)),
            synth.pack_camera(imgsz=IMGSZ, f=1100.0, k=(0, 0, 0), xyz=(-35, 25, 95), viewdir=(125.5, -65.6, 0))]


@functools.lru_cache(maxsize=8)
def _station_frames(o, n_frames, seed):
    """The frames of station o (the scene is laid out under station 0 whatever the number of stations): rendered once."""
    from glimpse_amd import synth

    cams = _cameras()
    scene = synth.default_scene(cams[0], seed=seed, velocity=(0.15, 0.0), n_frames=n_frames, margin=60.0)
    return tuple(scene.render(cams[o], float(t)) for t in range(n_frames))


def multi_observer_case(O, T=4, P=3, N=1500, seed=5):
    """O stations around one scene (a nadir camera with k1-k3, the oblique station of C5, a second nadir station off to
    the side with another focal length, a second oblique station), points every one of them sees."""
    from glimpse_amd import synth

    imgsz = IMGSZ
    cams = _cameras()[:O]
    frames = [list(_station_frames(o, T, seed)) for o in range(O)]
    rng = np.random.default_rng(seed)
    xy = []
    while len(xy) < P:
        cand = rng.uniform(-6, 6, 2)
        uv = [synth.project(cam, np.array([[cand[0], cand[1], 0.0]]))[0] for cam in cams]
        if all(90 < u[0] < imgsz[0] - 90 and 90 < u[1] < imgsz[1] - 90 for u in uv):
            xy.append(cand)
    params = np.zeros((P, 18))
    params[:, 0:2] = xy
    params[:, 2:4] = 0.15
    params[:, 4:7] = (0.15, 0.0, 0.0)
    params[:, 7:10] = (0.1, 0.1, 0.03)
    params[:, 13:16] = (0.04, 0.04, 0.01)
    params[:, 17] = 0.4
    return dict(cams=cams, frames=frames, params=params, imgsz=imgsz, T=T, P=P, N=N, sigmas=[0.3, 0.45, 0.35, 0.5][:O])


def configuration(cs, config):
    """What a configuration sets on top of the scene: dict(motion=[P][18] Cartesian table or [P][24] table of glh_set_motion,
    rasters=None or (x limits, y limits, dem values, dem_sigma values)).

    plain    Cartesian motion (a constant DEM term), uint8 frames, 5 x 5 median, bicubic sampling.
    general  point 0 on TangentCartesianMotion over constant surfaces: the general code.
    rasters  gridded dem / dem_sigma as in test_tangent_models_over_rasters_with_three_observers: point 0 on
             TangentCartesianMotion (its evolved height parked for the gather), point 1 Cartesian with the DEM term
             sampled from the rasters."""
    if config == "plain":
        return dict(motion=cs["params"], rasters=None)
    P = cs["P"]
    params = np.zeros((P, 24))
    params[:, :18] = cs["params"]
    params[0, 18] = 2      # TangentCartesianMotion
    params[:, 19] = 0.05   # slope_sigma
    if config == "general":
        return dict(motion=params, rasters=None)
    assert config == "rasters"
    params[:, 20:22] = 1.0
    rng = np.random.default_rng(31)
    xy = cs["params"][:, 0:2]
    lo, hi = xy.min(axis=0) - 60.0, xy.max(axis=0) + 60.0
    nx, ny = 57, 49
    return dict(motion=params, rasters=((lo[0], hi[0]), (hi[1], lo[1]), 0.03 * rng.standard_normal((ny, nx)),
                                        0.2 + 0.1 * rng.random((ny, nx))))


# ---- the five shapes no other test launches, against the oracle ---------------------------------------------------------
# shape -> dict(N, P, scene seed).  T = 3.  The counts: the largest of the table for each shape (every pass of the particle
# loops full or nearly so, the LDS plan at its tightest).  The scene seed is the first, counting up from 5 (the sibling
# tests' scene), that `admit` accepts; the host-fed draws are seeded with N + O.
ORACLE_T = 3
ORACLE_CASES = {
    (1024, 0, 1): dict(N=10500, P=2, seed=5),
    (1024, 0, 2): dict(N=10241, P=2, seed=5),
    (1024, 0, 3): dict(N=10500, P=2, seed=5),
    (1024, 0, 4): dict(N=10500, P=2, seed=6),  # (seed 5: one index of 42 000 hinges on the accumulation order of the SSD)
    (1024, 10, 2): dict(N=10240, P=2, seed=5),
}


def oracle_case(shape):
    """The scene of an oracle-compared shape with its host-fed draws (init (P, N, 6), evolve (T - 1, P, N, 3), u (T - 1, P))."""
    q = ORACLE_CASES[tuple(shape)]
    O = shape[2]
    cs = multi_observer_case(O, T=ORACLE_T, P=q["P"], N=q["N"], seed=q["seed"])
    rng = np.random.default_rng(q["N"] + O)
    cs["draws"] = (rng.standard_normal((q["P"], q["N"], 6)), rng.standard_normal((ORACLE_T - 1, q["P"], q["N"], 3)),
                   rng.random((ORACLE_T - 1, q["P"])))
    return cs


def oracle_tracks(cs, draws, ssd="row_f32"):
    """oracle.tracker.track_one over every point of a case on the given draws, every station with an image on every frame.
    Returns dict(means (T, P, 6), sigmas (T, P, 6), idx (T - 1, P, N), clean): `clean` -- no search box left its frame."""
    from oracle import motion as omotion
    from oracle import tracker as otracker

    n_frames, n_obs, N = cs["T"], len(cs["cams"]), cs["N"]
    init, ev, us = draws
    observers = [otracker.Observer(cs["frames"][o], np.tile(cs["cams"][o], (n_frames, 1)), cs["sigmas"][o], ssd=ssd)
                 for o in range(n_obs)]
    matching = np.tile(np.arange(n_frames)[:, None], (1, n_obs))
    means, sigmas, idx = [], [], []
    clean = True
    for p in range(cs["P"]):
        q = cs["params"][p]
        model = omotion.CartesianMotion(xy=q[0:2], xy_sigma=q[2:4], vxyz=q[4:7], vxyz_sigma=q[7:10], axyz=q[10:13],
                                        axyz_sigma=q[13:16], dem=q[16], dem_sigma=q[17], n=N)
        d = {"init": init[p], "evolve": [ev[s, p] for s in range(n_frames - 1)], "u": [us[s, p] for s in range(n_frames - 1)]}
        trace = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref = otracker.track_one(model, observers, matching, np.ones(n_frames - 1), tile_size=TILE, draws=d, trace=trace)
        steps = [tr for tr in trace if "idx" in tr]
        assert len(steps) == n_frames - 1
        clean &= all("sse" in ot for tr in steps for ot in tr["obs"])
        means.append(ref["means"])
        sigmas.append(ref["sigmas"])
        idx.append(np.stack([tr["idx"] for tr in steps]))
    return dict(means=np.stack(means, axis=1), sigmas=np.stack(sigmas, axis=1), idx=np.stack(idx, axis=1), clean=clean)


def admit(shape):
    """The admission rule of tests/option_cases.py for an oracle-compared shape: its host-fed draws through the oracle with
    the SSD accumulated in float64 and with the kernels' row-wise float32 accumulation.  dict(ok, why, ref): admitted only
    if both give the same resample indices at every step of every point and no search box leaves its frame; `ref` is the
    row_f32 run."""
    cs = oracle_case(shape)
    runs = {ssd: oracle_tracks(cs, cs["draws"], ssd) for ssd in ("f64", "row_f32")}
    if not all(r["clean"] for r in runs.values()):
        return dict(ok=False, why="a search box leaves its frame")
    n_diff = int((runs["f64"]["idx"] != runs["row_f32"]["idx"]).sum())
    if n_diff:
        return dict(ok=False, why=f"{n_diff} resample indices depend on the accumulation order of the SSD")
    if not all(np.isfinite(runs["row_f32"][k]).all() for k in ("means", "sigmas")):
        return dict(ok=False, why="moments are not finite")
    return dict(ok=True, why="", ref=runs["row_f32"])
