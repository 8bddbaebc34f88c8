"""Seeded cases over the tracker's option space, and the rule that admits them (a plain helper module).

`case(seed)` is built like `_random_case` of tests/test_gpu_random_sweep.py and varies what that one varies (camera
model, template shape, particle count, time steps, one or two observers with a missing image); on top of it
  * the frame type: uint8 / uint16 / float32 / float64, one or three channels; the 16-bit frames are synth's 16-bit
    rendering, the float frames a fixed map of it; a share of the 16-bit cases is squeezed into 300 levels (fewer than the
    1024 buckets of the ranking), a share of the float cases is quantised first (repeated values inside a template);
  * the median window: rows and columns from {1, 3, 5, 7}, never (1, 1), and scipy.ndimage's four boundary modes;
  * the spline orders (kx, ky), each 1 .. 5: a little over half of the cases (3, 3) or (1, 1), which the fused kernel takes;
  * the motion model: the four of oracle/motion.py on constant surfaces, a DEM term in a share of the Cartesian /
    Cylindrical ones;
  * the template: odd, even and non-square sides 7 .. 47, a few cases with sides in 49 .. 63, a few above 63 (staged kernels);
  * cloud-width cases: sigmas wide enough that the SSD surface exceeds 40 cells on a side (the banded spline fit).
N comes from the sweep's list, P = 3, T = 4, frames of 300 .. 520 pixels.

`admit(seed)` is the admission rule, evaluated by the oracle alone: the case's host-fed draws run twice, with the SSD
accumulated in float64 and with the kernels' row-wise float32 accumulation (oracle/ssd.py), and the seed is admitted only if
both runs give the same resample indices at every step of every point, no track raises and no search box leaves its
frame.  A case whose indices hinge on the accumulation order of the SSD says nothing about the kernels.  `admitted(n)`
walks the seeds upwards from 0 and skips those the rule refuses; SEEDS is that list, committed, and
tests/test_option_cases.py checks that the rule still yields it.
"""
import functools
import warnings

import numpy as np

FRAME_TYPES = ("uint8", "uint16", "float32", "float64")
MODES = ("reflect", "nearest", "mirror", "wrap")
WINDOWS = (1, 3, 5, 7)
KINDS = ("cartesian", "cylindrical", "tangent_cartesian", "tangent_cylindrical")
N_CHOICES = (37, 64, 100, 513, 777, 1500, 2049, 3000)
FUSED_ORDERS = ((3, 3), (1, 1))
P, T = 3, 4

# the first forty seeds the rule admits (tests/test_option_cases.py: the rule run again gives this list)
SEEDS = tuple(range(40))


def float_map(frame16, dtype):
    """The float frame of a 16-bit rendering: a reflectance-like curve into (-1.25, 2.25) (the map of the float goldens'
    scenes, tests/test_oracle_golden.py: float64_scene)."""
    return (np.power(frame16.astype(np.float64) / 65535.0, 0.8) * 3.5 - 1.25).astype(dtype)


def render(scene, cam, t, ftype, channels, levels):
    """The frame of a scene at time t in one of FRAME_TYPES: synth's 8-bit rendering, its 16-bit one (whole, squeezed into
    300 levels offset from zero, or quantised to 300 steps), or float_map of the latter."""
    if ftype == "uint8":
        return scene.render(cam, float(t), channels=channels)
    f = scene.render(cam, float(t), channels=channels, bits=16)
    if levels == "300":  # a narrow range of levels, offset from zero
        return (f.astype(np.uint32) * 300 // 65535 + 1000).astype(np.uint16)
    if levels == "quantised":
        f = (f.astype(np.uint32) * 300 // 65535 * 218).astype(np.uint16)
    return f if ftype == "uint16" else float_map(f, np.dtype(ftype))


def _orders(seed, fused):
    if fused:
        return FUSED_ORDERS[(seed // 2 + seed // 10) % 2]
    kx, ky = 1 + (2 * seed + seed // 5) % 5, 1 + (3 * seed + seed // 7) % 5
    if (kx, ky) in FUSED_ORDERS:
        ky = ky % 5 + 1
    return kx, ky


def _tile(seed, rng):
    """(width, height) and its class."""
    a, b = int(rng.integers(7, 48)), int(rng.integers(7, 48))
    shape = int(rng.integers(0, 4))
    if seed % 16 == 9:
        return (int(rng.integers(64, 72)), int(rng.integers(20, 40))), "above 63"
    if seed % 10 == 3:
        return ((int(rng.integers(49, 64)), b) if seed % 20 == 3 else (a | 1, int(rng.integers(49, 64)))), "49 .. 63"
    if seed % 16 == 4:  # (the cloud-width cases: a small template keeps the search tile inside the workspace)
        return (min(a, 25), min(b, 25)), "non-square" if min(a, 25) != min(b, 25) else ("odd" if min(a, 25) % 2 else "even")
    if shape == 0:
        return (a | 1, a | 1), "odd"
    if shape == 1:
        return (a + a % 2, a + a % 2), "even"
    if a == b:
        b = b + 1 if b < 47 else b - 1
    return (a, b), "non-square"


def options(seed):
    """The option axes of a seed (cheap: no frames are rendered)."""
    rng = np.random.default_rng(2000 + seed)
    ftype = FRAME_TYPES[seed % 4]
    mode = MODES[(seed // 4) % 4]
    channels = 3 if rng.random() < 0.4 else 1
    window = (1, 1)
    while window == (1, 1):
        window = (int(rng.choice(WINDOWS)), int(rng.choice(WINDOWS)))  # scipy order: (rows, columns)
    wide = seed % 16 == 4
    kind = 0 if wide else int(rng.integers(0, 4))
    has_z = bool(rng.random() < 0.4)  # Cartesian / Cylindrical: a DEM term; tangent models: a z offset at the start
    tile, tile_class = _tile(seed, rng)
    fused_orders = ((seed // 4 + seed + seed // 16) % 2 == 0 or seed % 8 == 5) and tile_class != "above 63"
    interp = _orders(seed, fused_orders)
    levels = "full"
    if ftype == "uint16" and (seed // 4) % 3 == 0:
        levels = "300"
    if ftype in ("float32", "float64") and (seed // 4) % 3 == 1:
        levels = "quantised"
    N = int(N_CHOICES[(5 * seed + seed // 8) % 8])
    return dict(ftype=ftype, mode=mode, channels=channels, window=window, wide=wide, kind=kind, has_z=has_z, tile=tile,
                tile_class=tile_class, interp=interp, levels=levels, N=N)


@functools.lru_cache(maxsize=2)
def case(seed):
    from glimpse_amd import synth

    rng = np.random.default_rng(1000 + seed)
    imgsz = (int(rng.integers(300, 520)), int(rng.integers(300, 520)))
    n_obs = 1 if seed % 3 else 2
    # ---- cameras: as in the random sweep
    k = np.zeros(6)
    nk = int(rng.integers(0, 4))
    k[:nk] = rng.uniform(-0.05, 0.05, nk) * np.array([1.0, 0.3, 0.05])[:nk]
    if seed % 5 == 0:
        nden = int(rng.integers(1, 4))
        k[3:3 + nden] = rng.uniform(-0.01, 0.01, nden)
    p = rng.uniform(-0.002, 0.002, 2) if seed % 4 == 1 else np.zeros(2)
    c = rng.uniform(-6, 6, 2) if seed % 2 else np.zeros(2)
    correction = bool(seed % 7 == 3)
    cam0 = synth.pack_camera(imgsz=imgsz, f=(float(rng.uniform(700, 1100)), float(rng.uniform(700, 1100))), c=c, k=k,
                             p=p, xyz=(float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), 100.0),
                             viewdir=(float(rng.uniform(-20, 20)), -90.0 + float(rng.uniform(0, 4)), 0.0),
                             correction=correction)
    cams = [cam0]
    if n_obs == 2:
        cams.append(synth.pack_camera(imgsz=imgsz, f=900.0, k=(0.02, 0, 0), xyz=(12.0, -9.0, 95.0),
                                      viewdir=(-53.13, -82.0, 0.0)))
    opt = options(seed)
    ftype, mode, channels, window, wide, kind, has_z = (opt[k] for k in ("ftype", "mode", "channels", "window", "wide",
                                                                          "kind", "has_z"))
    tile, tile_class, interp, levels, N = (opt[k] for k in ("tile", "tile_class", "interp", "levels", "N"))
    # ---- frames
    velocity = (float(rng.uniform(0.05, 0.25)), float(rng.uniform(-0.1, 0.1)))
    scene = synth.default_scene(cams[-1], seed=seed, velocity=velocity, n_frames=T, margin=40.0)
    taus = np.array([1.0, float(rng.choice([1.0, 0.5, 1.5])), 1.0])
    times = np.concatenate(([0.0], np.cumsum(taus)))
    if seed % 6 == 4:
        taus, times = -taus, -times

    frames = [[render(scene, cam, t, ftype, channels, levels) for t in times] for cam in cams]
    # ---- points every camera sees with room for the template and the search tile
    xy = []
    margin = 0.5 * max(tile) + (75.0 if wide else 45.0)
    tries = 0
    while len(xy) < P:
        tries += 1
        assert tries < 10000
        cand = np.array([rng.uniform(-14, 14), rng.uniform(-14, 14)])
        ok = True
        for cam in cams:
            uv = synth.project(cam, np.array([[cand[0], cand[1], 0.0]]))[0]
            ok &= bool(margin < uv[0] < cam[6] - margin and margin < uv[1] < cam[7] - margin)
        if ok:
            xy.append(cand)
    # ---- motion: the [P][24] table of glh_set_motion (include/glimpse_hip.h)
    sign = np.sign(taus[0])
    v = np.array(velocity) * sign
    z = (0.03, 0.01) if has_z else (0.0, 0.0)  # sigmas of the vertical velocity and acceleration
    params = np.zeros((P, 24))
    params[:, 0:2] = xy
    params[:, 2:4] = 0.6 if wide else 0.15
    params[:, 18] = kind
    if kind in (0, 2):
        params[:, 4:6] = v
        params[:, 7:9] = 0.5 if wide else 0.1
        params[:, 13:15] = 0.04
    else:  # (radius rate, theta) instead of (vx, vy)
        params[:, 4:6] = (np.hypot(*v), np.arctan2(v[1], v[0]))
        params[:, 7:9] = (0.08, 0.4)
        params[:, 13:15] = (0.03, 0.05)
    if kind < 2:
        params[:, 9], params[:, 15] = z
        params[:, 17] = 0.4 if has_z else 0.0
    else:
        params[:, 17] = 0.2 if has_z else 0.0
        params[:, 19] = 0.05  # slope_sigma
    matching = np.tile(np.arange(T)[:, None], (1, n_obs))
    if n_obs == 2 and seed % 2 == 0:
        matching[2, 1] = -1  # the second station has no image for frame 2
    sigmas = [0.3, 0.45][:n_obs]
    host = np.random.default_rng(seed)
    draws = dict(init=host.standard_normal((P, N, 6)), evolve=host.standard_normal((T - 1, P, N, 3)),
                 u=host.random((T - 1, P)))
    return dict(seed=seed, imgsz=imgsz, cams=cams, frames=frames, channels=channels, dtype=np.dtype(ftype), ftype=ftype,
                levels=levels, window=window, mode=mode, interp=interp, kind=kind, has_z=has_z, tile=tile,
                tile_class=tile_class, wide=wide, N=N, P=P, T=T, params=params, matching=matching, taus=taus,
                sigmas=sigmas, draws=draws, max_tile=max(31, max(tile)), max_search_dim=160 if max(tile) <= 63 else 192)


def axes(cs):
    """The axis values of a case, for the coverage count."""
    return {"frame type": cs["ftype"], "channels": cs["channels"], "window rows": cs["window"][0],
            "window columns": cs["window"][1], "boundary mode": cs["mode"], "kx": cs["interp"][0], "ky": cs["interp"][1],
            "fused orders": cs["interp"] in FUSED_ORDERS, "motion model": KINDS[cs["kind"]],
            "dem term": bool(cs["kind"] < 2 and cs["has_z"]), "template": cs["tile_class"], "N": cs["N"],
            "observers": len(cs["cams"])}


AXIS_VALUES = {"frame type": FRAME_TYPES, "channels": (1, 3), "window rows": WINDOWS, "window columns": WINDOWS,
               "boundary mode": MODES, "kx": (1, 2, 3, 4, 5), "ky": (1, 2, 3, 4, 5), "fused orders": (False, True),
               "motion model": KINDS, "dem term": (False, True), "template": ("odd", "even", "non-square", "49 .. 63"),
               "N": N_CHOICES, "observers": (1, 2)}


def oracle_model(cs, p):
    """The oracle's motion model of point p."""
    from oracle import motion as omotion

    q, n = cs["params"][p], cs["N"]
    if q[18] < 2:
        cls = omotion.CartesianMotion if q[18] == 0 else omotion.CylindricalMotion
        return cls(xy=q[0:2], xy_sigma=q[2:4], vxyz=q[4:7], vxyz_sigma=q[7:10], axyz=q[10:13], axyz_sigma=q[13:16],
                   dem=q[16], dem_sigma=q[17], n=n)
    cls = omotion.TangentCartesianMotion if q[18] == 2 else omotion.TangentCylindricalMotion
    return cls(xy=q[0:2], xy_sigma=q[2:4], vxy=q[4:6], vxy_sigma=q[7:9], axy=q[10:12], axy_sigma=q[13:15], dem=q[16],
               dem_sigma=q[17], n=n, slope_sigma=q[19])


def oracle_observers(cs, ssd):
    from oracle import tracker as otracker

    return [otracker.Observer(cs["frames"][o], np.tile(cs["cams"][o], (cs["T"], 1)), cs["sigmas"][o], interp=cs["interp"],
                              ssd=ssd, highpass_size=cs["window"], highpass_mode=cs["mode"]) for o in range(len(cs["cams"]))]


def oracle_run(cs, ssd, n_frames=None):
    """The oracle's whole tracks of a case on its host-fed draws: per point the result of track_one and its trace; an
    exception (a template box off the frame, NaN particles) propagates."""
    from oracle import tracker as otracker

    n = cs["T"] if n_frames is None else n_frames
    observers = oracle_observers(cs, ssd)
    out = []
    for p in range(cs["P"]):
        d = cs["draws"]
        draws = {"init": d["init"][p], "evolve": [d["evolve"][s, p] for s in range(n - 1)],
                 "u": [d["u"][s, p] for s in range(n - 1)]}
        trace = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = otracker.track_one(oracle_model(cs, p), observers, cs["matching"][:n], cs["taus"][:n - 1],
                                     tile_size=cs["tile"], draws=draws, trace=trace)
        out.append((res, trace))
    return out


def _clean(cs, run):
    """Every image the matching names was used: no search box left its frame."""
    for _, trace in run:
        steps = [tr for tr in trace if "idx" in tr]
        if len(steps) != cs["T"] - 1:
            return False
        for tr in steps:
            for o, ot in enumerate(tr["obs"]):
                if cs["matching"][tr["i"]][o] >= 0 and "sse" not in ot:
                    return False
    return True


@functools.lru_cache(maxsize=None)
def admit(seed):
    """The admission rule on case(seed): admit_case."""
    return admit_case(case(seed))


def admit_case(cs, keep_run=False):
    """The admission rule.  Returns dict(ok, why, ref, facts): `ref` the row_f32 run's means (T, P, 6), sigmas and indices
    (T - 1, P, N) -- the reference the device is compared with --, `spread` the relative tolerance (beside atol 1e-8) at
    which the two runs' moments agree, `facts` what the case exercises (largest SSD surface, levels and repeats inside the
    first template); with `keep_run` also `run`, the row_f32 run itself (oracle_run's results and traces)."""
    try:
        runs = {ssd: oracle_run(cs, ssd) for ssd in ("f64", "row_f32")}
    except (IndexError, ValueError) as e:
        return dict(ok=False, why=f"the oracle raises: {e}")
    if not all(_clean(cs, r) for r in runs.values()):
        return dict(ok=False, why="a search box leaves its frame")

    def indices(run):
        return np.stack([[tr["idx"] for tr in trace if "idx" in tr] for _, trace in run], axis=1)  # (T - 1, P, N)

    idx = {k: indices(r) for k, r in runs.items()}
    n_diff = int((idx["f64"] != idx["row_f32"]).sum())
    if n_diff:
        return dict(ok=False, why=f"{n_diff} resample indices depend on the accumulation order of the SSD")
    mom = {k: np.stack([np.concatenate((res["means"], res["sigmas"]), axis=1) for res, _ in r], axis=1)
           for k, r in runs.items()}  # (T, P, 12)
    if not np.isfinite(mom["row_f32"]).all():
        return dict(ok=False, why="moments are not finite")
    # what rtol would have to be for assert_allclose(row_f32, f64, rtol, atol=1e-8) to hold
    with np.errstate(divide="ignore", invalid="ignore"):
        excess = (np.abs(mom["f64"] - mom["row_f32"]) - 1e-8) / np.abs(mom["f64"])
    spread = float(max(0.0, np.nanmax(np.where(np.abs(mom["f64"]) > 0, excess, 0.0))))
    surfaces = [ot["sse"].shape for _, trace in runs["row_f32"] for tr in trace if "idx" in tr for ot in tr["obs"]
                if "sse" in ot]
    first = runs["row_f32"][0][1][0]["templates"][0]
    x0, y0, x1, y1 = first["box"]
    raw = cs["frames"][0][0][y0:y1, x0:x1]
    facts = dict(max_surface=max(max(s) for s in surfaces), min_surface=min(min(s) for s in surfaces),
                 frame_levels=int(len(np.unique(cs["frames"][0][0]))),
                 template_repeats=int(raw.size // cs["channels"] - len(first["histogram"][0])))
    ref = dict(means=mom["row_f32"][:, :, 0:6], sigmas=mom["row_f32"][:, :, 6:12], idx=idx["row_f32"])
    out = dict(ok=True, why="", ref=ref, spread=spread, facts=facts)
    if keep_run:
        out["run"] = runs["row_f32"]
    return out


def admitted(count, limit=200):
    """(the first `count` seeds the rule admits, the seeds it skipped on the way): the generator's fixed rule -- a seed
    that fails is passed over and the next one is tried."""
    seeds, skipped = [], []
    seed = 0
    while len(seeds) < count:
        assert seed < limit, "the admission rule refuses nearly every seed"
        (seeds if admit(seed)["ok"] else skipped).append(seed)
        seed += 1
    return tuple(seeds), tuple(skipped)
