"""Designed cases at the search-tile sizes and particle counts where the frame step changes its path (a plain helper
module; the cases are the dicts of tests/option_cases.py: case, and its oracle_run, admit_case and the runner of
tests/test_gpu_option_sweep.py serve them unchanged).

The generator of option_cases.py reaches search tiles of 118 x 113 pixels on uint8 frames and about 60 x 60 on the others,
and 3000 particles.  Here the size is designed.  A nadir camera (f = 1000 at 100 units: PX = 10 pixels per world unit, no
distortion) makes pixel offsets a fixed multiple of world offsets, and the host-fed `init` draws are not Gaussian: the
first four particles of a point sit on the corners (+-1, +-1) of the prior's box with zero velocity draws and zero
evolve draws, a quarter is spread evenly over (-0.96, 0.96)^2 and the rest lies within a few pixels of the point.  The
search box of the first update is then the corners' extent plus the template, to the pixel: xy_sigma = (side - template
- 1) / 2 / PX.  Later updates see the resampled cloud, a few pixels wide.  P = 2, T = 3, N = 500 .. 1500.

TILE_CASES -- name: what it is the edge of (the size class is asserted by tests/test_wide_cases.py from the oracle's trace)
  u8_300          uint8 gray, ~300 x 300, workspace 320: fused kernel, tile in its HBM workspace, a surface above 255 cells
  u8rgb_300x70    uint8 RGB, ~300 x 70, 7 x 7 window with 'wrap' (the band-with-halo path), 766 keys, non-square
  u16_250         uint16 gray, ~250 x 250, workspace 255: 60 000 <= n <= 65 025, the fused kernel's 16-bit keys at their limit
  u16_256         uint16 gray in 300 levels, ~280 x 280, 31 x 31 template, workspace 320: the first size the plan refuses;
                  many equal keys per bucket of the ranking
  u16rgb_1117     uint16 RGB, ~1110 x 60 on 1280 x 192 frames, workspace 1117: the widest band glh_observer_set_depth takes
  f32_96          float32 gray, ~93 x 93 (n a little over 8192): fused kernel, tile in LDS.  8192 is NumPy's summation
                  chunk, but the search tile depends on its normalisation only through ties (the CDF match uses ranks):
                  this case shows that the path runs and ends with the oracle's indices, it is no pin of the sums
  f32rgb_200x130  float32 RGB quantised, ~200 x 130, 47 x 47 template: a CDF of 2209 entries, scratch too large for LDS
  f32_300         float32 gray, ~290 x 290: staged kernels only
  f64_260         float64 gray, ~270 x 270, orders (1, 1): staged only, bilinear sampling of a wide surface
  f64rgb_128      float64 RGB, ~128 x 128: the fused kernel's general instantiation
FUSED_TILE_CASES are those the plan (glh_point_plan.h: pt_plan) accepts; the others run on the staged kernels.

COUNT_CASES -- uint8 gray 320 x 320 frames, 15 x 15 templates, the sweep's narrow prior with Gaussian host-fed draws:
  n10976 the last count the fused kernel takes (shape (1024, 0, 1)), n10977 the first it refuses, n12000, n14950 the last
  glh_create takes, n14950x2 the same with two observers.  FUSED_LAST and CREATE_LAST are written down here and derived:
  fused_last(plan) sweeps pt_plan, create_last() evaluates the check of glh_create as the library's source states it;
  tests/test_wide_cases.py asserts that both give the literals.

Seeds: a case that fails admission (option_cases.admit_case: the oracle alone, SSD accumulated in float64 and row-wise in
float32, equal indices, no track raises, no search box leaves its frame) gets another seed here, and this paragraph says
so.  Replaced so far: n10977 22 -> 26 (under seed 22 one resample index of 65 862 depends on the accumulation order of
the SSD).
"""
import functools
import os
import re

import numpy as np

from tests import option_cases as oc

P, T = 2, 3
PX = 10.0  # pixels per world unit of the nadir camera
VELOCITY = (0.15, 0.05)

# name: frame type, channels, levels, frame size, search tile aimed at (w, h), template, window, mode, orders, N,
#       max_search_dim, seed
TILE_CASES = {
    "u8_300": dict(ftype="uint8", channels=1, levels="full", imgsz=(640, 640), aim=(300, 300), tile=(15, 15),
                   window=(5, 5), mode="reflect", interp=(3, 3), N=1000, max_search_dim=320, seed=1),
    "u8rgb_300x70": dict(ftype="uint8", channels=3, levels="full", imgsz=(640, 320), aim=(300, 70), tile=(15, 15),
                         window=(7, 7), mode="wrap", interp=(3, 3), N=700, max_search_dim=320, seed=2),
    "u16_250": dict(ftype="uint16", channels=1, levels="full", imgsz=(576, 576), aim=(250, 250), tile=(15, 15),
                    window=(3, 5), mode="nearest", interp=(3, 3), N=1500, max_search_dim=255, seed=3),
    "u16_256": dict(ftype="uint16", channels=1, levels="300", imgsz=(640, 640), aim=(280, 280), tile=(31, 31),
                    window=(5, 5), mode="mirror", interp=(3, 3), N=800, max_search_dim=320, seed=4),
    "u16rgb_1117": dict(ftype="uint16", channels=3, levels="full", imgsz=(1280, 192), aim=(1110, 60), tile=(15, 15),
                        window=(5, 5), mode="reflect", interp=(3, 3), N=1200, max_search_dim=1117, seed=5),
    "f32_96": dict(ftype="float32", channels=1, levels="full", imgsz=(320, 320), aim=(93, 93), tile=(15, 15),
                   window=(5, 3), mode="reflect", interp=(3, 3), N=500, max_search_dim=160, seed=6),
    "f32rgb_200x130": dict(ftype="float32", channels=3, levels="quantised", imgsz=(512, 448), aim=(200, 130),
                           tile=(47, 47), window=(3, 3), mode="nearest", interp=(3, 3), N=600, max_search_dim=224, seed=7),
    "f32_300": dict(ftype="float32", channels=1, levels="full", imgsz=(640, 640), aim=(290, 290), tile=(15, 15),
                    window=(5, 5), mode="wrap", interp=(3, 3), N=900, max_search_dim=320, seed=8),
    "f64_260": dict(ftype="float64", channels=1, levels="full", imgsz=(640, 640), aim=(270, 270), tile=(15, 15),
                    window=(3, 7), mode="mirror", interp=(1, 1), N=1000, max_search_dim=320, seed=9),
    "f64rgb_128": dict(ftype="float64", channels=3, levels="full", imgsz=(384, 384), aim=(128, 128), tile=(15, 15),
                       window=(7, 3), mode="mirror", interp=(3, 3), N=1100, max_search_dim=160, seed=10),
}
FUSED_TILE_CASES = ("u8_300", "u8rgb_300x70", "u16_250", "f32_96", "f32rgb_200x130", "f64rgb_128")

# the size class of every tile case: bounds on (width, height, pixels) of the largest search tile of a track
BIG = 10 ** 9
SIZE_CLASS = {
    "u8_300": dict(w=(290, 320), h=(290, 320)),
    "u8rgb_300x70": dict(w=(290, 320), h=(60, 80)),
    "u16_250": dict(w=(240, 255), h=(240, 255), n=(60000, 65025)),
    "u16_256": dict(w=(256, 300), h=(256, 300)),
    "u16rgb_1117": dict(w=(1100, 1117), h=(16, 64)),
    "f32_96": dict(w=(91, 96), h=(91, 96), n=(8193, 96 * 96)),
    "f32rgb_200x130": dict(w=(190, 210), h=(120, 140)),
    "f32_300": dict(w=(256, 320), h=(256, 320)),
    "f64_260": dict(w=(256, 320), h=(256, 320)),
    "f64rgb_128": dict(w=(120, 136), h=(120, 136)),
}

FUSED_LAST = 10976   # the largest particle count pt_plan accepts (no rasters, one or two observers): fused_last()
CREATE_LAST = 14950  # the largest max_particles glh_create accepts: create_last()
COUNT_CASES = {
    "n10976": dict(N=FUSED_LAST, observers=1, seed=21),
    "n10977": dict(N=FUSED_LAST + 1, observers=1, seed=26),
    "n12000": dict(N=12000, observers=1, seed=23),
    "n14950": dict(N=CREATE_LAST, observers=1, seed=24),
    "n14950x2": dict(N=CREATE_LAST, observers=2, seed=25),
}
FUSED_COUNT_CASES = ("n10976",)
NAMES = tuple(TILE_CASES) + tuple(COUNT_CASES)
FUSED = FUSED_TILE_CASES + FUSED_COUNT_CASES


def fused_last(plan, observers=1, rasters=0, tile=(15, 15), lo=10000, hi=16000):
    """The largest N in [lo, hi) that `plan(n, observers, tile=..., rasters=...)` (tests/test_hostcheck.py: _plan with the
    library bound) accepts, every count below it down to lo accepted as well."""
    took = [n for n in range(lo, hi) if plan(n, observers, tile=tile, rasters=rasters)[0]]
    assert took == list(range(lo, took[-1] + 1))
    return took[-1]


@functools.lru_cache(maxsize=None)
def _create_check():
    """(A, B, C) of the check of glh_create in glimpse_amd/csrc/glimpse_hip.hip: max_particles * A + B > C * 1024."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "glimpse_amd", "csrc", "glimpse_hip.hip")).read()
    found = re.findall(r"k\.max_particles \* (\d+) \+ (\d+) > (\d+) \* 1024", text)
    assert len(found) == 1, found
    return tuple(int(v) for v in found[0])


def create_refuses(n):
    """Whether glh_create refuses max_particles = n."""
    a, b, c = _create_check()
    return n * a + b > c * 1024


def create_last():
    """The largest max_particles glh_create takes."""
    return max(n for n in range(1, 1 << 16) if not create_refuses(n))


def _cameras(imgsz, observers):
    from glimpse_amd import synth

    cams = [synth.nadir_camera(imgsz, f=100.0 * PX, height=100.0)]
    if observers == 2:  # (the second station of option_cases.case)
        cams.append(synth.pack_camera(imgsz=imgsz, f=900.0, k=(0.02, 0, 0), xyz=(12.0, -9.0, 95.0),
                                      viewdir=(-53.13, -82.0, 0.0)))
    return cams


def _points(cam, imgsz):
    """World xy of the P points: a few pixels either side of the frame's centre, at fractional pixel positions."""
    from glimpse_amd import synth

    uv = np.array([[imgsz[0] / 2 - 6.3, imgsz[1] / 2 + 3.6], [imgsz[0] / 2 + 5.8, imgsz[1] / 2 - 2.9]])
    return synth.uv_to_ground(cam, uv)


def _build(name, spec, observers, xy_sigma, v_sigma, draws):
    from glimpse_amd import synth

    seed, imgsz, ftype, channels, levels = (spec[k] for k in ("seed", "imgsz", "ftype", "channels", "levels"))
    cams = _cameras(imgsz, observers)
    scene = synth.default_scene(cams[-1], seed=seed, velocity=VELOCITY, n_frames=T, margin=8.0)
    taus = np.ones(T - 1)
    times = np.concatenate(([0.0], np.cumsum(taus)))
    frames = [[oc.render(scene, cam, t, ftype, channels, levels) for t in times] for cam in cams]
    params = np.zeros((P, 24))
    params[:, 0:2] = _points(cams[0], imgsz)
    params[:, 2:4] = xy_sigma
    params[:, 4:6] = VELOCITY
    params[:, 7:9] = v_sigma
    params[:, 13:15] = 0.04
    tile = spec["tile"]
    return dict(seed=seed, name=name, imgsz=imgsz, cams=cams, frames=frames, channels=channels, dtype=np.dtype(ftype),
                ftype=ftype, levels=levels, window=spec["window"], mode=spec["mode"], interp=spec["interp"], kind=0,
                has_z=False, tile=tile, tile_class="designed", wide=True, N=spec["N"], P=P, T=T, params=params,
                matching=np.tile(np.arange(T)[:, None], (1, observers)), taus=taus, sigmas=[0.3, 0.45][:observers],
                draws=draws, max_tile=max(31, max(tile)), max_search_dim=spec["max_search_dim"])


def _spread_draws(seed, N):
    """The draws of a tile case: see the module docstring."""
    rng = np.random.default_rng(seed)
    init = rng.standard_normal((P, N, 6))
    evolve = rng.standard_normal((T - 1, P, N, 3))
    n_wide = N // 4
    init[:, :, 0:2] *= 0.02
    init[:, :n_wide, 0:2] = rng.uniform(-0.96, 0.96, (P, n_wide, 2))
    init[:, :4, 0:2] = [(-1, -1), (1, -1), (-1, 1), (1, 1)]
    init[:, :4, 2:6] = 0.0
    evolve[:, :, :4] = 0.0
    return dict(init=init, evolve=evolve, u=rng.random((T - 1, P)))


@functools.lru_cache(maxsize=None)
def case(name):
    if name in TILE_CASES:
        spec = TILE_CASES[name]
        aim, tile = spec["aim"], spec["tile"]
        xy_sigma = [(aim[k] - tile[k] - 1) / 2.0 / PX for k in (0, 1)]
        return _build(name, spec, 1, xy_sigma, 0.05, _spread_draws(spec["seed"], spec["N"]))
    spec = dict(COUNT_CASES[name], ftype="uint8", channels=1, levels="full", imgsz=(320, 320), tile=(15, 15),
                window=(5, 5), mode="reflect", interp=(3, 3), max_search_dim=160)
    host = np.random.default_rng(spec["seed"])
    N = spec["N"]
    draws = dict(init=host.standard_normal((P, N, 6)), evolve=host.standard_normal((T - 1, P, N, 3)),
                 u=host.random((T - 1, P)))
    return _build(name, spec, spec["observers"], 0.15, 0.1, draws)  # (the sweep's narrow prior)


@functools.lru_cache(maxsize=None)
def admit(name):
    """option_cases.admit_case of the case, with the row_f32 run kept (the stage comparisons read its trace)."""
    return oc.admit_case(case(name), keep_run=True)


def tiles_reached(run):
    """(width, height) of every search tile of a run's trace: [(step, point, observer, w, h)]."""
    out = []
    for p, (_, trace) in enumerate(run):
        for tr in trace:
            for o, ot in enumerate(tr.get("obs", [])):
                if "sse" in ot:
                    x0, y0, x1, y1 = (int(v) for v in ot["box"])
                    out.append((tr["i"], p, o, x1 - x0, y1 - y0))
    return out


def largest_tile(run):
    """(w, h) of the search tile with the most pixels."""
    return max(((w, h) for _, _, _, w, h in tiles_reached(run)), key=lambda s: s[0] * s[1])


def in_class(name, w, h):
    c = SIZE_CLASS[name]
    n = c.get("n", (0, BIG))
    return c["w"][0] <= w <= c["w"][1] and c["h"][0] <= h <= c["h"][1] and n[0] <= w * h <= n[1]


def plan_frames(cs):
    """The `frames` entry of tests/test_hostcheck.py: _plan for a case, and its interp_k."""
    bits = 8 * cs["dtype"].itemsize
    k = cs["interp"][0] if cs["interp"] in oc.FUSED_ORDERS else 0
    return (bits, cs["channels"], cs["max_search_dim"]), k
