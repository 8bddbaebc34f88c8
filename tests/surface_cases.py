"""Seeded and designed cases of the frame step over gridded surfaces, and the rule that admits them (a plain helper module).

`case(seed)` starts from `option_cases.case(seed)` -- its cameras, frames, frame type, median window, spline orders,
template, N, host-fed draws, P = 3 and T = 4 -- and puts on top of it, by fixed rules of the seed,
  * which surfaces are gridded: `dem` only, `dem_sigma` only, both on one grid (the pair path), both on different grids
    (another cell size or orientation, limits shifted by a fraction of a cell), a viewshed on top in a third of the cases; one
    point of every case keeps constant surfaces (`params[p, 20:22] = 0`), and so does a point whose cloud the raster of a
    case placed at an edge does not hold;
  * the raster geometry: x and y ascending or descending in all four combinations, square and non-square cells, axes of
    fewer than 12 nodes (a window that is not `full`), one raster of 2 x 2 nodes, rasters of several hundred nodes a side and
    rasters that barely hold the clouds; the limits follow the clouds, so they are no round numbers;
  * the cell size relative to the cloud: 5.0 (the cloud well inside one cell), 0.4 (a few cells, inside the 9 the window
    serves) and 0.05 (more than the window serves: a share of the samples falls through to the general code);
  * the position in the raster: interior; particle 0 within six nodes of an edge or corner (the window's origin is clamped);
    the cloud reaching into the half-cell border between the outer cell centres and the outer limits (extrapolated samples,
    the interval clipped at 0 or n - 2);
  * the motion model: all four kinds by a rule of the seed (not the base case's draw), Cartesian and cylindrical with the DEM
    term sampled from the rasters, a `dem_sigma` raster with a block of exact zeros under the cloud in a share of the cases
    (the reference's `nonzero` mask: no term for those particles), the tangent models over a sloped, rough `dem` with
    `slope_sigma > 0`.
Surface values stay below a metre under cameras 100 m up, so every point stays in view.

The designed cases (DESIGNED) are built by hand on a base case and admitted by the same rule:
  * `glacier`: two observers, one oblique, RGB frames, TangentCartesianMotion on both points, `dem` and `dem_sigma` on one
    grid, a viewshed visible around the points, N = 5000, T = 3;
  * `border_tie_ascending` / `border_tie_descending`: a viewshed of cell size 1 with integer limits; four points pinned
    (sigma 0, no velocity, acceleration or noise along that axis) exactly on the border between a visible and a hidden
    cell -- in x with the hidden cell below and above, in y likewise; the same surfaces once with ascending and once with
    descending axes;
  * `on_the_limit`: a point pinned exactly to `dem.max[0]` (inside, extrapolated) and its twin one ulp beyond (out of bounds
    when the particles are drawn);
  * `leaves_the_raster`: a Cartesian point whose cloud crosses the outer limit of `dem` mid-sequence, a point that walks onto
    hidden viewshed cells, a tangent point that runs into NaN nodes of `dem`, one clean point.

`admit(name_or_seed)` is the rule of `option_cases.admit`, evaluated by the oracle alone: the host-fed draws run with the
SSD accumulated in float64 and row-wise in float32, and the case is admitted only if both runs give the same resample indices at
every step of every point and no search box leaves its frame; in a seeded case no track may raise; in a designed case the
tracks its `expect` names must raise the named error (at a step after the first where it says so), no other track may, and
both runs must fail at the same step.  On top, no particle of the oracle's run may lie within 1e-9 (1 + |limit|) of a
raster's outer limit or of a viewshed cell border, unless the case pins it there (`pinned`).  SEEDS is the first 24 seeds the
rule admits, walking up from 0; tests/test_surface_cases.py checks that the rule still yields it.
"""
import functools
import warnings

import numpy as np

from tests import option_cases as oc

COMBOS = ("dem", "dem_sigma", "pair", "two grids")
REGIMES = ("inside one cell", "a few cells", "beyond the window")
CELL = {"inside one cell": 5.0, "a few cells": 0.4, "beyond the window": 0.05}
POSITIONS = ("interior", "edge", "border")
ORIENTATIONS = ((1, 1), (-1, 1), (1, -1), (-1, -1))  # signs of (dx, dy): which way the array's columns and rows run
DESIGNED = ("glacier", "border_tie_ascending", "border_tie_descending", "on_the_limit", "leaves_the_raster")
OOB = "Some of the sampling coordinates are out of bounds"
HIDDEN = "Some particles are on non-visible viewshed cells"
MISSING = "Some particles have missing (NaN) values"

# the first 24 seeds the rule admits (tests/test_surface_cases.py: the rule run again gives this list)
SEEDS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24)
# eight of them that the fused kernel takes: once more on the staged kernels and with the tiles in the HBM workspaces
AGAIN = (0, 2, 7, 8, 10, 13, 15, 20)


def options(seed):
    """The surface axes of a seed (cheap: nothing is rendered)."""
    base = oc.options(seed)
    regime = REGIMES[(seed // 2) % 3]
    position = POSITIONS[(seed // 3 + seed // 12) % 3]
    tiny = seed % 12 == 0  # (an "inside one cell" case) a raster of 2 x 2 nodes
    return dict(combo=COMBOS[seed % 4], viewshed=seed % 3 == 1, orientation=ORIENTATIONS[(seed + seed // 4) % 4],
                regime=regime, position="interior" if tiny else position, tiny=tiny,
                aspect=(1.0, 1.0, 0.73, 1.0, 1.37)[seed % 5], kind=(seed + seed // 4 + seed // 16) % 4,
                zeros=seed % 4 != 0 and (seed // 4) % 2 == 1, sides=((seed // 2) % 2, (seed // 5) % 2),
                edge_axes=((0,), (1,), (0, 1))[(seed // 6) % 3], constant_point=seed % oc.P,
                fused=base["interp"] in oc.FUSED_ORDERS and max(base["tile"]) <= 63)


def _velocity(base):
    """The scene's velocity in the direction of time, back from the base case's motion table."""
    q = base["params"][0]
    return q[4:6].copy() if base["kind"] in (0, 2) else q[4] * np.array((np.cos(q[5]), np.sin(q[5])))


def motion_table(xy, kind, v, wide=False):
    """The [P][24] table of glh_set_motion for points `xy`, all of one kind, like option_cases.case makes it with a z term."""
    params = np.zeros((len(xy), 24))
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
        params[:, 9], params[:, 15] = 0.03, 0.01  # sigmas of the vertical velocity and acceleration
        params[:, 17] = 0.4
    else:
        params[:, 17] = 0.2
        params[:, 19] = 0.05  # slope_sigma
    return params


def _model(q, n, dem=None, dem_sigma=None):
    """The oracle's motion model of a row of the motion table; `dem` / `dem_sigma`: the case's rasters, taken where the row's
    flags [20], [21] say so."""
    from oracle import motion as omotion

    d = dem if q[20] else q[16]
    s = dem_sigma if q[21] else q[17]
    if q[18] < 2:
        cls = omotion.CartesianMotion if q[18] == 0 else omotion.CylindricalMotion
        return cls(xy=q[0:2], xy_sigma=q[2:4], vxyz=q[4:7], vxyz_sigma=q[7:10], axyz=q[10:13], axyz_sigma=q[13:16],
                   dem=d, dem_sigma=s, n=n)
    cls = omotion.TangentCartesianMotion if q[18] == 2 else omotion.TangentCylindricalMotion
    return cls(xy=q[0:2], xy_sigma=q[2:4], vxy=q[4:6], vxy_sigma=q[7:9], axy=q[10:12], axy_sigma=q[13:15], dem=d,
               dem_sigma=s, n=n, slope_sigma=q[19])


def hulls(params, draws, taus, N):
    """Per point and step the box (T, P, 2, 2) = [min, max] of (x, y) of the cloud evolved WITHOUT resampling over constant
    surfaces (x and y do not depend on the surfaces): what the geometry of a case is laid out around."""
    T, P = len(taus) + 1, len(params)
    out = np.empty((T, P, 2, 2))
    for p in range(P):
        q = params[p].copy()
        q[20:22] = 0.0
        model = _model(q, N)
        particles, _ = model.initialize_particles(draws["init"][p])
        out[0, p] = particles[:, 0:2].min(axis=0), particles[:, 0:2].max(axis=0)
        for s in range(T - 1):
            model.evolve_particles(particles, taus[s], draws["evolve"][s, p])
            out[s + 1, p] = particles[:, 0:2].min(axis=0), particles[:, 0:2].max(axis=0)
    return out


def surface(kind, shape, xlim, ylim, rng, zeros_at=None, nan_box=None):
    """A surface as (array, xlim, ylim).  "dem": a slope, a swell and node-to-node roughness, below a metre; "dem_sigma":
    0.3 .. 0.4, with a block of 3 x 3 .. 5 x 5 exact zeros around `zeros_at`; `nan_box` = (x0, x1, y0, y1): NaN nodes."""
    ny, nx = shape
    x = np.linspace(xlim[0], xlim[1], 2 * nx + 1)[1::2]  # cell centres, first column to last
    y = np.linspace(ylim[0], ylim[1], 2 * ny + 1)[1::2]
    X, Y = np.meshgrid(x, y)
    if kind == "dem":
        z = 0.02 * X - 0.015 * Y + 0.2 * np.sin(0.9 * X + 0.3) * np.cos(0.7 * Y) + 0.05 * rng.standard_normal(shape)
    else:
        z = 0.3 + 0.1 * rng.random(shape)
        if zeros_at is not None:
            half = 1 + int(rng.integers(0, 2))
            j, i = int(np.abs(y - zeros_at[1]).argmin()), int(np.abs(x - zeros_at[0]).argmin())
            z[max(j - half, 0):j + half + 1, max(i - half, 0):i + half + 1] = 0.0
    if nan_box is not None:
        z[(X >= nan_box[0]) & (X <= nan_box[1]) & (Y >= nan_box[2]) & (Y <= nan_box[3])] = np.nan
    return z, tuple(float(v) for v in xlim), tuple(float(v) for v in ylim)


def _limits(lo, hi, cell, sign, grow_high=True, n=None):
    """(limits in array order, node count) of an axis of cells `cell` that holds [lo, hi]; the side that must stay where it is
    keeps its value, the other moves out to a whole number of cells."""
    if n is None:
        n = max(2, int(np.ceil((hi - lo) / cell)))
    if grow_high:
        hi = lo + n * cell
    else:
        lo = hi - n * cell
    return ((lo, hi) if sign > 0 else (hi, lo)), n


def _inside(box, xlim, ylim, margin=1e-6):
    return bool(min(xlim) + margin < box[0, 0] and box[1, 0] < max(xlim) - margin and
                min(ylim) + margin < box[0, 1] and box[1, 1] < max(ylim) - margin)


def _viewshed_around(boxes, cell, sign, rng, pad=4.0, clear=2.5):
    """A viewshed that holds every box with `pad` to spare: visible within `clear` of a box, hidden cells scattered beyond."""
    lo, hi = boxes[:, 0].min(axis=0) - pad, boxes[:, 1].max(axis=0) + pad
    xlim, nx = _limits(lo[0], hi[0], cell[0], sign[0])
    ylim, ny = _limits(lo[1], hi[1], cell[1], sign[1])
    x = np.linspace(xlim[0], xlim[1], 2 * nx + 1)[1::2]
    y = np.linspace(ylim[0], ylim[1], 2 * ny + 1)[1::2]
    X, Y = np.meshgrid(x, y)
    near = np.zeros((ny, nx), dtype=bool)
    for b in boxes:
        near |= (X > b[0, 0] - clear) & (X < b[1, 0] + clear) & (Y > b[0, 1] - clear) & (Y < b[1, 1] + clear)
    vis = np.where(near | (rng.random((ny, nx)) < 0.5), 1.0, 0.0)
    return vis, tuple(float(v) for v in xlim), tuple(float(v) for v in ylim)


def _finish(cs, surfaces, expect=None, pinned=(), name=None):
    """The case dict: the base case's entries, the surfaces as (array, xlim, ylim) for glimpse_amd.Raster and as oracle
    Rasters, what the admission rule is to expect."""
    from oracle import raster as oraster

    cs = dict(cs)
    cs["surfaces"] = {k: surfaces.get(k) for k in ("dem", "dem_sigma", "viewshed")}
    cs["oracle_surfaces"] = {k: None if v is None else oraster.Raster(v[0], x=v[1], y=v[2])
                             for k, v in cs["surfaces"].items()}
    cs["expect"] = dict(expect or {})  # point -> (message, "init" / "later" / None: whatever the oracle says)
    cs["pinned"] = tuple(pinned)       # (point, axis): left out of the distance-to-a-limit precondition
    cs["name"] = name if name is not None else cs["seed"]
    return cs


@functools.lru_cache(maxsize=4)
def _seeded(seed):
    base = oc.case(seed)
    opt = options(seed)
    rng = np.random.default_rng(3000 + seed)
    P, N, T = base["P"], base["N"], base["T"]
    params = motion_table(base["params"][:, 0:2], opt["kind"], _velocity(base), base["wide"])
    hull = hulls(params, base["draws"], base["taus"], N)
    box = np.stack((hull[:, :, 0].min(axis=0), hull[:, :, 1].max(axis=0)), axis=1)  # (P, 2, 2) over the steps
    focus = (opt["constant_point"] + 1) % P
    others = [p for p in range(P) if p != opt["constant_point"]]
    cell = np.array((CELL[opt["regime"]], CELL[opt["regime"]] * opt["aspect"])) * float(rng.uniform(0.85, 1.2))
    lims, counts = [], []
    for a in range(2):
        lo = min(box[p, 0, a] for p in others) - float(rng.uniform(6.5, 9.0)) * cell[a]
        hi = max(box[p, 1, a] for p in others) + float(rng.uniform(6.5, 9.0)) * cell[a]
        grow_high = True
        if opt["tiny"]:
            lo = min(box[p, 0, a] for p in others) - float(rng.uniform(0.3, 0.6)) * cell[a]
            hi = max(box[p, 1, a] for p in others) + float(rng.uniform(0.3, 0.6)) * cell[a]
            cell[a] = (hi - lo) / 2
        elif opt["position"] != "interior" and a in opt["edge_axes"]:
            # the chosen side follows the focus point alone: a few cells off its cloud, or a fraction of a cell
            gap = float(rng.uniform(0.6, 2.5) if opt["position"] == "edge" else rng.uniform(0.02, 0.3)) * cell[a]
            if opt["sides"][a]:
                hi, grow_high = box[focus, 1, a] + gap, False
            else:
                lo = box[focus, 0, a] - gap
        lim, n = _limits(lo, hi, cell[a], opt["orientation"][a], grow_high, n=2 if opt["tiny"] else None)
        lims.append(lim)
        counts.append(n)
    shape = (counts[1], counts[0])
    gridded = [p for p in others if _inside(box[p], lims[0], lims[1])]
    assert focus in gridded
    zeros_at = box[focus].mean(axis=0) if opt["zeros"] else None
    surfaces = {}
    combo = opt["combo"]
    if combo in ("dem", "pair", "two grids"):
        surfaces["dem"] = surface("dem", shape, lims[0], lims[1], rng)
    if combo in ("dem_sigma", "pair"):
        surfaces["dem_sigma"] = surface("dem_sigma", shape, lims[0], lims[1], rng, zeros_at)
    if combo == "two grids":
        # another cell size in half of the cases, the other orientation in x, limits a fraction of a cell further out
        c2 = cell * (1.6 if (seed // 4) % 2 else 1.0)
        sign2 = (-opt["orientation"][0], opt["orientation"][1])
        xl, nx2 = _limits(min(lims[0]) - 0.37 * cell[0], max(lims[0]) + 0.21 * cell[0], c2[0], sign2[0])
        yl, ny2 = _limits(min(lims[1]) - 0.58 * cell[1], max(lims[1]) + 0.13 * cell[1], c2[1], sign2[1])
        surfaces["dem_sigma"] = surface("dem_sigma", (ny2, nx2), xl, yl, rng, zeros_at)
    if opt["viewshed"]:
        sign3 = ORIENTATIONS[(ORIENTATIONS.index(opt["orientation"]) + 2) % 4]
        surfaces["viewshed"] = _viewshed_around(box, (1.3, 0.9), sign3, rng)
    for p in gridded:
        params[p, 20] = float("dem" in surfaces)
        params[p, 21] = float("dem_sigma" in surfaces)
    cs = dict(base, params=params, kind=opt["kind"], surface_options=opt, gridded=tuple(gridded), focus=focus)
    return _finish(cs, surfaces)


def _points(base, rng, count, margin, candidates=None, apart=4.0):
    """`count` points every camera of the base case sees with `margin` pixels to spare, at least `apart` from one another."""
    from glimpse_amd import synth

    xy = []
    for _ in range(20000):
        cand = np.array([rng.uniform(-14, 14), rng.uniform(-14, 14)]) if candidates is None else candidates(rng)
        ok = all(np.abs(cand - q).max() >= apart for q in xy)
        for cam in base["cams"]:
            uv = synth.project(cam, np.array([[cand[0], cand[1], 0.0]]))[0]
            ok &= bool(margin < uv[0] < cam[6] - margin and margin < uv[1] < cam[7] - margin)
        if ok:
            xy.append(cand)
        if len(xy) == count:
            return np.array(xy)
    raise AssertionError("no room for the points")


def _rebase(base, xy, N, T, kind, host_seed):
    """The base case with other points, particle count and length: a new motion table of one kind and new host-fed draws."""
    P = len(xy)
    host = np.random.default_rng(host_seed)
    draws = dict(init=host.standard_normal((P, N, 6)), evolve=host.standard_normal((T - 1, P, N, 3)),
                 u=host.random((T - 1, P)))
    return dict(base, P=P, N=N, T=T, params=motion_table(xy, kind, _velocity(base)), kind=kind, draws=draws,
                matching=base["matching"][:T], taus=base["taus"][:T - 1],
                frames=[f[:T] for f in base["frames"]])


def _pin(params, p, axis):
    """Point p does not move along `axis`: no spread, velocity, acceleration or noise there (a Cartesian point)."""
    params[p, 2 + axis] = params[p, 4 + axis] = params[p, 7 + axis] = params[p, 10 + axis] = params[p, 13 + axis] = 0.0


GLACIER_BASE, TIE_BASE, LIMIT_BASE, LEAVES_BASE = 30, 5, 2, 7


def _glacier():
    base = oc.case(GLACIER_BASE)
    assert len(base["cams"]) == 2 and base["channels"] == 3 and base["interp"] in oc.FUSED_ORDERS
    cs = _rebase(base, base["params"][:2, 0:2], 5000, 3, 2, 501)
    rng = np.random.default_rng(502)
    hull = hulls(cs["params"], cs["draws"], cs["taus"], cs["N"])
    box = np.stack((hull[:, :, 0].min(axis=0), hull[:, :, 1].max(axis=0)), axis=1)
    lo, hi = box[:, 0].min(axis=0) - 3.1, box[:, 1].max(axis=0) + 2.7
    xlim, nx = _limits(lo[0], hi[0], 0.25, 1)
    ylim, ny = _limits(lo[1], hi[1], 0.25, -1)  # (north up: y descends along the rows, like a DEM read from a file)
    surfaces = dict(dem=surface("dem", (ny, nx), xlim, ylim, rng), dem_sigma=surface("dem_sigma", (ny, nx), xlim, ylim, rng),
                    viewshed=_viewshed_around(box, (1.0, 1.0), (1, -1), rng, pad=2.0))
    cs["params"][:, 20:22] = 1.0
    return _finish(dict(cs, gridded=(0, 1), focus=0), surfaces, name="glacier")


def _border_tie(sign):
    base = oc.case(TIE_BASE)
    rng = np.random.default_rng(511)
    margin = 0.5 * max(base["tile"]) + 45.0
    # four points on integer x or y: the cell borders of a viewshed of cell size 1 with integer limits
    xy = _points(base, rng, 4, margin, lambda r: np.array([float(r.integers(-13, 14)), float(r.integers(-13, 14))]) + 0.37)
    xy[0:2, 0] = np.round(xy[0:2, 0] - 0.37)
    xy[2:4, 1] = np.round(xy[2:4, 1] - 0.37)
    cs = _rebase(base, xy, 513, 4, 0, 512)
    vis = np.ones((40, 40))
    xlim, ylim = ((-20.0, 20.0), (-20.0, 20.0)) if sign > 0 else ((20.0, -20.0), (20.0, -20.0))

    def hide(x0, x1, y0, y1):  # the cells whose centres lie in the box
        c = np.arange(-20, 20) + 0.5
        cx, cy = (c, c) if sign > 0 else (c[::-1], c[::-1])
        vis[np.ix_((cy > y0) & (cy < y1), (cx > x0) & (cx < x1))] = 0.0

    for p in range(4):
        axis, above = p // 2, p % 2
        _pin(cs["params"], p, axis)
        b = [xy[p, 0] - 2.6, xy[p, 0] + 2.6, xy[p, 1] - 2.6, xy[p, 1] + 2.6]
        b[2 * axis + (0 if above else 1)] = xy[p, axis]  # hidden above (below) the border the point sits on
        b[2 * axis + (1 if above else 0)] = xy[p, axis] + (1.0 if above else -1.0)
        hide(*b)
    pinned = tuple((p, p // 2) for p in range(4))
    name = "border_tie_ascending" if sign > 0 else "border_tie_descending"
    # (whether a point is hidden is the oracle's word: the rule takes whatever it says, the same in both runs)
    expect = {p: (HIDDEN, None) for p in range(4)}
    return _finish(dict(cs, gridded=(), focus=0), dict(viewshed=(vis, xlim, ylim)), expect, pinned, name)


def _on_the_limit():
    base = oc.case(LIMIT_BASE)
    rng = np.random.default_rng(521)
    margin = 0.5 * max(base["tile"]) + 45.0
    xy = _points(base, rng, 2, margin)
    xy = np.array([xy[0], (np.nextafter(xy[0, 0], np.inf), xy[0, 1]), xy[1]])
    cs = _rebase(base, xy, 777, 4, 0, 522)
    _pin(cs["params"], 0, 0)
    _pin(cs["params"], 1, 0)
    ylim, ny = _limits(xy[0, 1] - 6.3, xy[0, 1] + 5.9, 0.4, -1)
    xlim = (xy[0, 0] - 31 * 0.4, xy[0, 0])  # max[0] is the pinned x itself
    cs["params"][0:2, 20] = 1.0
    return _finish(dict(cs, gridded=(0, 1), focus=0), dict(dem=surface("dem", (ny, 31), xlim, ylim, rng)),
                   {1: (OOB, "init")}, ((0, 0), (1, 0)), "on_the_limit")


def _leaves_the_raster():
    base = oc.case(LEAVES_BASE)
    assert base["taus"][0] > 0
    rng = np.random.default_rng(531)
    margin = 0.5 * max(base["tile"]) + 45.0
    xy = _points(base, rng, 4, margin, apart=6.0)
    xy = xy[np.argsort(-xy[:, 0])]  # point 0 the one furthest along x: the raster ends ahead of it
    cs = _rebase(base, xy, 777, 4, 0, 532)
    v = _velocity(base)
    cs["params"][2] = motion_table(xy[2:3], 2, v)[0]  # the tangent point
    hull = hulls(cs["params"], cs["draws"], cs["taus"], cs["N"])
    box = np.stack((hull[:, :, 0].min(axis=0), hull[:, :, 1].max(axis=0)), axis=1)
    ahead = 1.0 if v[0] > 0 else -1.0
    edge = lambda p, s: hull[s, p, 1 if ahead > 0 else 0, 0]  # noqa: E731  the leading x of point p's cloud at step s
    # dem: ends a little ahead of where the cloud of point 0 stands after one step; NaN nodes ahead of point 2
    lead = edge(0, 1) + ahead * 0.02
    far = min(box[0, 0, 0], box[2, 0, 0]) - 4.3 if ahead > 0 else max(box[0, 1, 0], box[2, 1, 0]) + 4.3
    xlim, nx = _limits(min(lead, far), max(lead, far), 0.4, 1, grow_high=ahead < 0)
    ylo, yhi = min(box[0, 0, 1], box[2, 0, 1]) - 3.7, max(box[0, 1, 1], box[2, 1, 1]) + 4.1
    ylim, ny = _limits(ylo, yhi, 0.4, -1)
    nan_from = edge(2, 1) + ahead * 0.45
    nan_box = (min(nan_from, nan_from + ahead * 3.0), max(nan_from, nan_from + ahead * 3.0), box[2, 0, 1] - 2.0,
               box[2, 1, 1] + 2.0)
    dem = surface("dem", (ny, nx), xlim, ylim, rng, nan_box=nan_box)
    # viewshed: hidden cells ahead of point 1
    vis, vx, vy = _viewshed_around(box, (0.5, 0.5), (1, 1), np.random.default_rng(533), pad=3.0, clear=50.0)
    gx = np.linspace(vx[0], vx[1], 2 * vis.shape[1] + 1)[1::2]
    gy = np.linspace(vy[0], vy[1], 2 * vis.shape[0] + 1)[1::2]
    hide_from = edge(1, 1) + ahead * 0.3
    cols = (gx > hide_from) & (gx < hide_from + 3.0) if ahead > 0 else (gx < hide_from) & (gx > hide_from - 3.0)
    vis[np.ix_((gy > box[1, 0, 1] - 2.0) & (gy < box[1, 1, 1] + 2.0), cols)] = 0.0
    cs["params"][0, 20] = cs["params"][2, 20] = 1.0
    expect = {0: (OOB, "later"), 1: (HIDDEN, "later"), 2: (MISSING, "later")}
    return _finish(dict(cs, gridded=(0, 2), focus=0), dict(dem=dem, viewshed=(vis, vx, vy)), expect, (),
                   "leaves_the_raster")


@functools.lru_cache(maxsize=None)
def _designed(name):
    return {"glacier": _glacier, "border_tie_ascending": lambda: _border_tie(1),
            "border_tie_descending": lambda: _border_tie(-1), "on_the_limit": _on_the_limit,
            "leaves_the_raster": _leaves_the_raster}[name]()


def case(name_or_seed):
    return _designed(name_or_seed) if isinstance(name_or_seed, str) else _seeded(int(name_or_seed))


def oracle_run(cs, ssd):
    """The oracle's tracks of a case on its host-fed draws: per point (result of track_one with its error captured, trace)."""
    from oracle import tracker as otracker

    observers = oc.oracle_observers(cs, ssd)
    sf = cs["oracle_surfaces"]
    out = []
    for p in range(cs["P"]):
        d = cs["draws"]
        draws = {"init": d["init"][p], "evolve": [d["evolve"][s, p] for s in range(cs["T"] - 1)],
                 "u": [d["u"][s, p] for s in range(cs["T"] - 1)]}
        trace = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = otracker.track_one(_model(cs["params"][p], cs["N"], sf["dem"], sf["dem_sigma"]), observers,
                                     cs["matching"], cs["taus"], tile_size=cs["tile"], draws=draws, trace=trace,
                                     capture_errors=True, viewshed=sf["viewshed"])
        out.append((res, trace))
    return out


def failing_frame(res, trace):
    """The frame at which a track raised (None: it ran through): the last one the oracle began."""
    return None if res["error"] is None else int(trace[-1]["i"])


def _too_close(cs, run):
    """The precondition on distances: a description of the first particle within 1e-9 (1 + |limit|) of an outer limit of a
    raster its point samples, or of a cell border of the viewshed; None if there is none."""
    sf = cs["oracle_surfaces"]
    for p, (_, trace) in enumerate(run):
        used = [k for k, flag in (("dem", cs["params"][p, 20]), ("dem_sigma", cs["params"][p, 21])) if flag and sf[k]]
        for tr in trace:
            if "evolved" not in tr:
                continue
            for a in range(2):
                if (p, a) in cs["pinned"]:
                    continue
                x = tr["evolved"][:, a]
                x = x[np.isfinite(x)]
                for k in used + (["viewshed"] if sf["viewshed"] is not None else []):
                    r = sf[k]
                    for limit in (r.min[a], r.max[a]):
                        if (np.abs(x - limit) <= 1e-9 * (1 + abs(limit))).any():
                            return f"point {p} frame {tr['i']}: a particle on the {'xy'[a]} limit {limit} of {k}"
                if sf["viewshed"] is not None:
                    r = sf["viewshed"]
                    t = (x - r.min[a]) / abs(r.d[a])
                    near = np.abs(t - np.round(t)) * abs(r.d[a]) <= 1e-9 * (1 + np.abs(x))
                    if near.any():
                        return f"point {p} frame {tr['i']}: a particle on a cell border of the viewshed ({'xy'[a]})"
    return None


@functools.lru_cache(maxsize=None)
def admit(name_or_seed):
    """The admission rule.  Returns dict(ok, why, ref): `ref` the row_f32 run -- means and sigmas (T, P, 6), NaN from the
    frame at which a track failed; idx (T - 1, P, N), -1 where a track had failed; evolved (T, P, N, 6), the particles
    after the motion step of every frame (NaN where the oracle did not get that far); pre0 (T, P, 2): x, y of particle 0
    before the step of frame i (what the raster windows are placed around); errors: per point None or (frame, message)."""
    cs = case(name_or_seed)
    T, P, N = cs["T"], cs["P"], cs["N"]
    runs = {ssd: oracle_run(cs, ssd) for ssd in ("f64", "row_f32")}
    errors = {k: [None if res["error"] is None else (failing_frame(res, trace), str(res["error"]))
                  for res, trace in r] for k, r in runs.items()}
    if errors["f64"] != errors["row_f32"]:
        return dict(ok=False, why=f"the two accumulations fail differently: {errors}")
    errs = errors["row_f32"]
    for p in range(P):
        want = cs["expect"].get(p)
        if errs[p] is None:
            if want is not None and want[1] is not None:
                return dict(ok=False, why=f"point {p} does not raise '{want[0]}'")
            continue
        if want is None:
            return dict(ok=False, why=f"the oracle raises at point {p}, frame {errs[p][0]}: {errs[p][1]}")
        if errs[p][1] != want[0]:
            return dict(ok=False, why=f"point {p} raises '{errs[p][1]}', not '{want[0]}'")
        if want[1] is not None and (errs[p][0] == 0) != (want[1] == "init"):
            return dict(ok=False, why=f"point {p} raises at frame {errs[p][0]}, expected: {want[1]}")
    idx = {k: np.full((T - 1, P, N), -1, dtype=np.int64) for k in runs}
    for k, r in runs.items():
        for p, (res, trace) in enumerate(r):
            for tr in trace:
                if "idx" in tr:
                    idx[k][tr["i"] - 1, p] = tr["idx"]
                    for o, ot in enumerate(tr["obs"]):
                        if cs["matching"][tr["i"]][o] >= 0 and "sse" not in ot:
                            return dict(ok=False, why="a search box leaves its frame")
            done = T - 1 if errs[p] is None else max(errs[p][0] - 1, 0)
            if int((idx[k][:done, p] >= 0).all(axis=1).sum()) != done:
                return dict(ok=False, why=f"point {p}: steps are missing from the trace")
    n_diff = int((idx["f64"] != idx["row_f32"]).sum())
    if n_diff:
        return dict(ok=False, why=f"{n_diff} resample indices depend on the accumulation order of the SSD")
    close = _too_close(cs, runs["row_f32"])
    if close:
        return dict(ok=False, why=close)
    run = runs["row_f32"]
    means, sigmas = (np.stack([res[k] for res, _ in run], axis=1) for k in ("means", "sigmas"))
    for p in range(P):
        ok_frames = T if errs[p] is None else errs[p][0]
        if not (np.isfinite(means[:ok_frames, p]).all() and np.isfinite(sigmas[:ok_frames, p]).all()):
            return dict(ok=False, why="moments are not finite")
    evolved = np.full((T, P, N, 6), np.nan)
    pre0 = np.full((T, P, 2), np.nan)
    for p, (_, trace) in enumerate(run):
        for tr in trace:
            if "evolved" in tr:
                evolved[tr["i"], p] = tr["evolved"]
        for i in range(1, T):
            # the state before the step of frame i: the particles of frame i - 1, resampled (frame 0: as drawn)
            src = 0 if i == 1 else idx["row_f32"][i - 2, p, 0]
            if src >= 0:
                pre0[i, p] = evolved[i - 1, p, src, 0:2]
    ref = dict(means=means, sigmas=sigmas, idx=idx["row_f32"], evolved=evolved, pre0=pre0, errors=errs)
    return dict(ok=True, why="", ref=ref)


def admitted(count, limit=200):
    """(the first `count` seeds the rule admits, the seeds it skipped on the way)."""
    seeds, skipped = [], []
    seed = 0
    while len(seeds) < count:
        assert seed < limit, "the admission rule refuses nearly every seed"
        (seeds if admit(seed)["ok"] else skipped).append(seed)
        seed += 1
    return tuple(seeds), tuple(skipped)
