"""The cases of tests/surface_cases.py, on the CPU: the admission rule run again, and a NumPy restatement of where the fused
kernel places its raster windows and of which code serves every raster sample of every admitted case -- the coverage the
device sweep (tests/test_gpu_surface_sweep.py) relies on is a condition on the oracle's runs, checked here."""
import collections

import numpy as np
import pytest

from tests import option_cases as oc
from tests import surface_cases as sc

COUNT = 24
W = 12  # GLH_PATCH_W (glh_math.h): nodes a side of a raster window
CLASSES = ("window only", "window by guess", "from the raster", "border")


# ---- the restatement (glh_math.h) -------------------------------------------------------------------------------------
class Grid:
    """What RasterDev holds of a raster: ascending cell centres, outer limits, cells per unit length."""

    def __init__(self, r):
        self.n = [int(v) for v in r.size]
        self.lo, self.hi = r.min, r.max
        self.g = [np.linspace(r.min[a] + abs(r.d[a]) / 2, r.max[a] - abs(r.d[a]) / 2, self.n[a]) for a in range(2)]
        self.k = [self.n[a] / (r.max[a] - r.min[a]) for a in range(2)]
        self.cell = np.abs(r.d)


def guess(n, x, lo, k):
    """raster_guess"""
    t = (x - lo) * k - 0.5
    return np.where(t > 0.0, np.where(t < n - 2, np.trunc(np.minimum(t, n)), n - 2), 0).astype(np.int64)


def interval(g, x, i):
    """raster_interval: the guess moved by at most one, clipped to [0, n - 2]"""
    n = len(g)
    down = (i > 0) & (g[i] >= x)
    up = ~down & (i < n - 2) & (g[i + 1] < x)
    return i - down.astype(np.int64) + up.astype(np.int64)


def patch_origin(grid, xy):
    """raster_patch_origin: per axis (first node, nodes held, whether the origin was clamped)"""
    out = []
    inside = all(grid.lo[a] <= xy[a] <= grid.hi[a] for a in range(2))
    for a in range(2):
        n = grid.n[a]
        w = min(n, W)
        c = int(guess(n, np.float64(xy[a]), grid.lo[a], grid.k[a])) if inside else 0
        raw = c - (w // 2 - 1)
        o = min(max(raw, 0), n - w)
        out.append((o, w, o != raw))
    return out


def window_ok(grid, a, o, x):
    """the `ok` of raster_window_axis: 1 <= cells from the window's first node < W - 2"""
    f = (x - grid.g[a][o]) * grid.k[a]
    return (f >= 1.0) & (f < W - 2)


def in_window(gi, o, w, n):
    """raster_in_window"""
    ell = gi - o
    return ((ell >= 1) | (gi == 0)) & (ell >= 0) & ((ell + 2 < w) | (gi == n - 2)) & (ell + 1 < w)


def classify(grid, origin, xy):
    """Per sample (x, y) of a raster with its window at `origin`: the class (an index into CLASSES) and the interval per axis."""
    full = all(w == W for _, w, _ in origin)
    only = np.full(len(xy), full)
    by_guess = np.ones(len(xy), dtype=bool)
    border = np.zeros(len(xy), dtype=bool)
    cells = []
    for a in range(2):
        o, w, _ = origin[a]
        x = xy[:, a]
        assert ((x >= grid.lo[a]) & (x <= grid.hi[a])).all()  # (the oracle ran through: every sample is inside)
        gi = guess(grid.n[a], x, grid.lo[a], grid.k[a])
        i = interval(grid.g[a], x, gi)
        cells.append(i)
        if full:
            only &= window_ok(grid, a, o, x)
        by_guess &= in_window(gi, o, w, grid.n[a])
        border |= (x < grid.g[a][0]) | (x > grid.g[a][-1])
    cls = np.where(border, 3, np.where(only, 0, np.where(by_guess, 1, 2)))
    assert not (border & only).any()  # the window-only code serves no extrapolated sample
    return cls, cells


def samples(cs, ref):
    """Every raster sample the frame step takes, as (slot, frame, point, window centre, (n, 2) positions): Cartesian and
    cylindrical points sample their gridded surfaces under the evolved particles (the DEM term), the tangent models sample
    `dem` under every particle before and after the move."""
    for p in cs["gridded"]:
        q = cs["params"][p]
        for i in range(1, cs["T"]):
            after = ref["evolved"][i, p]
            if ref["errors"][p] is not None and i >= ref["errors"][p][0]:
                break  # (the track ends at this frame)
            if q[18] < 2:
                for slot, flag in (("dem", q[20]), ("dem_sigma", q[21])):
                    if flag:
                        yield slot, i, p, ref["pre0"][i, p], after[:, 0:2]
            elif q[20]:
                before = ref["evolved"][i - 1, p] if i == 1 else ref["evolved"][i - 1, p][ref["idx"][i - 2, p]]
                yield "dem", i, p, ref["pre0"][i, p], np.concatenate((before[:, 0:2], after[:, 0:2]))


def survey(name):
    """What a case exercises: samples per class, clamped origins, the cloud's span in cells, exact zeros of dem_sigma."""
    cs, ref = sc.case(name), sc.admit(name)["ref"]
    grids = {k: Grid(r) for k, r in cs["oracle_surfaces"].items() if r is not None and k != "viewshed"}
    counts = collections.Counter()
    facts = dict(clamped=False, span=0.0, zeros=0)
    for slot, i, p, centre, xy in samples(cs, ref):
        grid = grids[slot]
        origin = patch_origin(grid, centre)
        cls, cells = classify(grid, origin, xy)
        for a in range(2):  # the restatement's own check: the interval is scipy's clipped searchsorted
            want = np.clip(np.searchsorted(grid.g[a], xy[:, a], side="left") - 1, 0, grid.n[a] - 2)
            np.testing.assert_array_equal(cells[a], want)
        counts.update(CLASSES[c] for c in cls)
        clamped = any(c for _, _, c in origin)
        facts["clamped"] |= clamped
        facts["span"] = max(facts["span"], float(((xy.max(axis=0) - xy.min(axis=0)) / grid.cell).max()))
        if slot == "dem_sigma":
            facts["zeros"] += int((cs["oracle_surfaces"]["dem_sigma"].sample(xy) == 0.0).sum())
    return counts, facts


def regime_of(span):
    return sc.REGIMES[0] if span < 1.0 else (sc.REGIMES[2] if span > W - 3 else sc.REGIMES[1])


def axes(cs, facts):
    """The axis values of a seeded case, for the coverage count."""
    opt, sf = cs["surface_options"], cs["surfaces"]
    main = sf["dem"] if sf["dem"] is not None else sf["dem_sigma"]
    nodes = [s for k in ("dem", "dem_sigma") if sf[k] is not None for s in sf[k][0].shape]
    return {"surfaces": opt["combo"], "viewshed": sf["viewshed"] is not None, "orientation": opt["orientation"],
            "square cells": opt["aspect"] == 1.0 or opt["tiny"], "an axis below 12 nodes": min(nodes) < W,
            "2 x 2 nodes": main[0].shape == (2, 2), "200 nodes a side or more": max(nodes) >= 200,
            "regime": regime_of(facts["span"]), "clamped origin": facts["clamped"],
            "motion model": oc.KINDS[cs["kind"]], "observers": len(cs["cams"]), "frame type": cs["ftype"],
            "a missing image": bool((cs["matching"] < 0).any()),
            "every other point gridded": len(cs["gridded"]) == cs["P"] - 1}


AXIS_VALUES = {"surfaces": sc.COMBOS, "viewshed": (False, True), "orientation": sc.ORIENTATIONS,
               "square cells": (False, True), "an axis below 12 nodes": (False, True), "2 x 2 nodes": (True,),
               "200 nodes a side or more": (True,), "regime": sc.REGIMES, "clamped origin": (False, True),
               "motion model": oc.KINDS, "observers": (1, 2), "frame type": oc.FRAME_TYPES, "a missing image": (False, True),
               "every other point gridded": (False, True)}


def test_the_rule_admits_the_committed_cases_and_they_cover_the_raster_code():
    seeds, skipped = sc.admitted(COUNT)
    print(f"skipped: {[(s, sc.admit(s)['why']) for s in skipped]}")
    assert seeds == tuple(sc.SEEDS), (seeds, skipped)
    assert 4 * len(skipped) <= len(seeds) + len(skipped)
    assert len(sc.AGAIN) == 8 and all(s in sc.SEEDS and sc.options(s)["fused"] for s in sc.AGAIN)
    count = collections.defaultdict(collections.Counter)
    share = collections.Counter()
    with_kind = collections.defaultdict(set)
    clamped_orientations, zero_cases = set(), 0
    print(f"{'case':>22} " + " ".join(f"{c:>16}" for c in CLASSES) + "   span (cells)  clamped  sigma == 0")
    for name in seeds + sc.DESIGNED:
        cs = sc.case(name)
        counts, facts = survey(name)
        total = sum(counts.values())
        print(f"{str(name):>22} " + " ".join(f"{counts[c]:>16}" for c in CLASSES) +
              f"   {facts['span']:12.2f}  {str(facts['clamped']):>7}  {facts['zeros']:>10}")
        if isinstance(name, str):
            continue
        assert cs["P"] == 3 and cs["T"] == 4 and cs["N"] in oc.N_CHOICES and all(v <= 520 for v in cs["imgsz"])
        assert 1 <= len(cs["gridded"]) < cs["P"] and (cs["params"][:, 20:22] == 0).all(axis=1).any()
        for axis, value in axes(cs, facts).items():
            count[axis][value] += 1
        for c in CLASSES:
            share[c] += 20 * counts[c] >= total > 0
        if facts["clamped"]:
            clamped_orientations.add(cs["surface_options"]["orientation"])
        if cs["kind"] < 2:
            with_kind[cs["surface_options"]["combo"]].add(cs["kind"])
        zero_cases += facts["zeros"] > 0 and cs["kind"] < 2
    for axis, values in AXIS_VALUES.items():
        print(axis, dict(count[axis]))
        for value in values:
            assert count[axis][value] >= 2, (axis, value, dict(count[axis]))
    print("cases with 5 % of their samples or more in a class:", dict(share))
    for c in CLASSES:
        assert share[c] >= 3, (c, dict(share))
    assert clamped_orientations == set(sc.ORIENTATIONS), clamped_orientations
    assert with_kind["pair"] == {0, 1} and with_kind["two grids"] == {0, 1}, dict(with_kind)
    assert zero_cases >= 2, zero_cases  # the `nonzero` mask of the DEM term has particles to leave out


@pytest.mark.parametrize("name", sc.DESIGNED)
def test_the_rule_admits_the_designed_cases(name):
    a = sc.admit(name)
    assert a["ok"], a["why"]
    cs, errs = sc.case(name), a["ref"]["errors"]
    print(name, errs)
    assert cs["P"] <= 4 and cs["T"] <= 4
    if name == "glacier":
        assert errs == [None, None] and cs["N"] == 5000 and cs["channels"] == 3 and len(cs["cams"]) == 2
        assert (cs["params"][:, 18] == 2).all() and (cs["params"][:, 20:22] == 1).all()
        assert np.array_equal(cs["surfaces"]["dem"][1:], cs["surfaces"]["dem_sigma"][1:])
        counts, _ = survey(name)
        assert counts["window only"] > 0
    elif name.startswith("border_tie"):
        # every particle of a pinned point sits exactly on a cell border of the viewshed, all through the sequence; the tie
        # goes to the cell of the lower coordinate (y0 <= 0.5), whichever way the array runs
        ev = a["ref"]["evolved"]
        for p in range(4):
            axis, at = p // 2, cs["params"][p, p // 2]
            assert at == np.round(at) and cs["params"][p, 2 + axis] == 0.0
            if errs[p] is None:  # (a track that raises when its particles are drawn leaves none to look at)
                assert (ev[:, p, :, axis] == at).all()
        assert [e is not None for e in errs] == [True, False, True, False]
        assert all(e is None or e == (0, sc.HIDDEN) for e in errs)
        other = sc.admit("border_tie_descending" if name.endswith("_ascending") else "border_tie_ascending")
        assert other["ref"]["errors"] == errs
    elif name == "on_the_limit":
        x = a["ref"]["evolved"][:, 0, :, 0]
        assert (x == cs["oracle_surfaces"]["dem"].max[0]).all()
        assert errs == [None, (0, sc.OOB), None]
    else:
        assert [e and e[1] for e in errs] == [sc.OOB, sc.HIDDEN, sc.MISSING, None]
        assert all(e is None or 2 <= e[0] <= 3 for e in errs), errs
