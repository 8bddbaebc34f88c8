"""Generate tests/golden/orient_*.npz by RUNNING THE REFERENCE's optimize.ObserverCameras (optimize.py:1974-2083) and match
classes (:462-975) under the stub modules of tools/refstubs.py.  Build-container only; the fixtures hold inputs and the
reference's outputs, no reference source.  Re-run with:  python tools/make_golden_orient.py

Two shims let the reference's `fit` run on this SciPy, neither touching its arithmetic:
  * a sparse matrix cannot hold objects any more, so the grid of matches is built as
    coo_matrix((np.ones(k), (rows, cols))) and the object array is then assigned to `.data`;
  * scipy.optimize.minimize is wrapped: for the probe goldens by a fake that calls the reference's closure `fun` at given
    view directions and records (objective, gradient); for the fit goldens by the real one with `x0` flattened (this
    SciPy refuses a 2-D start).

  orient_sequence.npz  5 images, 6 pairs of 1 .. 1000 matches (either side of a wave and of a workgroup; one pair with
                       i > j; two images matched twice; one image only ever j), anchors [0, 3]: cameras, matches, the
                       reference's camera coordinates, R and Rprime, probes at anchor_weight 1e6 and 0, the four classes'
                       `predicted`, `filter`'s selections, and fits (maxiter = 5 and converged)
  orient_chunks.npz    6 images: a pair of 2 chunks + 37 matches, a pair without matches, an image in no pair: camera
                       coordinates and probes

sign(d_i - d_j) is rounding noise where the difference is ~0, so the noise on the matches is a condition: every component
at every probe must exceed 1e-9 in size (asserted here; the seeds were chosen so that the reference passes).
"""
import datetime
import io
import os
import sys
import contextlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refstubs  # noqa: E402

glimpse = refstubs.import_reference()
import scipy.optimize  # noqa: E402
import scipy.sparse  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
INTERNALS = dict(imgsz=(800, 536), f=(1000, 1010), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))
MIN_DXYZ = 1e-9


def observer(viewdirs):
    images = [glimpse.Image("synthetic", cam=glimpse.Camera(viewdir=v, **INTERNALS),
                            datetime=datetime.datetime(2020, 1, 1) + datetime.timedelta(hours=n))
              for n, v in enumerate(viewdirs)]
    return glimpse.Observer(images)


def make_matches(rng, true, pairs, sizes, noise_px=0.3):
    """uv uniform in the frame of image i, carried through the true cameras into image j, plus noise on both."""
    cams = [glimpse.Camera(viewdir=v, **INTERNALS) for v in true]
    uvs = []
    for (i, j), n in zip(pairs, sizes):
        uv_i = rng.uniform((40, 40), (760, 496), (n, 2))
        uv_j = cams[j].xyz_to_uv(cams[i].uv_to_xyz(uv_i), directions=True) if n else np.empty((0, 2))
        uvs.append((uv_i + rng.normal(0, noise_px, (n, 2)), uv_j + rng.normal(0, noise_px, (n, 2))))
    return uvs


def coo_of(objects, pairs):
    grid = scipy.sparse.coo_matrix((np.ones(len(pairs)), ([i for i, _ in pairs], [j for _, j in pairs])))
    data = np.empty(len(objects), dtype=object)
    data[:] = objects
    grid.data = data
    return grid


class Probe:
    """scipy.optimize.minimize replaced: the reference's callback evaluated at `points`."""

    def __init__(self, points):
        self.points, self.objective, self.gradient = points, [], []

    def __call__(self, fun, x0, jac=None, method=None, **kwargs):
        for x in self.points:
            objective, gradient = fun(np.array(x, dtype=float).ravel())
            self.objective.append(float(objective))
            self.gradient.append(np.array(gradient, dtype=float).reshape(-1, 3))
        return scipy.optimize.OptimizeResult(success=True, x=np.ravel(x0), message="probe")


def with_minimize(model, replacement, **fit_kwargs):
    original = scipy.optimize.minimize
    scipy.optimize.minimize = replacement
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return model.fit(**fit_kwargs)
    finally:
        scipy.optimize.minimize = original


def probes_of(model, points, matches):
    out = {}
    for name, weight in (("w1e6", 1e6), ("w0", 0.0)):
        probe = Probe(points)
        with_minimize(model, probe, anchor_weight=weight)
        out[f"probe_objective_{name}"] = np.array(probe.objective)
        out[f"probe_gradient_{name}"] = np.array(probe.gradient)
    # the condition on the noise, on the reference's own rays
    smallest = np.inf
    for x in points:
        model.set_cameras(x)
        for m in matches:
            if m.size:
                smallest = min(smallest, np.abs(m.predicted(cam=0) - m.predicted(cam=1)).min())
    model.reset_cameras()
    assert smallest > MIN_DXYZ, f"min |dxyz| = {smallest}: choose another seed"
    out["min_abs_dxyz"] = np.array(smallest)
    return out


def flat_minimize(fun, x0, **kwargs):
    return REAL_MINIMIZE(fun=fun, x0=np.ravel(np.array(x0, dtype=float)), **kwargs)


REAL_MINIMIZE = scipy.optimize.minimize


def build(seed, n_images, pairs, sizes, anchors, with_uv):
    rng = np.random.default_rng(seed)
    true = np.array([10.0, -3.0, 1.0]) + rng.normal(0, 0.3, (n_images, 3))
    start = true + rng.normal(0, 0.2, (n_images, 3))
    uvs = make_matches(rng, true, pairs, sizes)
    points = start + rng.normal(0, 0.1, (3, n_images, 3))
    obs = observer(start)
    cams = [img.cam for img in obs.images]
    if not with_uv:  # camera coordinates are the fixture; the reference still wants image coordinates to exist
        xys = [tuple(cams[c]._uv_to_xy(uv[k]) if len(uv[k]) else np.empty((0, 2)) for k, c in enumerate(pair))
               for pair, uv in zip(pairs, uvs)]
        matches = [glimpse.optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], uvs=list(uv), xys=list(xy))
                   for (i, j), uv, xy in zip(pairs, uvs, xys)]
    else:
        matches = [glimpse.optimize.RotationMatchesXYZ(cams=[cams[i], cams[j]], uvs=list(uv)) for (i, j), uv in zip(pairs, uvs)]
    model = glimpse.optimize.ObserverCameras(obs, matches=coo_of(matches, pairs), anchors=anchors)
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    out = {
        "internals": np.concatenate([np.asarray(INTERNALS[key], dtype=float) for key in ("imgsz", "f", "c", "k", "p")]),
        "viewdirs_true": true, "viewdirs_start": start, "pair_i": np.array([i for i, _ in pairs]),
        "pair_j": np.array([j for _, j in pairs]), "offsets": offsets, "anchors": np.array(anchors), "points": points,
        "xy_i": np.concatenate([m.xys[0].reshape(-1, 2) for m in matches]),
        "xy_j": np.concatenate([m.xys[1].reshape(-1, 2) for m in matches]),
        "R": np.array([cam.R for cam in cams]), "Rprime": np.array([cam.Rprime for cam in cams]),
    }
    if with_uv:
        out["uv_i"] = np.concatenate([uv[0] for uv in uvs])
        out["uv_j"] = np.concatenate([uv[1] for uv in uvs])
    out.update(probes_of(model, points, matches))
    return out, model, obs, matches, uvs


def sequence():
    pairs = [(0, 1), (0, 2), (1, 2), (1, 3), (3, 1), (2, 4)]
    sizes = [1, 63, 64, 65, 257, 1000]
    out, model, obs, matches, uvs = build(7, 5, pairs, sizes, [0, 3], with_uv=True)
    cams = [img.cam for img in obs.images]
    # the four classes' predictions on pair (1, 2), and filter's selections on pair (2, 4) as plain Matches
    p = 2
    i, j = pairs[p]
    for name, mtype in (("matches", glimpse.optimize.Matches), ("rotation", glimpse.optimize.RotationMatches),
                        ("xy", glimpse.optimize.RotationMatchesXY), ("xyz", glimpse.optimize.RotationMatchesXYZ)):
        m = mtype(cams=[cams[i], cams[j]], uvs=list(uvs[p]))
        for c in (0, 1):
            out[f"predicted_{name}_{c}"] = m.predicted(cam=c)
    i, j = pairs[5]
    rng = np.random.default_rng(70)
    weights = rng.uniform(0, 1, sizes[5])
    out["filter_weights"] = weights
    probe = glimpse.optimize.Matches(cams=[cams[i], cams[j]], uvs=list(uvs[5]))
    errors = [np.linalg.norm(probe.observed(c) - probe.predicted(c), axis=1) for c in (0, 1)]
    distance = np.linalg.norm(probe.observed(0) - probe.observed(1), axis=1)
    # thresholds inside the data (two decimals, so that no match sits on one): about half pass each
    e0, e1, d = (float(np.round(np.median(v), 2)) for v in (*errors, distance))
    width = float(INTERNALS["imgsz"][0])
    cases = (("error", dict(max_error=e0)), ("distance", dict(max_distance=d)),
             ("both", dict(max_error=1.2 * e1, max_distance=1.1 * d, cam=1)),
             ("scaled", dict(max_error=1.1 * e0 / width, max_distance=1.2 * d / width, scaled=True, min_weight=0.2)))
    for name, kwargs in cases:
        m = glimpse.optimize.Matches(cams=[cams[i], cams[j]], uvs=[uv.copy() for uv in uvs[5]], weights=weights.copy())
        before = m.uvs[0].copy()
        m.filter(**kwargs)
        keep = np.array([np.flatnonzero((before == row).all(axis=1))[0] for row in m.uvs[0]], dtype=np.int64)
        assert 0 < len(keep) < sizes[5], (name, len(keep))
        out[f"filter_{name}"] = keep
        out[f"filter_{name}_args"] = np.array([kwargs.get(key, 0) for key in ("max_error", "max_distance", "cam", "scaled", "min_weight")],
                                              dtype=float)
    # the fits
    for name, options in (("maxiter5", {"maxiter": 5}), ("converged", {})):
        result = with_minimize(model, flat_minimize, options=options)
        out[f"fit_{name}_x"] = np.asarray(result.x)
        out[f"fit_{name}_fun"] = np.array(float(result.fun))
        out[f"fit_{name}_nit"] = np.array(int(result.nit))
        out[f"fit_{name}_nfev"] = np.array(int(result.nfev))
        out[f"fit_{name}_success"] = np.array(bool(result.success))
        assert np.array_equal(np.array([c.viewdir for c in cams]), out["viewdirs_start"])
    np.savez_compressed(os.path.join(OUT, "orient_sequence.npz"), **out)
    return out


def chunks():
    pairs = [(0, 1), (1, 2), (2, 3), (4, 0), (3, 4)]
    sizes = [2 * 4096 + 37, 0, 300, 100, 50]
    out, *_ = build(11, 6, pairs, sizes, [0], with_uv=False)
    np.savez_compressed(os.path.join(OUT, "orient_chunks.npz"), **out)
    return out


if __name__ == "__main__":
    for make in (sequence, chunks):
        g = make()
        print(make.__name__, {k: v.shape for k, v in g.items() if k.startswith(("probe", "fit", "xy"))},
              "min |dxyz|", float(g["min_abs_dxyz"]))
