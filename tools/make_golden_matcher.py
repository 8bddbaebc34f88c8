"""Generate tests/golden/matcher_*.npz by RUNNING THE REFERENCE's optimize.match_keypoints (optimize.py:2234-2309) and
KeypointMatcher (:2312-2773) under the stub modules of tools/refstubs.py.  Build-container only; the fixtures hold inputs
and the reference's outputs, no reference source.  Re-run with:  python tools/make_golden_matcher.py

cv2 is absent, so the reference is given a stand-in `matcher` (tests/matcher_restated.py: exact brute force, a stable sort
of the squared distances) and keypoints that are objects with `.pt`.  Its default argument cv2.FlannBasedMatcher() is
evaluated at import; the permissive cv2 stub covers that.

The reference keeps the matches of a sequence in a scipy.sparse.coo_matrix of objects, which this SciPy cannot build, so
  * build_matches runs with path=<tmp>, clear_matches=True and the pair pickles it writes are read back;
  * convert_matches, filter_matches, matches_per_image, images_per_image, drop_images and match_breaks run on a stand-in
    grid: coo_matrix((np.ones(k), (rows, cols))) with the object array assigned to `.data` (make_golden_orient.coo_of).

  matcher_pairs.npz     two keypoint sets of 182 and 181 SIFT-like uint8 descriptors (shared features under noise, an exact
                        duplicate in the train set, a query equal to a train row), match_keypoints for the 16 combinations
                        of cross_check, max_ratio, max_distance and return_ratios; the empty cases; the 0 / 0 case
  matcher_sequence.npz  six images (hours 0, 1, 2, 5, 6, 10) of 90 .. 140 keypoints: the pair lists of six (maxdt, seq,
                        imgs) settings, the matches of every pair (max_ratio 0.8, weights), and the container methods
"""
import collections
import contextlib
import datetime
import io
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refstubs  # noqa: E402

glimpse = refstubs.import_reference()
import scipy.sparse  # noqa: E402

import matcher_restated as mr  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
INTERNALS = dict(imgsz=(800, 536), f=(1000, 1010), c=(3, -2), k=(0.1, -0.05, 0.01, 0, 0, 0), p=(0.001, -0.002))
KP = collections.namedtuple("KP", "pt")
HOURS = (0, 1, 2, 5, 6, 10)
MAX_RATIO, MAX_DISTANCE = 0.8, 20.0
H = datetime.timedelta(hours=1)
# name -> (maxdt in hours or None, seq, imgs)
SETTINGS = {"all": (None, None, None), "maxdt2": (2, None, None), "seq12": (None, (1, 2), None),
            "maxdt1_seq3": (1, (3,), None), "seq1_imgs25": (None, (1,), (2, 5)), "maxdt4_imgs0": (4, None, (0,))}


def sift_like(rng, n, dim=128):
    return np.minimum(rng.gamma(0.6, 40.0, (n, dim)), 255).astype(np.uint8)


def noisy(rng, d, amplitude=8):
    return np.clip(d.astype(int) + rng.integers(-amplitude, amplitude + 1, d.shape), 0, 255).astype(np.uint8)


def keypoints(points, descriptors):
    return [KP((float(u), float(v))) for u, v in points], descriptors


def quiet(call, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return call(*args, **kwargs)


def pairs():
    rng = np.random.default_rng(21)
    base = sift_like(rng, 220)
    points = rng.uniform((20, 20), (780, 516), (220, 2))
    ia, ib = rng.permutation(np.arange(0, 180)), rng.permutation(np.arange(40, 220))
    desc_a, desc_b = noisy(rng, base[ia]), noisy(rng, base[ib])
    pts_a = points[ia] + rng.normal(0, 0.5, (180, 2))
    pts_b = points[ib] + (12.0, -7.0) + rng.normal(0, 0.5, (180, 2))
    # an exact duplicate of train row 5 at the end of the train set; queries equal to train rows 5 and 9; the extremes
    desc_b = np.vstack([desc_b, desc_b[5]])
    pts_b = np.vstack([pts_b, pts_b[5] + (300.0, 0.0)])
    desc_a = np.vstack([desc_a, desc_b[9], np.zeros((1, 128), np.uint8)])
    desc_a[7] = 255
    pts_a = np.vstack([pts_a, pts_b[9] - (12.0, -7.0), (400.0, 300.0)])
    out = {"desc_a": desc_a, "desc_b": desc_b, "pts_a": pts_a, "pts_b": pts_b, "max_ratio": np.array(MAX_RATIO),
           "max_distance": np.array(MAX_DISTANCE)}
    ka, kb = keypoints(pts_a, desc_a), keypoints(pts_b, desc_b)
    matcher = mr.BruteForceMatcher()
    for c in (0, 1):
        for r in (0, 1):
            for d in (0, 1):
                for w in (0, 1):
                    result = glimpse.optimize.match_keypoints(
                        ka, kb, cross_check=bool(c), max_ratio=MAX_RATIO if r else None,
                        max_distance=MAX_DISTANCE if d else None, return_ratios=bool(w), matcher=matcher)
                    assert len(result) == 2 + w and 0 < len(result[0]) < len(desc_a) + (not (c or r or d)), (c, r, d, w, len(result[0]))
                    for name, value in zip(("uva", "uvb", "ratios"), result):
                        out[f"case{c}{r}{d}{w}_{name}"] = value
    # the empty cases: too few keypoints for k = 2; nothing passes the ratio test
    one = keypoints(pts_a[:1], desc_a[:1])
    far = keypoints(pts_a[:180], desc_a[:180])  # (without the query that equals a train row: its ratio is 0)
    for name, result in (("few", glimpse.optimize.match_keypoints(one, kb, return_ratios=True, matcher=matcher)),
                         ("few_k1", glimpse.optimize.match_keypoints((one[0][:0], desc_a[:0]), kb, matcher=matcher)),
                         ("none", glimpse.optimize.match_keypoints(far, kb, max_ratio=1e-9, return_ratios=True, matcher=matcher)),
                         ("none_plain", glimpse.optimize.match_keypoints(far, kb, max_ratio=1e-9, matcher=matcher))):
        for k, value in enumerate(result):
            assert len(value) == 0
            out[f"empty_{name}_{k}"] = value
    # k = 1 against one train row is served (no second neighbour is asked for)
    single = glimpse.optimize.match_keypoints(ka, keypoints(pts_b[:1], desc_b[:1]), matcher=matcher)
    out["single_uva"], out["single_uvb"] = single
    # 0 / 0: query 0 has two exact copies in the train set
    zd_a, zd_b = desc_a[:3], np.vstack([desc_a[0], desc_b[:2], desc_a[0]])
    out["zd_a"], out["zd_b"] = zd_a, zd_b
    try:
        glimpse.optimize.match_keypoints(keypoints(pts_a[:3], zd_a), keypoints(pts_b[:4], zd_b), max_ratio=MAX_RATIO, matcher=matcher)
        raise AssertionError("the reference did not raise")
    except ZeroDivisionError:
        pass
    np.savez_compressed(os.path.join(OUT, "matcher_pairs.npz"), **out)
    return out


def coo_of(objects, rows, cols, n):
    grid = scipy.sparse.coo_matrix((np.ones(len(objects)), (rows, cols)), shape=(n, n))
    data = np.empty(len(objects), dtype=object)
    data[:] = objects
    grid.data = data
    return grid


def sequence_inputs():
    rng = np.random.default_rng(33)
    n = len(HOURS)
    viewdirs = np.array([10.0, -3.0, 1.0]) + rng.normal(0, 0.6, (n, 3))
    cams = [glimpse.Camera(viewdir=v, **INTERNALS) for v in viewdirs]
    m = 200
    base = sift_like(rng, m)
    rays = cams[0].uv_to_xyz(rng.uniform((-150, -100), (950, 640), (m, 2)))
    points, descriptors = [], []
    for cam in cams:
        uv = cam.xyz_to_uv(rays, directions=True)
        seen = np.flatnonzero(cam.inframe(uv) & (rng.uniform(size=m) < 0.8))
        seen = rng.permutation(seen)
        extra = int(rng.integers(5, 15))  # keypoints of nothing shared
        points.append(np.vstack([uv[seen] + rng.normal(0, 0.3, (len(seen), 2)), rng.uniform((0, 0), (800, 536), (extra, 2))]))
        descriptors.append(np.vstack([noisy(rng, base[seen]), sift_like(rng, extra)]))
    return viewdirs, points, descriptors


def reference_matcher(viewdirs, points, descriptors):
    images = [glimpse.Image(f"frames/img_{i}.jpg", cam=glimpse.Camera(viewdir=v, **INTERNALS),
                            datetime=datetime.datetime(2020, 1, 1) + h * H)
              for i, (v, h) in enumerate(zip(viewdirs, HOURS))]
    model = glimpse.optimize.KeypointMatcher(images)
    model.keypoints = [keypoints(p, d) for p, d in zip(points, descriptors)]
    return model


def written_pairs(model, tmp, **kwargs):
    """[(i, j, Matches)] of the pickles the reference's build_matches writes, in (i, j) order."""
    quiet(model.build_matches, path=tmp, clear_matches=True, clear_keypoints=False, matcher=mr.BruteForceMatcher(), **kwargs)
    assert model.matches is None
    names = [glimpse.helpers.strip_path(img.path) for img in model.images]
    found = []
    for i in range(len(names)):
        for j in range(len(names)):
            file = os.path.join(tmp, f"{names[i]}-{names[j]}.pkl")
            if os.path.exists(file):
                found.append((i, j, glimpse.helpers.read_pickle(file)))
    return found


def sequence():
    viewdirs, points, descriptors = sequence_inputs()
    n = len(HOURS)
    out = {"viewdirs": viewdirs, "hours": np.array(HOURS), "max_ratio": np.array(MAX_RATIO),
           "internals": np.concatenate([np.asarray(INTERNALS[key], dtype=float) for key in ("imgsz", "f", "c", "k", "p")]),
           "sizes": np.array([len(p) for p in points]), "points": np.vstack(points), "descriptors": np.vstack(descriptors),
           "settings": np.array(list(SETTINGS))}
    found = {}
    for name, (maxdt, seq, imgs) in SETTINGS.items():
        model = reference_matcher(viewdirs, points, descriptors)
        with tempfile.TemporaryDirectory() as tmp:
            found[name] = written_pairs(model, tmp, maxdt=None if maxdt is None else maxdt * H, seq=seq, imgs=imgs,
                                        max_ratio=MAX_RATIO, weights=True)
        out[f"pairs_{name}"] = np.array([(i, j) for i, j, _ in found[name]], dtype=np.int64).reshape(-1, 2)
        # the shape of the reference's grid: what its own expression, coo_matrix(([1] * k, (rows, cols))), infers
        k = len(found[name])
        out[f"shape_{name}"] = np.array(scipy.sparse.coo_matrix(([1] * k, (out[f"pairs_{name}"][:, 0], out[f"pairs_{name}"][:, 1]))).shape)
    every = found["all"]
    assert len(every) == n * (n - 1) // 2 and all(m.size > 3 for _, _, m in every), [m.size for _, _, m in every]
    out["match_offsets"] = np.concatenate(([0], np.cumsum([m.size for _, _, m in every]))).astype(np.int64)
    out["match_uva"] = np.vstack([m.uvs[0] for _, _, m in every])
    out["match_uvb"] = np.vstack([m.uvs[1] for _, _, m in every])
    out["match_weights"] = np.concatenate([m.weights for _, _, m in every])

    def on_grid(name):
        """A reference KeypointMatcher holding the pairs of setting `name` in the stand-in grid, cameras re-pointed."""
        model = reference_matcher(viewdirs, points, descriptors)
        objects = []
        for i, j, m in found[name]:
            objects.append(glimpse.optimize.Matches(cams=(model.images[i].cam, model.images[j].cam), uvs=[uv.copy() for uv in m.uvs],
                                                    weights=m.weights.copy()))
        model.matches = coo_of(objects, [i for i, _, _ in found[name]], [j for _, j, _ in found[name]], n)
        return model

    model = on_grid("all")
    out["matches_per_image"] = np.asarray(model.matches_per_image())
    out["images_per_image"] = np.asarray(model.images_per_image())
    out["min_weight"] = np.array(float(np.round(np.median(out["match_weights"]), 2)))
    model.filter_matches(min_weight=float(out["min_weight"]), clear_weights=True)
    assert all(m.weights is None for m in model.matches.data)
    out["filtered_sizes"] = np.array([m.size for m in model.matches.data])
    out["filtered_matches_per_image"] = np.asarray(model.matches_per_image())
    model.convert_matches(glimpse.optimize.RotationMatchesXYZ, clear_uvs=True)
    assert all(type(m) is glimpse.optimize.RotationMatchesXYZ and m.uvs is None for m in model.matches.data)
    out["converted_xy_a"] = np.vstack([m.xys[0] for m in model.matches.data])
    out["converted_xy_b"] = np.vstack([m.xys[1] for m in model.matches.data])
    # drop_images and match_breaks
    for name, setting, drop in (("a", "all", 1), ("b", "seq12", [1, 2]), ("c", "maxdt2", [4]), ("d", "seq1_imgs25", 2)):
        model = on_grid(setting)
        before = list(model.images)
        model.drop_images(drop)
        out[f"drop_{name}_setting"] = np.array(setting)
        out[f"drop_{name}_imgs"] = np.atleast_1d(drop)
        out[f"drop_{name}_scalar"] = np.array(not np.iterable(drop))
        out[f"drop_{name}_row"], out[f"drop_{name}_col"] = np.asarray(model.matches.row), np.asarray(model.matches.col)
        out[f"drop_{name}_shape"] = np.array(model.matches.shape)
        out[f"drop_{name}_images"] = np.array([before.index(img) for img in model.images], dtype=np.int64)
        out[f"drop_{name}_sizes"] = np.array([m.size for m in model.matches.data])
        out[f"drop_{name}_breaks"] = np.asarray(model.match_breaks())
    for name in SETTINGS:
        model = on_grid(name)
        out[f"breaks_{name}"] = np.asarray(model.match_breaks())
        # min_matches compares the counts of the images that start a pair with one bound per image: the reference's own
        # arithmetic refuses that unless one image starts every pair
        starts = len(np.unique(model.matches.row))
        try:
            out[f"breaks_{name}_min2"] = np.asarray(model.match_breaks(min_matches=2))
            assert starts == 1, name
        except ValueError as error:
            assert "broadcast" in str(error) and starts not in (1, n), name
    np.savez_compressed(os.path.join(OUT, "matcher_sequence.npz"), **out)
    return out


if __name__ == "__main__":
    for make in (pairs, sequence):
        g = make()
        print(make.__name__, len(g), "arrays;", {k: v.shape for k, v in g.items() if k.startswith(("case1111", "pairs_", "drop_a", "match_"))})
