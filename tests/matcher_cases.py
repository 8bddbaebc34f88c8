"""What tests/test_matcher_host.py and tests/test_gpu_matcher.py share: the fixtures of tools/make_golden_matcher.py
(tests/golden/matcher_pairs.npz, matcher_sequence.npz) as glimpse_amd objects."""
import datetime
import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = datetime.timedelta(hours=1)
# name -> (maxdt in hours or None, seq, imgs): tools/make_golden_matcher.py SETTINGS
SETTINGS = {"all": (None, None, None), "maxdt2": (2, None, None), "seq12": (None, (1, 2), None),
            "maxdt1_seq3": (1, (3,), None), "seq1_imgs25": (None, (1,), (2, 5)), "maxdt4_imgs0": (4, None, (0,))}
OPTIONS = list(itertools.product((0, 1), repeat=4))  # cross_check, max_ratio, max_distance, return_ratios


def load(name):
    return np.load(os.path.join(GOLDEN, name))


class KeyPoint:
    """What the reference reads of a cv2.KeyPoint."""

    def __init__(self, pt):
        self.pt = pt


def option_kwargs(g, c, r, d, w):
    return dict(cross_check=bool(c), max_ratio=float(g["max_ratio"]) if r else None,
                max_distance=float(g["max_distance"]) if d else None, return_ratios=bool(w))


def expected(g, c, r, d, w):
    return [g[f"case{c}{r}{d}{w}_{name}"] for name in ("uva", "uvb", "ratios")[: 2 + w]]


def same(result, golden):
    assert len(result) == len(golden)
    for a, b in zip(result, golden):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def setting_kwargs(name):
    maxdt, seq, imgs = SETTINGS[name]
    return dict(maxdt=None if maxdt is None else maxdt * H, seq=seq, imgs=imgs)


def sequence_matcher(g, paths=None):
    """A KeypointMatcher of the six images of matcher_sequence.npz with their keypoints."""
    import glimpse_amd
    from glimpse_amd import optimize

    v = g["internals"]
    internals = dict(imgsz=v[0:2], f=v[2:4], c=v[4:6], k=v[6:12], p=v[12:14])
    images = [glimpse_amd.Image(f"frames/img_{i}.jpg" if paths is None else paths[i],
                                cam=glimpse_amd.Camera(viewdir=view, **internals),
                                datetime=datetime.datetime(2020, 1, 1) + int(h) * H)
              for i, (view, h) in enumerate(zip(g["viewdirs"], g["hours"]))]
    model = optimize.KeypointMatcher(images)
    model.keypoints = sequence_keypoints(g)
    return model


def sequence_keypoints(g):
    off = np.concatenate(([0], np.cumsum(g["sizes"])))
    return [(g["points"][a:b], g["descriptors"][a:b]) for a, b in zip(off[:-1], off[1:])]


def pair_slices(g):
    off = g["match_offsets"]
    return [slice(int(a), int(b)) for a, b in zip(off[:-1], off[1:])]


def assert_pairs_equal_golden(matches, g, weights=True):
    """`matches` (a PairMatches of setting "all", max_ratio, weights) against the reference's, pair for pair."""
    assert np.array_equal(np.column_stack([matches.row, matches.col]), g["pairs_all"])
    for m, s in zip(matches.data, pair_slices(g)):
        assert np.array_equal(m.uvs[0], g["match_uva"][s]) and np.array_equal(m.uvs[1], g["match_uvb"][s])
        if weights:
            assert np.array_equal(m.weights, g["match_weights"][s])
