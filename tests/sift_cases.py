"""The images of the SIFT tests (tests/test_sift_restated.py, tests/test_sift_host.py, tests/test_gpu_sift.py) and the
restatement's stages of each, computed once a session."""
import functools

import numpy as np
from scipy.ndimage import gaussian_filter

from tests import sift_restated as sr

SIZES = {"61x47": (47, 61), "47x61": (61, 47), "256x192": (192, 256), "strip": (40, 12), "5x5": (5, 5),
         "300x400": (300, 400)}  # (rows, columns)
FULL = ("61x47", "47x61", "256x192")  # the images on which every branch of the rule must be seen to fire
LIST_SLOTS = 4096  # the candidate list of a fresh handle (glh_sift.hip); "300x400" yields more, the others fewer
SEED = 1


def blob(s, amplitude=180.0, centre=(40.3, 37.6), n=80, second=None):
    """round(40 + amplitude exp(-d^2 / 2 s^2)) about `centre` (x, y); `second` = (dx, dy, amplitude) adds another."""
    y, x = np.mgrid[0:n, 0:n]
    a = 40.0 + amplitude * np.exp(-((x - centre[0]) ** 2 + (y - centre[1]) ** 2) / (2.0 * s * s))
    if second is not None:
        a = a + second[2] * np.exp(-((x - centre[0] - second[0]) ** 2 + (y - centre[1] - second[1]) ** 2) / (2.0 * s * s))
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


def texture(h, w, seed=SEED):
    """Seeded noise smoothed at three scales, blobs of both signs, and two thin modulated lines (edge responses)."""
    rng = np.random.default_rng(seed)
    a = (gaussian_filter(rng.standard_normal((h, w)), 1.2) * 2.0 + gaussian_filter(rng.standard_normal((h, w)), 3.0) * 5.0
         + gaussian_filter(rng.standard_normal((h, w)), 7.0) * 12.0)
    a = (a - a.min()) / (a.max() - a.min()) * 170 + 30
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(max(4, h * w // 500)):
        cy, cx, s, amp = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(1.5, 7), rng.uniform(-70, 70)
        a += amp * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    for _ in range(2):
        t = rng.uniform(0, np.pi)
        d = (xx - rng.uniform(0.3, 0.7) * w) * np.sin(t) - (yy - rng.uniform(0.3, 0.7) * h) * np.cos(t)
        a += rng.choice([-1, 1]) * 60 * np.exp(-d * d / 2.0) * (1 + 0.5 * np.sin((xx + yy) / 2.5))
    return np.clip(np.round(a), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def image(name):
    a = texture(*SIZES[name])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def stages(name, **params):
    """The restatement's stages of image `name` (shared: read, never written)."""
    return sr.stages(image(name), **params)


def mask_of(name):
    """Non-zero on a band and a block: some keypoints in, some out."""
    h, w = SIZES[name]
    m = np.zeros((h, w), np.uint8)
    m[h // 4: 3 * h // 4, :] = 1
    m[:, : w // 3] = 0
    m[: h // 8, w // 2:] = 255
    return m
