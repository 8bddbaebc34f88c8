"""NumPy restatement of the CLAHE rule of INPUTS.md ("CLAHE: the rule"), which glimpse_amd/csrc/glh_clahe.hip computes on the
device (test-only).  The histograms are integers and every pixel is one fixed float32 expression, each product and sum
rounded on its own (NumPy never contracts), so the device's bytes equal these.  `CASES` and `frame` are the table both
tests/test_clahe.py (CPU) and tests/test_gpu_clahe.py (device) run."""
import functools

import numpy as np

BINS = 256


def reflect(i, n):
    """Index i >= 0 of an axis of n cells extended by reflection without the edge cell (BORDER_REFLECT_101, np.pad's
    "reflect"): i itself inside, 2 (n - 1) - i beyond.  At most n cells are ever added, so the only index that formula
    leaves outside is -1 (a full grid's worth of cells added to an axis exactly that long), which reflects once more, to 1;
    an axis of one cell repeats it."""
    i = np.asarray(i)
    r = np.where(i < n, i, np.abs(2 * (n - 1) - i))
    return r if n > 1 else np.zeros_like(r)


def geometry(h, w, grid):
    """(ext_h, ext_w, th, tw) of an h x w image under grid = (tilesX, tilesY)."""
    tiles_x, tiles_y = grid
    if w % tiles_x == 0 and h % tiles_y == 0:
        ext_h, ext_w = h, w
    else:
        ext_h, ext_w = h + (tiles_y - h % tiles_y), w + (tiles_x - w % tiles_x)
    return ext_h, ext_w, ext_h // tiles_y, ext_w // tiles_x


def extend(src, grid):
    ext_h, ext_w, _, _ = geometry(*src.shape, grid)
    return src[reflect(np.arange(ext_h), src.shape[0])[:, None], reflect(np.arange(ext_w), src.shape[1])[None, :]]


def clip_limit(clip, area):
    if clip <= 0:
        return 0
    return max(int(float(clip) * area / BINS), 1)


def redistribute_loop(hist, lim):
    """Step 3 of the rule on one tile's histogram, the residual handed out by the literal loop.  Returns (hist, residual,
    step); step is 0 when there is no residual."""
    hist = [int(v) for v in hist]
    clipped = 0
    for i in range(BINS):
        if hist[i] > lim:
            clipped += hist[i] - lim
            hist[i] = lim
    batch, residual = clipped // BINS, clipped % BINS
    for i in range(BINS):
        hist[i] += batch
    step = 0
    if residual != 0:
        step = max(BINS // residual, 1)
        left, i = residual, 0
        while i < BINS and left > 0:
            hist[i] += 1
            i += step
            left -= 1
    return np.array(hist, np.int64), residual, step


def redistribute_closed(hist, lim):
    """The same by the closed form: bin i gets one of the residual when i % step == 0 and i / step < residual."""
    hist = np.asarray(hist, np.int64)
    clipped = int(np.maximum(hist - lim, 0).sum())
    hist = np.minimum(hist, lim) + clipped // BINS
    residual = clipped % BINS
    step = 0
    if residual != 0:
        step = max(BINS // residual, 1)
        i = np.arange(BINS)
        hist = hist + ((i % step == 0) & (i // step < residual))
    return hist, residual, step


def luts(src, clip=40.0, grid=(8, 8), redistribute=redistribute_closed, trace=None):
    """uint8 [tilesY][tilesX][256]: steps 1 to 4.  `trace` (a dict) receives what the case reached: "padded", "lim" and per
    tile "clipped", "residual", "step"."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    tiles_x, tiles_y = grid
    ext = extend(src, grid)
    _, _, th, tw = geometry(*src.shape, grid)
    area = tw * th
    lim = clip_limit(clip, area)
    scale = np.float32(255) / np.float32(area)
    out = np.empty((tiles_y, tiles_x, BINS), np.uint8)
    reached = dict(padded=ext.shape != src.shape, lim=lim, clipped=[], residual=[], step=[])
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            hist = np.bincount(ext[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=BINS).astype(np.int64)
            if lim > 0:
                reached["clipped"].append(int(np.maximum(hist - lim, 0).sum()))
                hist, residual, step = redistribute(hist, lim)
                reached["residual"].append(residual)
                reached["step"].append(step)
            assert hist.sum() == area
            product = np.cumsum(hist).astype(np.float32) * scale  # float32 x float32, rounded once
            out[ty, tx] = np.clip(np.rint(product), 0, 255).astype(np.uint8)
    if trace is not None:
        trace.update(reached)
    return out


def axis_weights(n, t, tiles):
    """Step 5 along one axis of n source cells with tiles of t cells: (i1, i2, a, a1), float32 weights."""
    inv = np.float32(1) / np.float32(t)
    f = np.arange(n).astype(np.float32) * inv - np.float32(0.5)
    i1 = np.floor(f).astype(np.int64)
    a = f - i1.astype(np.float32)  # before clamping
    a1 = np.float32(1) - a
    i2 = np.minimum(i1 + 1, tiles - 1)
    i1 = np.maximum(i1, 0)
    assert a.dtype == a1.dtype == np.float32
    return i1, i2, a, a1


def blend(src, L, grid):
    """Step 5: uint8 [h][w] of `src` under the tables L [tilesY][tilesX][256]."""
    h, w = src.shape
    tiles_x, tiles_y = grid
    _, _, th, tw = geometry(h, w, grid)
    tx1, tx2, xa, xa1 = axis_weights(w, tw, tiles_x)
    ty1, ty2, ya, ya1 = axis_weights(h, th, tiles_y)
    Lf = L.astype(np.float32)
    v = src.astype(np.int64)
    ty1, ty2, ya, ya1 = ty1[:, None], ty2[:, None], ya[:, None], ya1[:, None]
    top = Lf[ty1, tx1, v] * xa1 + Lf[ty1, tx2, v] * xa
    bottom = Lf[ty2, tx1, v] * xa1 + Lf[ty2, tx2, v] * xa
    res = top * ya1 + bottom * ya
    assert res.dtype == np.float32
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def apply(src, clip=40.0, grid=(8, 8), trace=None):
    """(dst uint8 [h][w], luts) of the whole rule."""
    src = np.asarray(src)
    L = luts(src, clip, grid, trace=trace)
    return blend(src, L, grid), L


def channel_mean(array):
    """gray = (sum of the channels) // c of uint8 [h][w][c]."""
    array = np.asarray(array)
    assert array.dtype == np.uint8 and array.ndim == 3
    return (array.astype(np.int64).sum(axis=2) // array.shape[2]).astype(np.uint8)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def snow(h, w, seed=0):
    """A synthetic snow frame: a bright smooth band with small noise under a darker noisy third."""
    rng = np.random.default_rng(1000 + seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    bright = 232.0 + 9.0 * np.sin(x / max(w, 1) * 5.0 + y / max(h, 1) * 3.0) + rng.normal(0.0, 1.5, (h, w))
    dark = 95.0 + 30.0 * np.sin(x / 7.0) * np.cos(y / 5.0) + rng.normal(0.0, 22.0, (h, w))
    a = np.where(y < h / 3.0, dark, bright)
    return np.clip(np.rint(a), 0, 255).astype(np.uint8)


def stripes(h, w):
    """Only 0 and 255, in vertical stripes three and five pixels wide: every count lands in two bins."""
    return np.broadcast_to(np.where(np.arange(w) % 8 < 3, 0, 255).astype(np.uint8), (h, w)).copy()


# name -> (h, w, clipLimit, (tilesX, tilesY), kind)
CASES = {
    "divisible": (48, 64, 40.0, (8, 8), "snow"),
    "padded-odd": (47, 61, 40.0, (8, 8), "snow"),
    "grid3x5-clip2": (47, 61, 2.0, (3, 5), "snow"),
    "noclip-rows-padded": (33, 40, 0.0, (4, 4), "snow"),
    "one-tile-lim1": (16, 16, 0.001, (1, 1), "snow"),
    "tiles2x2": (9, 11, 40.0, (8, 8), "snow"),
    "slices-clip3": (300, 517, 3.0, (8, 8), "snow"),
    "constant255": (64, 64, 40.0, (8, 8), "constant"),
    "large-2x2": (1024, 1536, 40.0, (2, 2), "snow"),
    "stripes": (96, 200, 40.0, (8, 8), "stripes"),
    "grid-as-wide-as-the-image": (9, 4, 40.0, (4, 2), "snow"),  # a full grid of columns added: index -1 reflects to 1
}


@functools.lru_cache(maxsize=None)
def frame(name):
    h, w, _, _, kind = CASES[name]
    a = {"snow": lambda: snow(h, w), "constant": lambda: np.full((h, w), 255, np.uint8), "stripes": lambda: stripes(h, w)}[kind]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(name):
    """(dst, luts, trace) of case `name` (shared: read, never written)."""
    _, _, clip, grid, _ = CASES[name]
    trace = {}
    dst, L = apply(frame(name), clip, grid, trace=trace)
    dst.setflags(write=False)
    L.setflags(write=False)
    return dst, L, trace


def colour(h, w, c, seed=0):
    """uint8 [h][w][c]: the snow frame with a different tint and noise per channel."""
    rng = np.random.default_rng(2000 + seed)
    base = snow(h, w, seed).astype(np.int64)
    a = np.stack([base + rng.integers(-9, 10, (h, w)) - 6 * k for k in range(c)], axis=2)
    return np.clip(a, 0, 255).astype(np.uint8)


def sequence(n=2, h=96, w=128):
    """uint8 [h][w][3] frames of one glacier scene: low-contrast texture near white (what SIFT finds little in) under a
    darker sky, each frame moved by a few pixels."""
    from scipy.ndimage import gaussian_filter

    rng = np.random.default_rng(77)
    H, W = h + 16, w + 16
    t = gaussian_filter(rng.standard_normal((H, W)), 1.5) * 9.0 + gaussian_filter(rng.standard_normal((H, W)), 4.0) * 14.0
    y = np.arange(H)[:, None]
    scene = np.where(y < H // 4, 120.0 + t * 6.0, 236.0 + t)
    frames = []
    for k in range(n):
        crop = scene[4 * k:4 * k + h, 6 * k:6 * k + w]
        frames.append(np.clip(np.rint(np.stack([crop - 3.0, crop, crop + 2.0], axis=2)), 0, 255).astype(np.uint8))
    return frames
