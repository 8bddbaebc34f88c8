"""The rule of glimpse_amd.displacements restated in NumPy (INPUTS.md, "Displacements: the rule"), and the scenes the
tests share.  Written from the rule, not from the kernel: the integer path in exact int64 sums per offset, the float path
as float64 accumulators that take one product per template pixel in row-major order (vectorised over the offsets, which
does not change any sum's order).  No GPU, no library."""
import numpy as np

STATUS = ("matched", "peak on the edge", "no valid offset", "flat template", "template outside")
MATCHED, EDGE, NO_OFFSET, FLAT, OUTSIDE = range(5)
GUESS_LIMIT = 1 << 24


def plane(array):
    """The plane that is matched: 2-D uint8 as it is; everything else float32, three channels averaged first."""
    array = np.asarray(array)
    if array.ndim == 3:
        array = array.mean(axis=2)
    return array if array.dtype == np.uint8 else array.astype(np.float32)


def box(u, v, w, h, shape):
    """(l, t) of the template box of one point, or None where Observer.tile_box would raise (or uv is not finite)."""
    rows, cols = shape
    if not (np.isfinite(u) and np.isfinite(v)):
        return None
    edges = (u - w * 0.5, u + w * 0.5, v - h * 0.5, v + h * 0.5)
    if not (0 <= edges[0] <= cols and 0 <= edges[1] <= cols and 0 <= edges[2] <= rows and 0 <= edges[3] <= rows):
        return None
    return int(np.floor(edges[0] + 0.5)), int(np.floor(edges[2] + 0.5))


def whole(guess):
    """rint of one guess coordinate; not finite, or beyond the limit: the limit."""
    if not np.isfinite(guess):
        return GUESS_LIMIT
    return int(min(max(np.rint(guess), -GUESS_LIMIT), GUESS_LIMIT))


def windows(b, x0, y0, w, h, rx, ry):
    """S [2 ry + 1][2 rx + 1][h][w]: the windows of every offset (zeros where a window leaves `b`), and `inside`
    [2 ry + 1][2 rx + 1]: the window lies in `b`."""
    rows, cols = b.shape
    S = np.zeros((2 * ry + 1, 2 * rx + 1, h, w), dtype=b.dtype)
    inside = np.zeros((2 * ry + 1, 2 * rx + 1), dtype=bool)
    for j in range(2 * ry + 1):
        for i in range(2 * rx + 1):
            x, y = x0 + i - rx, y0 + j - ry
            if 0 <= x and x + w <= cols and 0 <= y and y + h <= rows:
                S[j, i], inside[j, i] = b[y:y + h, x:x + w], True
    return S, inside


def surface_u8(T, S):
    """(vt, scores [ny][nx]) on the integer path: exact int64 sums, then one product, square root and division."""
    n = T.size
    T, S = T.astype(np.int64), S.astype(np.int64)
    st, stt = int(T.sum()), int((T * T).sum())
    vt = n * stt - st * st
    ss, sq, sx = S.sum(axis=(2, 3)), (S * S).sum(axis=(2, 3)), (S * T).sum(axis=(2, 3))
    vs = n * sq - ss * ss
    num = n * sx - st * ss
    with np.errstate(all="ignore"):
        score = num.astype(np.float64) / np.sqrt(np.float64(vt) * vs.astype(np.float64))
    return vt, np.where(vs > 0, score, np.nan)


def surface_f32(T, S):
    """(vt, scores [ny][nx]) on the float path: float64 accumulators from 0.0, one product per template pixel in row-major
    order -- a slab of all offsets per step."""
    h, w = T.shape
    n = np.float64(w * h)
    T64, S64 = T.astype(np.float64), S.astype(np.float64)
    st = stt = np.float64(0.0)
    ss, sq, sx = (np.zeros(S.shape[:2]) for _ in range(3))
    with np.errstate(all="ignore"):
        for r in range(h):
            for c in range(w):
                t, s = T64[r, c], S64[:, :, r, c]
                st = st + t
                stt = stt + t * t
                ss = ss + s
                sq = sq + s * s
                sx = sx + t * s
        vt = n * stt - st * st
        vs = n * sq - ss * ss
        num = n * sx - st * ss
        score = num / np.sqrt(vt * vs)
    return vt, np.where(vs > 0, score, np.nan)


def vertex(a_, c_, b_):
    with np.errstate(all="ignore"):
        den = (a_ - 2.0 * c_) + b_
        return (a_ - b_) / (2.0 * den) if den < 0 else 0.0


def match_point(a, b, u, v, size, reach, guess, subpixel):
    """One point: (duv (2,), score, status, surface [2 ry + 1][2 rx + 1])."""
    (w, h), (rx, ry) = size, reach
    nan_surface = np.full((2 * ry + 1, 2 * rx + 1), np.nan)
    corner = box(u, v, w, h, a.shape)
    if corner is None:
        return (np.nan, np.nan), np.nan, OUTSIDE, nan_surface
    l, t = corner
    gu, gv = (whole(guess[0]), whole(guess[1])) if guess is not None else (0, 0)
    T = a[t:t + h, l:l + w]
    S, inside = windows(b, l + gu, t + gv, w, h, rx, ry)
    vt, score = (surface_u8 if a.dtype == np.uint8 else surface_f32)(T, S)
    if not vt > 0:
        return (np.nan, np.nan), np.nan, FLAT, nan_surface
    surface = np.where(inside & np.isfinite(score), score, np.nan)
    if np.isnan(surface).all():
        return (np.nan, np.nan), np.nan, NO_OFFSET, surface
    j, i = np.unravel_index(np.nanargmax(surface), surface.shape)  # (the first of equals in row-major order)
    du = dv = 0.0
    status = MATCHED
    if subpixel:
        if i == 0 or i == 2 * rx or np.isnan(surface[j, i - 1]) or np.isnan(surface[j, i + 1]):
            status = EDGE
        else:
            du = vertex(surface[j, i - 1], surface[j, i], surface[j, i + 1])
        if j == 0 or j == 2 * ry or np.isnan(surface[j - 1, i]) or np.isnan(surface[j + 1, i]):
            status = EDGE
        else:
            dv = vertex(surface[j - 1, i], surface[j, i], surface[j + 1, i])
    return (np.float64(gu + int(i) - rx) + du, np.float64(gv + int(j) - ry) + dv), surface[j, i], status, surface


def displacements(a, b, uv, size=(31, 31), reach=(16, 16), guess=None, subpixel=True):
    """(duv (n, 2), score (n,), status (n,) uint8, surface (n, 2 ry + 1, 2 rx + 1)) of two frames by the rule."""
    a, b = plane(a), plane(b)
    if a.dtype != b.dtype:
        a, b = a.astype(np.float32), b.astype(np.float32)
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    n = len(uv)
    duv, score = np.empty((n, 2)), np.empty(n)
    status = np.empty(n, dtype=np.uint8)
    surface = np.empty((n, 2 * reach[1] + 1, 2 * reach[0] + 1))
    for k in range(n):
        duv[k], score[k], status[k], surface[k] = match_point(a, b, uv[k, 0], uv[k, 1], size, reach,
                                                              None if guess is None else np.asarray(guess)[k], subpixel)
    return duv, score, status, surface


# ---- scenes ----------------------------------------------------------------------------------------------------------------

def noise_u8(shape=(61, 97), seed=0):
    """White noise, uint8 (rows, cols); the default is 97 x 61 pixels, a width that is no multiple of 4."""
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def moved(frame, dx, dy, out):
    """`out` with the content of `frame` at (x, y) written to (x + dx, y + dy); what moves in keeps `out`'s pixels."""
    rows, cols = frame.shape
    ys, yd = (slice(0, rows - dy), slice(dy, rows)) if dy >= 0 else (slice(-dy, rows), slice(0, rows + dy))
    xs, xd = (slice(0, cols - dx), slice(dx, cols)) if dx >= 0 else (slice(-dx, cols), slice(0, cols + dx))
    out[yd, xd] = frame[ys, xs]
    return out


def shifted(frame, dx, dy, seed=1):
    """`frame` moved by whole pixels (content at (x, y) goes to (x + dx, y + dy)); what moves in is fresh noise."""
    rng = np.random.default_rng(seed)
    if frame.dtype == np.uint8:
        out = rng.integers(0, 256, size=frame.shape, dtype=np.uint8)
    else:
        out = rng.random(frame.shape).astype(frame.dtype)
    return moved(frame, dx, dy, out)


def periodic_u8(shape=(61, 97), period=(7, 5), seed=5):
    """A random cell of period[1] rows x period[0] columns tiled over the frame: matched against itself, every offset
    that is a whole number of periods from the true one has the same window, hence the same score in every bit."""
    px, py = period
    rows, cols = shape
    cell = np.random.default_rng(seed).integers(0, 256, size=(py, px), dtype=np.uint8)
    return np.tile(cell, (rows // py + 1, cols // px + 1))[:rows, :cols].copy()


def half_striped_u8(shape=(61, 97), split=40, seed=5):
    """periodic_u8 up to column `split`; from there on every row is constant (rows of period 5).  Against itself, a
    template from the striped part ties with every window that lies in that part: the first of them has a lower
    neighbour before it and a tied one after it."""
    frame = periodic_u8(shape, (7, 5), seed)
    frame[:, split:] = periodic_u8(shape, (1, 5), seed + 1)[:, split:]
    return frame


SATURATED_SHIFT = (2, -1)


def saturated_u8(shape=(130, 160), seed=3):
    """(a, b): pixels drawn from {254, 255}, and the frame moved by SATURATED_SHIFT, where what moves in is noise of
    250 .. 255: the sums of a window are as large as uint8 pixels make them."""
    a = np.random.default_rng(seed).integers(254, 256, size=shape, dtype=np.uint8)
    return a, np.maximum(shifted(a, *SATURATED_SHIFT, seed=seed + 1), 250)


def holes_u8(shape=(130, 160), seed=4, spacing=32):
    """(a, b): all 255 but for single pixels of 0, one at a random place of every spacing x spacing cell, and the frame
    moved by SATURATED_SHIFT (255 moves in): n sum(S^2) - sum(S)^2 is a small integer under the largest sum(S^2)."""
    rng = np.random.default_rng(seed)
    rows, cols = shape
    a = np.full(shape, 255, dtype=np.uint8)
    for y in range(0, rows, spacing):
        for x in range(0, cols, spacing):
            a[min(rows - 1, y + rng.integers(spacing)), min(cols - 1, x + rng.integers(spacing))] = 0
    return a, moved(a, *SATURATED_SHIFT, np.full(shape, 255, dtype=np.uint8))


SUBNORMAL_UNIT = np.float32(1e-42)  # 714 times the smallest float32 subnormal; 256 of them stay far below 2^-126
SUBNORMAL_SHIFT = (1, -2)


def subnormal_f32(shape=(61, 97), seed=6):
    """(a, b): white noise of 1 .. 256 times SUBNORMAL_UNIT, every pixel a nonzero float32 subnormal, and the frame
    moved by SUBNORMAL_SHIFT (such noise moves in)."""
    a = noise_u8(shape, seed)
    b = shifted(a, *SUBNORMAL_SHIFT, seed=seed + 1)
    return tuple((f.astype(np.float32) + np.float32(1)) * SUBNORMAL_UNIT for f in (a, b))


HUGE_UNIT = np.float32(3e37)


def huge_f32(shape=(61, 97), seed=8):
    """(a, b): white noise of 1/32 .. 8 times HUGE_UNIT (up to 2.4e38, float32 ends at 3.4e38) and the frame moved by
    SUBNORMAL_SHIFT: the products of two pixels reach 5.8e76 and every sum of the rule stays finite in float64."""
    a = noise_u8(shape, seed)
    b = shifted(a, *SUBNORMAL_SHIFT, seed=seed + 1)
    return tuple((f.astype(np.float32) + np.float32(1)) / np.float32(32) * HUGE_UNIT for f in (a, b))


def tied(surface):
    """[the offsets o = j * nxo + i whose score equals the surface's largest in every bit] for each point of
    `surface` (n, nyo, nxo); empty where a point has no valid offset."""
    flat = np.asarray(surface).reshape(len(surface), -1)
    out = []
    for row in flat:
        valid = ~np.isnan(row)
        out.append(np.flatnonzero(valid & (row == row[valid].max())) if valid.any() else np.empty(0, dtype=np.int64))
    return out


TEXTURE_SEED, TEXTURE_BANDWIDTH = 7, 0.3  # cycles per pixel: the texture's spectrum is zero beyond it


def texture(shape=(96, 128), shift=(0.0, 0.0)):
    """A band-limited random texture (seed TEXTURE_SEED, no energy above TEXTURE_BANDWIDTH cycles per pixel), moved by
    `shift` = (dx, dy) pixels in the Fourier domain, as float64 of mean 127.5 and standard deviation 40."""
    rng = np.random.default_rng(TEXTURE_SEED)
    spectrum = np.fft.fft2(rng.standard_normal(shape))
    fy, fx = np.meshgrid(np.fft.fftfreq(shape[0]), np.fft.fftfreq(shape[1]), indexing="ij")
    spectrum[np.hypot(fx, fy) > TEXTURE_BANDWIDTH] = 0
    spectrum = spectrum * np.exp(-2j * np.pi * (fx * shift[0] + fy * shift[1]))
    image = np.fft.ifft2(spectrum).real
    return 127.5 + (image - image.mean()) * (40.0 / image.std())


def edge_points(shape, size):
    """Points whose template boxes lie flush with each edge and corner of a frame, and some inside: (n, 2).  With the
    interior points the left edge l of the boxes takes all four values modulo 4."""
    rows, cols = shape
    w, h = size
    left, right, top, bottom = w / 2, cols - w / 2, h / 2, rows - h / 2
    cx, cy = cols / 2, rows / 2
    points = [(left, top), (right, top), (left, bottom), (right, bottom), (cx, top), (cx, bottom), (left, cy), (right, cy)]
    points += [(cx + k, cy + 0.25 * k) for k in range(-2, 3)]
    return np.array(points, dtype=np.float64)
