"""NumPy restatement of the SIFT rule of INPUTS.md ("SIFT: the rule"), which glimpse_amd/csrc/glh_sift.hip computes on the
device (test-only).  The pyramid is float32; everything per keypoint is float64 made of + - x /, sqrt, rint, floor and
ldexp alone, in the order written here, so that the device's results equal these in every bit.  The elementary functions
(`exp_own`, `pow2_own`, `atan2_own`, `sincos_own`) are the rule's own, repeated from glh_sift.hip operation for operation.
The two histograms are summed in fixed point (every contribution is rint(v * 2^20) as an integer), so their sums do not
depend on the order of the cells."""
import math

import numpy as np
from scipy.ndimage import correlate1d

BORDER = 5
MAX_STEPS = 5
FIX = float(1 << 20)
IS = 1.0 / 255.0
EPS = 2.0 ** -52
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
EXP_C = [1.0 / math.factorial(n) for n in range(14)]
PIO2_HI = float.fromhex("0x1.921fb54400000p+0")
PIO2_LO = float.fromhex("0x1.0b4611a626331p-34")
TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
D2R = float.fromhex("0x1.1df46a2529d39p-6")  # pi / 180
SIN_C = [(-1.0) ** k / math.factorial(2 * k + 1) for k in range(9)]  # r, r^3 .. r^17
COS_C = [(-1.0) ** k / math.factorial(2 * k) for k in range(9)]  # 1, r^2 .. r^16
AT1 = float.fromhex("0x1.ca44dc8279760p+5")  # OpenCV's fastAtan2 polynomial, in degrees
AT3 = float.fromhex("-0x1.2aaddbf772879p+4")
AT5 = float.fromhex("0x1.1d3f7d350aa15p+3")
AT7 = float.fromhex("-0x1.4515b1b4863e3p+1")
REJECT = {1: "singular", 2: "border", 3: "unsettled", 4: "contrast", 5: "edge", 6: "step"}

Params = dict(nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10.0, sigma=1.6)


def exp_own(x):
    """e^x: x = k ln2 + r with k = rint(x / ln2) and ln2 in two parts, the degree-13 Taylor polynomial of r by Horner,
    scaled by 2^k.  0 below -700."""
    x = np.asarray(x, np.float64)
    xs = np.maximum(x, -700.0)
    kf = np.rint(xs * INV_LN2)
    r = (xs - kf * LN2_HI) - kf * LN2_LO
    p = np.full_like(r, EXP_C[13])
    for n in range(12, -1, -1):
        p = p * r + EXP_C[n]
    return np.where(x < -700.0, 0.0, np.ldexp(p, kf.astype(np.int32)))


def pow2_own(x):
    return exp_own(x * LN2)


def atan2_own(y, x):
    """The angle of (x, y) in degrees, [0, 360]: OpenCV's fastAtan2 polynomial in float64."""
    y, x = np.asarray(y, np.float64), np.asarray(x, np.float64)
    ax, ay = np.abs(x), np.abs(y)
    big = ax >= ay
    c = np.where(big, ay, ax) / (np.where(big, ax, ay) + EPS)
    c2 = c * c
    a = (((AT7 * c2 + AT5) * c2 + AT3) * c2 + AT1) * c
    a = np.where(big, a, 90.0 - a)
    a = np.where(x < 0.0, 180.0 - a, a)
    return np.where(y < 0.0, 360.0 - a, a)


def sincos_own(deg):
    """(sin, cos) of an angle in degrees, 0 <= deg <= 360 (scalars)."""
    rad = deg * D2R
    k = float(np.rint(rad * TWO_OVER_PI))
    r = (rad - k * PIO2_HI) - k * PIO2_LO
    z = r * r
    s, c = SIN_C[8], COS_C[8]
    for n in range(7, -1, -1):
        s = s * z + SIN_C[n]
        c = c * z + COS_C[n]
    s = s * r
    q = int(k) & 3
    return [(s, c), (c, -s), (-s, -c), (-c, s)][q]


# ---- the pyramid -----------------------------------------------------------------------------------------------------
def tables(S, sigma):
    """[(radius, weights float64)] of the S + 3 blurs of an octave: [0] the base's, [i] layer i - 1 -> layer i."""
    k = 2.0 ** (1.0 / S)
    sigs = [math.sqrt(max(sigma * sigma - 1.0, 0.01))]
    for i in range(1, S + 3):
        prev = math.pow(k, i - 1) * sigma
        total = prev * k
        sigs.append(math.sqrt(total * total - prev * prev))
    out = []
    for sig in sigs:
        r = (int(np.rint(8.0 * sig + 1.0)) | 1) // 2
        x = np.arange(-r, r + 1, dtype=np.float64)
        w = np.exp(-(x * x) / (2.0 * sig * sig))
        out.append((r, w / w.sum()))
    return out


def blur(a, table):
    r, w = table
    a = correlate1d(a, w, axis=0, output=np.float32, mode="mirror")
    return correlate1d(a, w, axis=1, output=np.float32, mode="mirror")


def _double_axis(n):
    i = np.arange(2 * n)
    k = i >> 1
    even = (i & 1) == 0
    i0 = np.where(even, np.maximum(k - 1, 0), k)
    i1 = np.where(even, k, np.minimum(k + 1, n - 1))
    w0 = np.where(even, 0.25, 0.75).astype(np.float32)
    return i0, i1, w0, (np.float32(1.0) - w0).astype(np.float32)


def base_image(img):
    a = np.asarray(img, np.uint8).astype(np.float32)
    r0, r1, wr0, wr1 = _double_axis(a.shape[0])
    c0, c1, wc0, wc1 = _double_axis(a.shape[1])
    t = a[:, c0] * wc0 + a[:, c1] * wc1
    return (t[r0] * wr0[:, None] + t[r1] * wr1[:, None]).astype(np.float32)


def octave_sizes(h, w):
    H, W, out = 2 * h, 2 * w, []
    while min(H, W) >= 12:
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def pyramid(img, S, sigma):
    """(gauss[o][0 .. S + 2], dog[o][0 .. S + 1]) float32."""
    tabs = tables(S, sigma)
    gauss, dog = [], []
    for o, _ in enumerate(octave_sizes(*np.shape(img))):
        first = blur(base_image(img), tabs[0]) if o == 0 else np.ascontiguousarray(gauss[o - 1][S][::2, ::2])
        layers = [first]
        for i in range(1, S + 3):
            layers.append(blur(layers[-1], tabs[i]))
        gauss.append(layers)
        dog.append([layers[i + 1] - layers[i] for i in range(S + 2)])
    return gauss, dog


def contrast_floor(S, contrast):
    return float(math.floor(0.5 * contrast / S * 255.0))


def candidates(dog, S, contrast):
    """int32 (n, 4): (octave, layer, row, column) ascending."""
    thr = np.float32(contrast_floor(S, contrast))
    out = []
    b = BORDER
    for o, d in enumerate(dog):
        H, W = d[0].shape
        if H <= 2 * b or W <= 2 * b:
            continue
        for l in range(1, S + 1):
            v = d[l][b:H - b, b:W - b]
            ge = np.ones(v.shape, bool)
            le = np.ones(v.shape, bool)
            for dl in (-1, 0, 1):
                for dr in (-1, 0, 1):
                    for dc in (-1, 0, 1):
                        if dl or dr or dc:
                            n = d[l + dl][b + dr:H - b + dr, b + dc:W - b + dc]
                            ge &= v >= n
                            le &= v <= n
            m = (np.abs(v) > thr) & (((v > 0) & ge) | ((v < 0) & le))
            rr, cc = np.nonzero(m)
            out.extend((o, l, int(r) + b, int(c) + b) for r, c in zip(rr, cc))
    return np.array(out, np.int32).reshape(-1, 4)


# ---- per keypoint ----------------------------------------------------------------------------------------------------
def solve3(a):
    """x of the 3 x 4 augmented system `a` by Gaussian elimination, in each column the pivot the row of largest |entry|
    (the first of equals); None when a pivot is zero."""
    a = [list(row) for row in a]
    for k in range(3):
        p = k
        for i in range(k + 1, 3):
            if abs(a[i][k]) > abs(a[p][k]):
                p = i
        if a[p][k] == 0.0:
            return None
        a[k], a[p] = a[p], a[k]
        for i in range(k + 1, 3):
            f = a[i][k] / a[k][k]
            for j in range(k, 4):
                a[i][j] = a[i][j] - f * a[k][j]
    x2 = a[2][3] / a[2][2]
    x1 = (a[1][3] - a[1][2] * x2) / a[1][1]
    x0 = (a[0][3] - a[0][1] * x1 - a[0][2] * x2) / a[0][0]
    return x0, x1, x2


def refine(d, S, contrast, edge, sigma, o, l, r, c):
    """One candidate: (status, record).  status 0: record = (o, l, r, c, xc, xr, xi, contr, size, ptx, pty, scl) with the
    settled cell; else the number of the rule that rejected it (REJECT) and whether it had moved."""
    H, W = d[0].shape
    ds, ss, cs = IS * 0.5, IS, IS * 0.25
    moved = False
    for step in range(MAX_STEPS):
        D = lambda dl, dr, dc: float(d[l + dl][r + dr, c + dc])  # noqa: E731
        dx = (D(0, 0, 1) - D(0, 0, -1)) * ds
        dy = (D(0, 1, 0) - D(0, -1, 0)) * ds
        dz = (D(1, 0, 0) - D(-1, 0, 0)) * ds
        v2 = D(0, 0, 0) * 2.0
        dxx = (D(0, 0, 1) + D(0, 0, -1) - v2) * ss
        dyy = (D(0, 1, 0) + D(0, -1, 0) - v2) * ss
        dss = (D(1, 0, 0) + D(-1, 0, 0) - v2) * ss
        dxy = (D(0, 1, 1) - D(0, 1, -1) - D(0, -1, 1) + D(0, -1, -1)) * cs
        dxs = (D(1, 0, 1) - D(1, 0, -1) - D(-1, 0, 1) + D(-1, 0, -1)) * cs
        dys = (D(1, 1, 0) - D(1, -1, 0) - D(-1, 1, 0) + D(-1, -1, 0)) * cs
        X = solve3([[dxx, dxy, dxs, dx], [dxy, dyy, dys, dy], [dxs, dys, dss, dz]])
        if X is None:
            return 1, moved
        xc, xr, xi = -X[0], -X[1], -X[2]
        if abs(xc) < 0.5 and abs(xr) < 0.5 and abs(xi) < 0.5:
            break
        if not (abs(xc) <= 1e6 and abs(xr) <= 1e6 and abs(xi) <= 1e6):
            return 6, moved
        nc, nr, nl = c + int(np.rint(xc)), r + int(np.rint(xr)), l + int(np.rint(xi))
        moved = moved or (nc, nr, nl) != (c, r, l)
        c, r, l = nc, nr, nl
        if l < 1 or l > S or c < BORDER or c >= W - BORDER or r < BORDER or r >= H - BORDER:
            return 2, moved
    else:
        return 3, moved
    contr = D(0, 0, 0) * IS + (dx * xc + dy * xr + dz * xi) * 0.5
    if abs(contr) * S < contrast:
        return 4, moved
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    if det <= 0.0 or tr * tr * edge >= (edge + 1.0) * (edge + 1.0) * det:
        return 5, moved
    scl = sigma * float(pow2_own((l + xi) / S))
    oscale = math.ldexp(0.5, o)
    size = scl * math.ldexp(1.0, o)
    return 0, (o, l, r, c, xc, xr, xi, contr, size, (c + xc) * oscale, (r + xr) * oscale, scl, moved)


def _gradients(g, rows, cols):
    """dx, dy (float64) of layer g at the cells (rows, cols), all inside the one-cell border."""
    dx = g[rows, cols + 1].astype(np.float64) - g[rows, cols - 1].astype(np.float64)
    dy = g[rows - 1, cols].astype(np.float64) - g[rows + 1, cols].astype(np.float64)
    return dx, dy


def orientations(g, r, c, scl):
    """[(bin j, angle)] of the peaks of the smoothed 36-bin histogram around (r, c) of Gaussian layer g."""
    H, W = g.shape
    rad = int(np.rint(4.5 * scl))
    sig = 1.5 * scl
    escale = -1.0 / (2.0 * sig * sig)
    i, j = np.mgrid[-rad:rad + 1, -rad:rad + 1]
    i, j = i.ravel(), j.ravel()
    y, x = r + i, c + j
    ok = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
    i, j, y, x = i[ok], j[ok], y[ok], x[ok]
    dx, dy = _gradients(g, y, x)
    w = exp_own((i * i + j * j).astype(np.float64) * escale)
    mag = np.sqrt(dx * dx + dy * dy)
    b = np.rint(atan2_own(dy, dx) * (36.0 / 360.0)).astype(np.int64)
    b = np.where(b >= 36, b - 36, b)
    b = np.where(b < 0, b + 36, b)
    q = np.zeros(36, np.int64)
    np.add.at(q, b, np.rint(w * mag * FIX).astype(np.int64))
    t = q.astype(np.float64) / FIX
    h = [(t[k - 2] + t[(k + 2) % 36]) * (1.0 / 16.0) + (t[k - 1] + t[(k + 1) % 36]) * (4.0 / 16.0) + t[k] * (6.0 / 16.0)
         for k in range(36)]
    thr = max(h) * 0.8
    out = []
    for k in range(36):
        a, z = h[k - 1], h[(k + 1) % 36]
        if h[k] > a and h[k] > z and h[k] >= thr:
            b = k + 0.5 * (a - z) / (a - 2.0 * h[k] + z)
            if b < 0.0:
                b = b + 36.0
            if b >= 36.0:
                b = b - 36.0
            angle = 360.0 - 10.0 * b
            if abs(angle - 360.0) < 2.0 ** -23:
                angle = 0.0
            out.append((k, float(angle)))
    return out


def descriptor(g, r, c, scl, angle):
    """(uint8 [128], whether the window was clipped by the layer's edge)."""
    H, W = g.shape
    ori = 360.0 - angle
    if abs(ori - 360.0) < 2.0 ** -23:
        ori = 0.0
    sin_t, cos_t = sincos_own(ori)
    width = 3.0 * scl
    radius = int(np.rint(width * 1.4142135623730951 * 2.5))
    radius = min(radius, int(math.floor(math.sqrt(float(W) * W + float(H) * H))))
    cos_t, sin_t = cos_t / width, sin_t / width
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    i, j = i.ravel(), j.ravel()
    fi, fj = i.astype(np.float64), j.astype(np.float64)
    c_rot = fj * cos_t - fi * sin_t
    r_rot = fj * sin_t + fi * cos_t
    rbin, cbin = r_rot + 1.5, c_rot + 1.5
    y, x = r + i, c + j
    inbin = (rbin > -1.0) & (rbin < 4.0) & (cbin > -1.0) & (cbin < 4.0)
    inside = (y > 0) & (y < H - 1) & (x > 0) & (x < W - 1)
    clipped = bool(np.any(inbin & ~inside))
    ok = inbin & inside
    y, x, rbin, cbin, c_rot, r_rot = y[ok], x[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    dx, dy = _gradients(g, y, x)
    w = exp_own((c_rot * c_rot + r_rot * r_rot) * -0.125)
    mag = np.sqrt(dx * dx + dy * dy) * w
    obin = (atan2_own(dy, dx) - ori) * (8.0 / 360.0)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    o0 = np.where(o0 < 0, o0 + 8, o0)
    o0 = np.where(o0 >= 8, o0 - 8, o0)
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    q = np.zeros(6 * 6 * 10, np.int64)
    base = ((r0 + 1) * 6 + c0 + 1) * 10 + o0
    for v, off in ((v_rc00, 0), (v_rc01, 10), (v_rc10, 60), (v_rc11, 70)):
        v1 = v * obin
        v0 = v - v1
        np.add.at(q, base + off, np.rint(v0 * FIX).astype(np.int64))
        np.add.at(q, base + off + 1, np.rint(v1 * FIX).astype(np.int64))
    q = q.reshape(6, 6, 10)
    q[:, :, 0] += q[:, :, 8]
    q[:, :, 1] += q[:, :, 9]
    dst = q[1:5, 1:5, :8].reshape(128).astype(np.float64) / FIX
    thr = math.sqrt(float(np.cumsum(dst * dst)[-1])) * 0.2
    val = np.minimum(dst, thr)
    nrm = 512.0 / max(math.sqrt(float(np.cumsum(val * val)[-1])), 2.0 ** -23)
    return np.clip(np.rint(val * nrm), 0.0, 255.0).astype(np.uint8), clipped


def pack_octave(o, l, xi):
    return ((o - 1) & 255) | (l << 8) | (int(np.rint((xi + 0.5) * 255.0)) << 16)


# ---- the whole ---------------------------------------------------------------------------------------------------------
def stages(img, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6):
    """Every stage of one detection, as the device's glh_sift_layer shows them, and a trace of which rules fired."""
    S, contrast, edge, sigma = int(nOctaveLayers), float(contrastThreshold), float(edgeThreshold), float(sigma)
    gauss, dog = pyramid(img, S, sigma)
    cand = candidates(dog, S, contrast)
    refined = np.zeros((len(cand), 12))
    trace = {"moved": 0, "two_orientations": 0, "clipped": 0, "octaves": set(), **{name: 0 for name in REJECT.values()}}
    rows = []  # (key, record)
    for n, (o, l, r, c) in enumerate(cand.tolist()):
        status, rec = refine(dog[o], S, contrast, edge, sigma, o, l, r, c)
        refined[n, 0] = status
        if status:
            trace[REJECT[status]] += 1
            continue
        o, l, r, c, xc, xr, xi, contr, size, ptx, pty, scl, moved = rec
        refined[n, 1:] = (o, l, r, c, xc, xr, xi, contr, size, ptx, pty)
        trace["moved"] += bool(moved)
        peaks = orientations(gauss[o][l], r, c, scl)
        trace["two_orientations"] += len(peaks) > 1
        for k, angle in peaks:
            rows.append(((o, l, r, c, k), (ptx, pty, size, angle, abs(contr), float(pack_octave(o, l, xi))), scl))
    rows.sort(key=lambda row: row[0])
    cells = np.array([row[0] for row in rows], np.int32).reshape(-1, 5)
    kps = np.array([row[1] for row in rows], np.float64).reshape(-1, 6)
    desc = np.zeros((len(rows), 128), np.uint8)
    for n, ((o, l, r, c, k), rec, scl) in enumerate(rows):
        desc[n], clipped = descriptor(gauss[o][l], r, c, scl, rec[3])
        trace["clipped"] += clipped
        trace["octaves"].add(o)
    return {"gauss": gauss, "dog": dog, "candidates": cand, "refined": refined, "cells": cells, "keypoints": kps,
            "descriptors": desc, "trace": trace}


def finish(kps, desc, mask=None, nfeatures=0):
    """The host-side steps on the sorted list: duplicates, mask, nfeatures.  ((n, 6), (n, 128))."""
    keep = np.ones(len(kps), bool)
    if len(kps) > 1:
        keep[1:] = np.any(kps[1:, :4] != kps[:-1, :4], axis=1)
    if mask is not None:
        mask = np.asarray(mask, np.uint8)
        v, u = (kps[:, 1] + 0.5).astype(np.int64), (kps[:, 0] + 0.5).astype(np.int64)
        inside = (v >= 0) & (v < mask.shape[0]) & (u >= 0) & (u < mask.shape[1])
        keep &= inside
        keep[inside] &= mask[v[inside], u[inside]] != 0
    kps, desc = kps[keep], desc[keep]
    if nfeatures > 0 and len(kps) > nfeatures:
        order = np.sort(np.argsort(-kps[:, 4], kind="stable")[:nfeatures])
        kps, desc = kps[order], desc[order]
    return kps, desc


def root_descriptors(desc):
    """`root=True`: the reference's expression (optimize.py:2227-2230) on the float32 copy cv2 would have returned."""
    d = np.asarray(desc).astype(np.float32)
    return np.sqrt(d / (d.sum(axis=1, keepdims=True) + 1e-7))


def detect(img, mask=None, nfeatures=0, **params):
    """(keypoints (n, 6) float64: pt x, pt y, size, angle, response, octave; descriptors uint8 (n, 128)), or (None, None)
    when the image holds no octave."""
    if not octave_sizes(*np.shape(img)):
        return None, None
    st = stages(img, **params)
    return finish(st["keypoints"], st["descriptors"], mask, nfeatures)
