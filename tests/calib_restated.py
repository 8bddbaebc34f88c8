"""optimize.Lines.predicted (optimize.py:355-376 with :320-353) restated in NumPy, operation by operation, and a
reference-equivalent fit driven by it: what tests/test_calib_host.py compares with the reference's outputs and
tests/test_gpu_calib.py with the device's, bit for bit.

A camera is its vector (oracle.camera's 24, or the first 20) and its rotation matrix R, passed in: the device tests pass
the package's own (`Camera.R`), the host tests oracle.camera's.  The polylines are split and clipped by the package's
restated helpers (glimpse_amd.helpers, themselves pinned against the reference in test_calib_host.py); everything from the
clipped vertices on is elementwise arithmetic written out here:

  np.linspace(start, stop, n)   arange(n) * step + start with step = (stop - start) / (n - 1), the last value set to stop
                                (n == 1: [start]; a zero step: arange / (n - 1) * (stop - start))
  np.interp(t, x, f)            j = searchsorted(x, t, "right") - 1;  slope * (t - x[j]) + f[j] with
                                slope = (f[j + 1] - f[j]) / (x[j + 1] - x[j]);  f[j] where t == x[j] or j is the last
  Camera._distort, _xy_to_uv    the host method's order (camera.py:1180-1196, :1499-1508)
  cdist(..., "sqeuclidean")     dx * dx + dy * dy;  np.argmin: the first of equal minima, 0 if none is below +inf
"""
import numpy as np

from glimpse_amd import helpers

TILE = 256  # projected points the nearest kernel holds in LDS at a time (glh_calib.h: CAL_TILE)


def xyz_to_xy(cam, R, xyz, directions=False):
    """Camera._xyz_to_xy (camera.py:1435-1470) term by term, without an elevation correction."""
    xyz = np.atleast_2d(np.asarray(xyz, dtype=float))
    d = xyz if directions else xyz - cam[0:3]
    c = [R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1] + R[r, 2] * d[:, 2] for r in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        xy = np.column_stack((c[0] / c[2], c[1] / c[2]))
    xy[c[2] <= 0] = np.nan
    return xy


def linspace(start, stop, n):
    if n == 0:
        return np.empty(0)
    i = np.arange(n, dtype=float)
    delta = stop - start
    if n == 1:
        return i * delta + start
    step = delta / (n - 1)
    t = (i * step if step != 0 else i / (n - 1) * delta) + start
    t[-1] = stop
    return t


def interp(t, x, f):
    if len(x) == 1:
        return np.full(len(t), f[0])
    j = np.searchsorted(x, t, side="right") - 1
    left, last = j < 0, j >= len(x) - 1
    jj = np.clip(j, 0, len(x) - 2)
    slope = (f[jj + 1] - f[jj]) / (x[jj + 1] - x[jj])
    out = slope * (t - x[jj]) + f[jj]
    out = np.where(t == x[jj], f[jj], out)
    out = np.where(last, f[-1], out)
    return np.where(left, f[0], out)


def distort(cam, xy):
    k, p = cam[12:18], cam[18:20]
    if not (k.any() or p.any()):
        return xy
    x, y = xy[:, 0], xy[:, 1]
    r2 = x * x + y * y
    qx, qy = x, y
    if k.any():
        def series(kk):
            total = np.ones(len(r2))
            if kk[0]:
                total = total + kk[0] * r2
            if kk[1]:
                total = total + kk[1] * r2 * r2
            if kk[2]:
                total = total + kk[2] * r2 * r2 * r2
            return total

        dr = series(k[0:3])
        if k[3:6].any():
            dr = dr / series(k[3:6])
        qx, qy = x * dr, y * dr
    if p.any():
        xty = x * y
        qx = qx + (2 * xty * p[0] + p[1] * (r2 + 2 * (x * x)))
        qy = qy + (p[0] * (r2 + 2 * (y * y)) + 2 * xty * p[1])
    return np.column_stack((qx, qy))


def xy_to_uv(cam, xy):
    return distort(cam, xy) * cam[8:10] + (cam[6:8] / 2 + cam[10:12])


def segments(cam, R, xyzs, xy_box, directions=False, density=1):
    """[(vertices (m, 2), distances (m,), count)] of Lines._xyzs_to_uvs, counts of 0 included; with no line in frame,
    the lines in front of the camera with count None (their vertices are the points)."""
    xy_step = (1 / density) / cam[8:10].max()
    out, inlines = [], []
    for xyz in xyzs:
        xy = xyz_to_xy(cam, R, xyz, directions)
        for line in helpers.boolean_split(xy, np.isnan(xy[:, 0]), include="false"):
            inlines.append(line)
            for cline in helpers.clip_polyline_box(line, xy_box):
                cline = np.array(cline)
                d = np.sqrt(np.sum(np.diff(cline, axis=0) ** 2, axis=1))
                x = np.concatenate(([0.0], np.cumsum(d)))
                n = abs((x[-1] - x[0]) / xy_step)
                if n == int(n):
                    n += 1
                out.append((cline, x, int(round(n))))
    if out:
        return out
    return [(line, None, None) for line in inlines]


def projected(cam, R, xyzs, xy_box, directions=False, density=1):
    """The image coordinates of every segment's points, one array per segment."""
    puvs = []
    for vertices, x, n in segments(cam, R, xyzs, xy_box, directions, density):
        if n is None:
            puvs.append(xy_to_uv(cam, vertices))
            continue
        t = linspace(x[0], x[-1], n)
        puvs.append(xy_to_uv(cam, np.column_stack((interp(t, x, vertices[:, 0]), interp(t, x, vertices[:, 1])))))
    return puvs


def nearest(observed, puv):
    """(indices, relative gap between the nearest and the second-nearest squared distance, smallest over the points)."""
    dx = observed[:, None, 0] - puv[None, :, 0]
    dy = observed[:, None, 1] - puv[None, :, 1]
    d = dx * dx + dy * dy
    index = np.argmin(d, axis=1)
    gap = np.inf
    if puv.shape[0] > 1 and len(observed):
        two = np.sort(d, axis=1)[:, :2]
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = np.nanmin(np.append((two[:, 1] - two[:, 0]) / two[:, 1], np.inf))
    return index, gap


def lines_predicted(cam, R, observed, xyzs, xy_box, directions=False, density=1, info=None):
    puv = np.vstack(projected(cam, R, xyzs, xy_box, directions, density))
    index, gap = nearest(np.asarray(observed, dtype=float), puv)
    if info is not None:
        info["gap"], info["n_projected"] = gap, len(puv)
    return puv[index]


# ---- a fit as the reference's, on the CPU: oracle.camera for the projection of points, the restatement for lines ---------
def clip_box(cam):
    """Lines._xyzs_to_uvs' box (optimize.py:328-330) with oracle.camera's inverse distortion."""
    from oracle import camera as oc

    w, h = cam[6], cam[7]
    u, v = np.linspace(0, w, 3), np.linspace(0, h, 3)
    edges = np.array([(a, b) for a in u for b in v if a in (0, w) or b in (0, h)])
    xy = oc.undistort(cam, (edges - (cam[6:8] / 2 + cam[10:12])) * (1 / cam[8:10]))
    return np.hstack((xy.min(axis=0), xy.max(axis=0)))


class HostModel:
    """Points and Lines controls of cameras that share `f` and fit their `viewdir`: parameters [f0, f1, viewdir of
    camera 0, 1, ...], the layout of Cameras(cam_params=[{"viewdir": True}] * n, group_params={"f": True})."""

    def __init__(self, vectors, controls):
        self.vectors = [np.array(v, dtype=float) for v in vectors]  # (24,) each
        self.controls = controls  # [("points", cam, uv, xyz) | ("lines", cam, uv, [xyz, ...])]

    def cameras(self, x):
        out = []
        for i, v in enumerate(self.vectors):
            v = v.copy()
            v[8:10] = x[0:2]
            v[3:6] = x[2 + 3 * i:5 + 3 * i]
            out.append(v)
        return out

    def residuals(self, x):
        from oracle import camera as oc

        cams = self.cameras(x)
        rows = []
        for kind, i, uv, world in self.controls:
            if kind == "points":
                rows.append(oc.xyz_to_uv(cams[i], world) - uv)
            else:
                rows.append(lines_predicted(cams[i], oc.rotation_matrix(cams[i][3:6]), uv, world, clip_box(cams[i])) - uv)
        return np.vstack(rows).ravel()
