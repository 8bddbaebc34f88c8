"""The rule of `Image.orthorectify` (INPUTS.md, "Orthorectification: the rule") restated on the host: NumPy and
`scipy.interpolate.RegularGridInterpolator` only, none of the library's code.  For every cell (r, c) of the DEM:

1. xyz = (X[r, c], Y[r, c], z[r, c]), the cell's centre;
2. uv = Camera.xyz_to_uv(xyz): the elevation correction, the rotation, NaN behind the camera, the distortion;
3. the cell is seen when z[r, c] is not NaN, Camera.inframe(uv), mask[r, c] and viewshed[r, c] (where given);
4. a seen cell's value is RegularGridInterpolator((pv, pu), frame[:, :, ch], method, bounds_error=False)(uv[::-1]);
5. every other cell is NaN.

The camera is anything with the attributes of `glimpse_amd.Camera` (xyz, viewdir, imgsz, f, c, k, p, correction); only
those plain arrays are read.
"""
import numpy as np
import scipy.interpolate


def rotation(viewdir):
    """Camera.R."""
    radians = np.deg2rad(np.asarray(viewdir, dtype=float))
    C, S = np.cos(radians), np.sin(radians)
    return np.array([
        [C[0] * C[2] + S[0] * S[1] * S[2], C[0] * S[1] * S[2] - C[2] * S[0], -C[1] * S[2]],
        [C[2] * S[0] * S[1] - C[0] * S[2], S[0] * S[2] + C[0] * C[2] * S[1], -C[1] * C[2]],
        [C[1] * S[0], C[0] * C[1], S[1]],
    ])


def xyz_to_uv(cam, xyz):
    """Camera.xyz_to_uv: _xyz_to_xy, _distort, _xy_to_uv, expression by expression."""
    dxyz = np.asarray(xyz, dtype=float) - np.asarray(cam.xyz, dtype=float)
    if isinstance(cam.correction, dict):  # helpers.elevation_corrections
        sq = np.sum(dxyz[:, 0:2] ** 2, axis=1)
        dxyz[:, 2] += (cam.correction["refraction"] - 1) * sq / (2 * cam.correction["radius"])
    xyz_c = np.matmul(rotation(cam.viewdir), dxyz.T).T
    with np.errstate(invalid="ignore", divide="ignore"):
        xy = xyz_c[:, 0:2] / xyz_c[:, 2:3]
    xy[xyz_c[:, 2] <= 0] = np.nan
    k, p = np.asarray(cam.k, dtype=float), np.asarray(cam.p, dtype=float)
    dxy = xy.copy()
    r2 = np.sum(xy ** 2, axis=1)
    if k.any():
        dr = 1
        for i in range(3):
            if k[i]:
                dr = dr + _power(k[i] * r2, r2, i)
        if k[3:6].any():
            temp = 1
            for i in range(3):
                if k[3 + i]:
                    temp = temp + _power(k[3 + i] * r2, r2, i)
            dr = dr / temp
        dxy *= dr[:, None]
    if p.any():
        xty = xy[:, 0] * xy[:, 1]
        dtx = 2 * xty * p[0] + p[1] * (r2 + 2 * xy[:, 0] ** 2)
        dty = p[0] * (r2 + 2 * xy[:, 1] ** 2) + 2 * xty * p[1]
        dxy += np.column_stack((dtx, dty))
    imgsz = np.asarray(cam.imgsz, dtype=float)
    return dxy * np.asarray(cam.f, dtype=float) + (imgsz / 2 + np.asarray(cam.c, dtype=float))


def _power(term, r2, times):
    """k * r2 * r2 * ... left to right, as the reference writes its radial series."""
    for _ in range(times):
        term = term * r2
    return term


def inframe(cam, uv):
    """Camera.inframe."""
    with np.errstate(invalid="ignore"):
        return np.all((uv >= 0) & (uv <= np.asarray(cam.imgsz)), axis=1)


def orthorectify(cam, frame, x, y, z, mask=None, viewshed=None, method="linear"):
    """(result (ny, nx, channels), uv (ny, nx, 2), seen (ny, nx)) of the rule for the frame (h, w) or (h, w, channels)
    seen by `cam` over the DEM `z` (ny, nx) with the cell centres `x` (nx,) and `y` (ny,).  float32 for float32 frames
    (what the interpolator returns, assigned into float32: one rounding, as Image.project's result array does), float64
    for every other."""
    frame = np.asarray(frame)
    frame = frame[:, :, None] if frame.ndim < 3 else frame
    z = np.asarray(z)
    ny, nx = z.shape
    X, Y = np.meshgrid(np.asarray(x, dtype=float), np.asarray(y, dtype=float))
    uv = xyz_to_uv(cam, np.column_stack((X.ravel(), Y.ravel(), z.ravel().astype(float))))
    seen = ~np.isnan(z.ravel().astype(float)) & inframe(cam, uv)
    if mask is not None:
        seen &= np.asarray(mask, dtype=bool).ravel()
    if viewshed is not None:
        seen &= np.asarray(viewshed, dtype=bool).ravel()
    h, w, channels = frame.shape
    pu, pv = np.linspace(0.5, w - 0.5, w), np.linspace(0.5, h - 0.5, h)
    out = np.full((ny * nx, channels), np.nan, dtype=np.float32 if frame.dtype == np.float32 else np.float64)
    if seen.any():
        for ch in range(channels):
            f = scipy.interpolate.RegularGridInterpolator((pv, pu), frame[:, :, ch], method=method, bounds_error=False)
            out[seen, ch] = f(uv[seen][:, ::-1])
    return out.reshape(ny, nx, channels), uv.reshape(ny, nx, 2), seen.reshape(ny, nx)


def fragile_cells(uv, seen, size, method, eps=1e-9):
    """How many seen cells have a restated uv within `eps` px of where the answer changes kind: a frame edge (inframe), a
    pixel-centre line (the interpolator's interval, and its domain's ends), and for "nearest" a pixel boundary (the
    pick).  A scene for an exact comparison of NaN patterns and nearest picks has none."""
    uv = uv[seen]
    w, h = size
    count = 0
    for a, n in ((uv[:, 0], w), (uv[:, 1], h)):
        near = (np.abs(a) < eps) | (np.abs(a - n) < eps) | (np.abs((a - 0.5) - np.round(a - 0.5)) < eps)
        if method == "nearest":
            near |= np.abs(a - np.round(a)) < eps
        count += int(near.sum())
    return count
