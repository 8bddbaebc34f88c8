"""`Camera.project_dem` and `Camera.rasterize` restated in plain NumPy from their description, and the inputs of
tests/golden/g29_project_dem.npz rebuilt from seeds.

The semantics (the reference's, quirks included):
  * the DEM is cut into tiles, row-major; per axis round(cells / size) tiles (none: one tile), cell i in tile
    floor(i / ceil(cells / tiles)), every tile but the first starting `overlap` cells early;
  * a tile carries its own coordinates: the slice of the DEM's when it has three or more cells along the axis, else
    rebuilt from the slice's outer limits;
  * a cell of a tile takes part when its mask is set, its elevation is not NaN, it lies in front of the camera and its uv
    lie in the frame (here 0 <= uv < imgsz: the far edge, where the reference raises, is out);
  * its pixel is (int(v), int(u)); within the tile a pixel is sum * (1 / count) per layer, the float64 sum accumulated in
    row-major cell order (np.bincount); the depth along the optical axis is the last layer when asked for;
  * tiles are written one over the other, in order, without a depth test: a pixel keeps its LAST tile's mean;
  * untouched pixels are NaN.
"""
import numpy as np

from tests import viewshed_terrain as vt


# ---- the restatement -----------------------------------------------------------------------------------------------
def axis_slices(cells, size, overlap):
    """[(start, stop)] of one axis."""
    tiles = int(np.round(cells / size))
    if tiles == 0:
        return [(0, cells)]
    per = int(np.ceil(cells / tiles))
    ends = list(range(per, cells, per)) + [cells]
    starts = [0] + [e - overlap for e in ends[:-1]]
    return list(zip(starts, ends))


def tile_slices(shape, size, overlap=(0, 0)):
    """[(row0, row1, col0, col1)] row-major; `size` and `overlap` are (x, y)."""
    ny, nx = shape
    return [(r0, r1, c0, c1) for r0, r1 in axis_slices(ny, size[1], overlap[1])
            for c0, c1 in axis_slices(nx, size[0], overlap[0])]


def tile_axis(coords, d, start, stop):
    """A tile's coordinates along one axis: `coords` the DEM's, `d` its signed cell size."""
    c = coords[start:stop]
    if len(c) >= 3:
        return c
    lim = (c[0] - 0.5 * d, c[-1] + 0.5 * d)
    return vt.centres(lim, len(c))


def rotation(viewdir):
    a, b, c = np.deg2rad(np.asarray(viewdir, dtype=float))
    ca, cb, cc, sa, sb, sc = np.cos(a), np.cos(b), np.cos(c), np.sin(a), np.sin(b), np.sin(c)
    return np.array([[ca * cc + sa * sb * sc, ca * sb * sc - cc * sa, -cb * sc],
                     [cc * sa * sb - ca * sc, sa * sc + ca * cc * sb, -cb * cc],
                     [cb * sa, ca * cb, sb]])


def camera_project(cam, xyz):
    """(uv, depth) of world points for the 24-vector `cam` (xyz, viewdir, imgsz, f, c, k[6], p[2], correction flag,
    radius, refraction): offset, optional elevation correction, rotation, perspective division (NaN behind the camera),
    radial then tangential distortion, focal length and principal point."""
    rel = np.asarray(xyz, dtype=float) - cam[0:3]
    if cam[20]:
        rel[:, 2] += (cam[22] - 1) * np.sum(rel[:, 0:2] ** 2, axis=1) / (2 * cam[21])
    c = np.matmul(rotation(cam[3:6]), rel.T).T
    with np.errstate(all="ignore"):
        xy = c[:, 0:2] / c[:, 2:3]
        xy[c[:, 2] <= 0] = np.nan
        k, p = cam[12:18], cam[18:20]
        out = xy.copy()
        r2 = np.sum(xy ** 2, axis=1)
        if any(k):
            num = 1
            for i, power in enumerate((r2, r2 * r2, r2 * r2 * r2)):
                if k[i]:
                    num = num + k[i] * power
            if any(k[3:6]):
                den = 1
                for i, power in enumerate((r2, r2 * r2, r2 * r2 * r2)):
                    if k[3 + i]:
                        den = den + k[3 + i] * power
                num = num / den
            out *= np.asarray(num)[..., None] if np.ndim(num) else num
        if any(p):
            cross = xy[:, 0] * xy[:, 1]
            out += np.column_stack((2 * cross * p[0] + p[1] * (r2 + 2 * xy[:, 0] ** 2),
                                    p[0] * (r2 + 2 * xy[:, 1] ** 2) + 2 * cross * p[1]))
        uv = out * cam[8:10] + (cam[6:8] / 2 + cam[10:12])
    return uv, c[:, 2]


def pixel_means(keys, columns, n_pixels):
    """(pixels hit, their means (len, layers)): per pixel the sum in the given order times 1 / count."""
    counts = np.bincount(keys, minlength=n_pixels)
    hit = np.flatnonzero(counts)
    sums = np.column_stack([np.bincount(keys, weights=col, minlength=n_pixels) for col in columns.T])
    return hit, sums[hit] * (1 / counts[hit].reshape(-1, 1))


def project_dem(cam, z, x, y, d, values=None, mask=None, tile_size=(256, 256), tile_overlap=(1, 1), return_depth=False,
                project=camera_project, return_counts=False):
    """float64 (imgsz[1], imgsz[0], layers).  `x`, `y`: the DEM's cell-centre coordinates, `d` its signed cell sizes;
    `project(cam, xyz) -> (uv, depth)`.  `return_counts`: also the number of cells behind every pixel."""
    width, height = int(cam[6]), int(cam[7])
    if values is not None:
        values = np.atleast_3d(values)
    layers = (0 if values is None else values.shape[2]) + int(return_depth)
    out = np.full((height * width, layers), np.nan)
    behind = np.zeros(height * width, dtype=np.int64)
    if mask is None:
        mask = ~np.isnan(z)
    for r0, r1, c0, c1 in tile_slices(z.shape, tile_size, tile_overlap):
        X, Y = np.meshgrid(tile_axis(x, d[0], c0, c1), tile_axis(y, d[1], r0, r1))
        m = np.asarray(mask[r0:r1, c0:c1], dtype=bool)
        if not m.any():
            continue
        uv, depth = project(cam, np.column_stack((X[m], Y[m], z[r0:r1, c0:c1][m].astype(np.float64))))
        with np.errstate(invalid="ignore"):
            inside = (uv[:, 0] >= 0) & (uv[:, 0] < width) & (uv[:, 1] >= 0) & (uv[:, 1] < height)
        if not inside.any():
            continue
        keys = uv[inside, 1].astype(int) * width + uv[inside, 0].astype(int)
        columns = [] if values is None else [values[r0:r1, c0:c1][m][inside].astype(np.float64)]
        if return_depth:
            columns.append(depth[inside, None])
        hit, means = pixel_means(keys, np.column_stack(columns), height * width)
        out[hit] = means
        behind[hit] = np.bincount(keys, minlength=height * width)[hit]
    out = out.reshape(height, width, layers)
    return (out, behind.reshape(height, width)) if return_counts else out


def rasterize(imgsz, uv, values):
    """Camera.rasterize: (ny, nx) for values (n,) or (n, 1), else (ny, nx, d)."""
    nx, ny = int(imgsz[0]), int(imgsz[1])
    uv, values = np.asarray(uv), np.asarray(values)
    with np.errstate(invalid="ignore"):
        inside = (uv[:, 0] >= 0) & (uv[:, 0] < nx) & (uv[:, 1] >= 0) & (uv[:, 1] < ny)
    columns = values[inside].reshape(int(inside.sum()), -1).astype(np.float64)
    out = np.full((ny * nx, columns.shape[1]), np.nan)
    keys = uv[inside, 1].astype(int) * nx + uv[inside, 0].astype(int)
    hit, means = pixel_means(keys, columns, ny * nx)
    out[hit] = means
    return out.reshape(ny, nx) if columns.shape[1] == 1 else out.reshape(ny, nx, -1)


# ---- the inputs of g29, rebuilt from seeds ---------------------------------------------------------------------------
CELL = 10.0


def case_inputs(shape, seed, y="desc", holes=False, mask=False, dem_dtype="float64", values="f64x1"):
    """(z, xlim, ylim, values, mask) of a g29 case.  The DEM is viewshed_terrain's exact surface; the value layers are
    seeded integers scaled by powers of two (exact in their dtype); the explicit mask drops a seeded fifth of the cells."""
    ny, nx = shape
    z = vt.terrain((ny, nx), seed)
    if holes:
        z = vt.holes(z, seed + 1, 0.03, (ny // 3, ny // 3 + 9, nx // 2, nx // 2 + 11))
    if dem_dtype == "float32":
        z = z.astype(np.float32)  # (multiples of 2^-14 below 2^11: exact)
    xlim = (0.0, nx * CELL)
    ylim = (ny * CELL, 0.0) if y == "desc" else (0.0, ny * CELL)
    rng = np.random.default_rng(seed + 29)
    if values == "none":
        v = None
    elif values == "f64x1":
        v = rng.integers(-2 ** 30, 2 ** 30, size=(ny, nx)) / 2.0 ** 12
    elif values == "f64x3":
        v = rng.integers(-2 ** 30, 2 ** 30, size=(ny, nx, 3)) / 2.0 ** 12
    elif values == "f32x2":
        v = (rng.integers(-2 ** 20, 2 ** 20, size=(ny, nx, 2)) / 2.0 ** 8).astype(np.float32)
    elif values == "u8x3":
        v = rng.integers(0, 256, size=(ny, nx, 3)).astype(np.uint8)
    elif values == "u16x1":
        v = rng.integers(0, 65536, size=(ny, nx)).astype(np.uint16)
    elif values == "boolx1":
        v = rng.integers(0, 2, size=(ny, nx)).astype(bool)
    else:
        raise ValueError(values)
    m = (np.random.default_rng(seed + 31).random((ny, nx)) >= 0.2) if mask else None
    return z, xlim, ylim, v, m


def rasterize_inputs(seed, n, imgsz):
    """(uv, values (n, 2)): seeded points over and around the frame, a third of them repeated exactly."""
    rng = np.random.default_rng(seed)
    uv = rng.integers(-8 * 1024, (np.array(imgsz) + 8) * 1024, size=(n, 2)) / 1024.0 + 1 / 2048.0
    uv[n // 3: 2 * (n // 3)] = uv[: n // 3]
    values = rng.integers(-2 ** 30, 2 ** 30, size=(n, 2)) / 2.0 ** 12
    return uv, values


def g29_case(g, name):
    """A case of g29 (`g`: the loaded file) as a dict: z, xlim, ylim, values, mask, cam (24-vector), tile_size,
    tile_overlap, return_depth, image (the reference's), counts, margins -- the DEM checked against its SHA-256."""
    y_asc, holes, mask, dem32, depth = (bool(v) for v in g[f"{name}__flags"])
    z, xlim, ylim, values, m = case_inputs((96, 128), int(g[f"{name}__seed"]), y="asc" if y_asc else "desc", holes=holes,
                                           mask=mask, dem_dtype="float32" if dem32 else "float64",
                                           values=str(g[f"{name}__values"]))
    assert np.array_equal(vt.sha256(z), g[f"{name}__sha256"]), name
    t = [int(v) for v in g[f"{name}__tiling"]]
    return dict(z=z, xlim=xlim, ylim=ylim, values=values, mask=m, cam=g[f"{name}__cam"], tile_size=(t[0], t[1]),
                tile_overlap=(t[2], t[3]), return_depth=depth, image=g[f"{name}__image"], counts=g[f"{name}__counts"],
                margins=g[f"{name}__margins"])
