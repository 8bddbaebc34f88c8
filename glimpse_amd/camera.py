"""`Camera`: host-side mirror of `glimpse.Camera` for the tracking path.

Same constructor and attributes as the reference (/root/reference/src/glimpse/camera.py:77-123,
state vector `_vector[20]` :101, :128-198).  `xyz_to_uv` (camera.py:591-628) -- the projection
half that sits on the Tracker hot path -- runs on the GPU through libglimpse_hip.so; there is no
CPU fallback for it.  The inverse projection (`uv_to_xyz`, camera.py:630-663, with the k1 closed form
and the Oulu undistortion, :1198-1337) runs on the GPU as well (`glh_stage_unproject`); it is not on
the per-frame path.  Of the rendering methods, `project_dem` (camera.py:967-1129: the image and the depth map a
camera records of a DEM) and `rasterize` (:858-883: points to a mean image) are served, on the GPU
(`glh_stage_project_dem`, `glh_stage_rasterize`); `project_dem` without the per-tile rescaling (`scale_limits` other than
(1, 1), which fails in the reference itself).  `uv_to_dem` and `xyz_map` go the other way, from pixels to the terrain
they see (`glh_stage_raycast`: the reference has the parts and leaves the ray cast to its users).  `Rprime` and the camera-coordinate halves of the projection (`_uv_to_xy`
on the GPU, `_xy_to_uv`, `_xy_to_xyz`, `_xyz_to_xy` on the host) and `edges` serve `glimpse_amd.optimize`.
"""
import numpy as np

from . import _lib, synth


def _fmt(value, length, default=None, dtype=float):
    """helpers.format_list (helpers.py:27-84) for the cases the Camera constructor uses."""
    if value is None:
        return None
    v = np.atleast_1d(np.asarray(value, dtype=dtype)).ravel()
    if len(v) == length:
        return v
    if len(v) == 1 and default is None:
        return np.repeat(v, length)
    if len(v) < length:
        fill = v[-1] if default is None else default
        return np.concatenate((v, np.full(length - len(v), fill, dtype=dtype)))
    return v[:length]


def rotations(viewdirs):
    """`Camera.R` (n, 3, 3) and `Camera.Rprime` (n, 3, 3, 3) of the view directions `viewdirs` (n, 3) at once, every entry
    by the expression of camera.py:263-280 and :290-329 in its order, so that they equal the properties bit for bit
    (optimize.ObserverCameras evaluates all images' per callback)."""
    rad = np.deg2rad(np.asarray(viewdirs, dtype=float).reshape(-1, 3))
    C, S = np.cos(rad).T, np.sin(rad).T
    zero = np.zeros(rad.shape[0])
    R = np.array([
        [C[0] * C[2] + S[0] * S[1] * S[2], C[0] * S[1] * S[2] - C[2] * S[0], -C[1] * S[2]],
        [C[2] * S[0] * S[1] - C[0] * S[2], S[0] * S[2] + C[0] * C[2] * S[1], -C[1] * C[2]],
        [C[1] * S[0], C[0] * C[1], S[1]],
    ])
    # [w][r][k] as the reference writes it down, stacked along axis 1 into [r][w][k]
    Rprime = np.array([
        [
            [C[0] * S[1] * S[2] - S[0] * C[2], S[0] * S[2] + C[0] * S[1] * C[2], C[0] * C[1]],
            [-S[0] * S[1] * S[2] - C[0] * C[2], C[0] * S[2] - S[0] * S[1] * C[2], -S[0] * C[1]],
            [zero, zero, zero],
        ],
        [
            [S[0] * C[1] * S[2], S[0] * C[1] * C[2], -S[0] * S[1]],
            [C[0] * C[1] * S[2], C[0] * C[1] * C[2], -C[0] * S[1]],
            [S[1] * S[2], S[1] * C[2], C[1]],
        ],
        [
            [S[0] * S[1] * C[2] - C[0] * S[2], -S[0] * S[1] * S[2] - C[0] * C[2], zero],
            [S[0] * S[2] + C[0] * S[1] * C[2], S[0] * C[2] - C[0] * S[1] * S[2], zero],
            [-C[1] * C[2], C[1] * S[2], zero],
        ],
    ])
    return np.ascontiguousarray(R.transpose(2, 0, 1)), np.ascontiguousarray(Rprime.transpose(3, 1, 0, 2)) * (np.pi / 180)


class Camera:
    def __init__(self, imgsz, f=None, c=None, sensorsz=None, fmm=None, cmm=None, k=(0, 0, 0, 0, 0, 0),
                 p=(0, 0), xyz=(0, 0, 0), viewdir=(0, 0, 0), correction=False):
        if (fmm is not None or cmm is not None) and sensorsz is None:
            raise ValueError("Attributes in mm (fmm, cmm) provided without sensor size")
        if f is not None and fmm is not None:
            raise ValueError("Focal length provided in both pixels and mm (f, fmm)")
        if c is not None and cmm is not None:
            raise ValueError("Principal point offset provided in both pixels and mm (c, cmm)")
        if imgsz is None:
            raise ValueError("Image size (imgsz) cannot be None")
        self._vector = np.full(20, np.nan, dtype=float)
        self.xyz = xyz
        self.viewdir = viewdir
        self.imgsz = imgsz
        self.sensorsz = sensorsz
        if fmm is not None:
            f = _fmt(fmm, 2) * self.imgsz / self.sensorsz
        if f is None:
            raise ValueError("Focal length (f or fmm) is missing")
        self.f = f
        if cmm is not None:
            c = _fmt(cmm, 2) * self.imgsz / self.sensorsz
        if c is None:
            c = (0, 0)
        self.c = c
        self.k = k
        self.p = p
        if correction is True:
            correction = {}
        if isinstance(correction, dict):
            correction = {"radius": 6.3781e6, "refraction": 0.13, **correction}
        self.correction = correction
        self._original_vector = self._vector.copy()

    # ---- properties (camera.py:128-236)
    xyz = property(lambda s: s._vector[0:3], lambda s, v: s._vector.__setitem__(slice(0, 3), _fmt(v, 3, 0)))
    viewdir = property(lambda s: s._vector[3:6], lambda s, v: s._vector.__setitem__(slice(3, 6), _fmt(v, 3, 0)))
    f = property(lambda s: s._vector[8:10], lambda s, v: s._vector.__setitem__(slice(8, 10), _fmt(v, 2)))
    c = property(lambda s: s._vector[10:12], lambda s, v: s._vector.__setitem__(slice(10, 12), _fmt(v, 2, 0)))
    k = property(lambda s: s._vector[12:18], lambda s, v: s._vector.__setitem__(slice(12, 18), _fmt(v, 6, 0)))
    p = property(lambda s: s._vector[18:20], lambda s, v: s._vector.__setitem__(slice(18, 20), _fmt(v, 2, 0)))

    @property
    def imgsz(self):
        return self._vector[6:8].astype(int)

    @imgsz.setter
    def imgsz(self, value):
        as_float = _fmt(value, 2)
        as_int = as_float.astype(int)
        if np.any(as_int != as_float):
            raise ValueError("Image size is not integer")
        self._vector[6:8] = as_int

    @property
    def sensorsz(self):
        return self._sensorsz

    @sensorsz.setter
    def sensorsz(self, value):
        self._sensorsz = None if value is None else np.array(_fmt(value, 2), dtype=float)

    @property
    def fmm(self):
        return None if self.sensorsz is None else self.f * self.sensorsz / self.imgsz

    @property
    def cmm(self):
        return None if self.sensorsz is None else self.c * self.sensorsz / self.imgsz

    @property
    def R(self):
        """camera.py:239-280."""
        return synth.rotation_matrix(self.viewdir)

    @property
    def Rprime(self):
        """camera.py:283-329: the derivative of `R` with respect to `viewdir`, (3, 3, 3) as [r][w][k]."""
        return rotations(self.viewdir)[1][0]

    @property
    def vector24(self):
        """The 24-double layout of include/glimpse_hip.h (GLH_CAM_LEN)."""
        v = np.zeros(_lib.CAM_LEN)
        v[:20] = self._vector
        if isinstance(self.correction, dict):
            v[20], v[21], v[22] = 1.0, self.correction["radius"], self.correction["refraction"]
        return v

    def copy(self):
        cam = Camera(imgsz=self.imgsz, f=self.f, c=self.c, sensorsz=self.sensorsz, k=self.k, p=self.p,
                     xyz=self.xyz, viewdir=self.viewdir,
                     correction=dict(self.correction) if isinstance(self.correction, dict) else self.correction)
        return cam

    # ---- the formats either side of the path: camera models live in JSON files (camera.py:334-509) --------------------
    _FIELDS = ("xyz", "viewdir", "imgsz", "f", "c", "k", "p", "correction")

    @classmethod
    def from_json(cls, path, **kwargs):
        """camera.py:334-357: the constructor arguments stored by `to_json`; entries that are null (all NaN once read as
        numbers) count as absent; `kwargs` override the file."""
        import json

        with open(path) as fp:
            stored = json.load(fp)
        args = {}
        for key, value in stored.items():
            if isinstance(value, dict) or isinstance(value, bool):  # (correction: a dict of constants, or a flag)
                args[key] = value
                continue
            numbers = np.array(value, dtype=float)
            args[key] = None if np.isnan(numbers).all() else numbers
        args.update(kwargs)
        return cls(**args)

    def to_array(self):
        """camera.py:412-429: xyz | viewdir | imgsz | f | c | k | p as one vector of 20."""
        return self._vector.copy()

    def to_dict(self, attributes=_FIELDS):
        """camera.py:431-460: attribute name -> plain Python lists / numbers."""
        return {key: getattr(getattr(self, key), "tolist", lambda key=key: getattr(self, key))() for key in attributes}

    def to_json(self, path=None, attributes=_FIELDS, **kwargs):
        """camera.py:462-509: the dictionary of `to_dict` as JSON text, returned or written to `path`."""
        import json

        text = json.dumps(self.to_dict(attributes=attributes), **kwargs)
        if path is None:
            return text
        with open(path, "w") as fp:
            fp.write(text)
        return None

    def reset(self):
        """camera.py:399-410: back to the state the camera was constructed (or copied) with."""
        self._vector = self._original_vector.copy()

    def idealize(self):
        """camera.py:511-530: no distortion, no principal point offset."""
        self.k, self.p, self.c = np.zeros(6), np.zeros(2), np.zeros(2)

    def resize(self, size=1, force=False):
        """camera.py:532-589: scale imgsz, f and c to a target image size (nx, ny) or by a factor of the ORIGINAL size.
        A target size must be reachable by one factor for both axes (round(factor * original) == target) unless
        `force`."""
        target = np.atleast_1d(np.asarray(size, dtype=float))
        original = self._original_vector[6:8]
        if len(target) > 1 and force:
            new_size = target
        else:
            if len(target) > 1:
                # the factors s with round(s * original) == target on an axis form an interval; one factor must serve both
                lo, hi = np.max((target - 0.5) / original), np.min((target + 0.5) / original)
                exact = target / original
                if np.all(exact == exact[0]):
                    scale = exact[0]
                elif lo < hi:
                    scale = 0.5 * (lo + hi)
                else:
                    raise ValueError("Target image size does not preserve the original aspect ratio")
            else:
                scale = target[0]
            new_size = np.floor(scale * original + 0.5)
        ratio = new_size / self.imgsz
        self.imgsz = np.round(new_size)
        self.f = self.f * ratio
        self.c = self.c * ratio

    def infront(self, xyz, directions=False):
        """camera.py:665-683: which points (or ray directions) lie in front of the camera, i.e. project at all."""
        xyz = np.atleast_2d(np.asarray(xyz, dtype=float))
        rel = xyz if directions else xyz - self.xyz
        return (rel @ self.R.T)[:, 2] > 0

    # ---- projection (hot path: GPU)
    def xyz_to_uv(self, xyz, directions=False, return_depth=False):
        """camera.py:591-628, evaluated by the projection kernel (`directions=True`: xyz are rays, :1448)."""
        xyz = np.atleast_2d(np.asarray(xyz, dtype=float))
        if return_depth:  # (uv, distance along the optical axis), camera.py:1468-1469
            return _lib.stage_project_depth(self.vector24, xyz, directions=directions)
        return _lib.stage_project(self.vector24, xyz, directions=directions)

    def inframe(self, uv):
        """camera.py:700-718."""
        uv = np.asarray(uv)
        with np.errstate(invalid="ignore"):
            return np.all((uv >= 0) & (uv <= self.imgsz), axis=1)

    def edges(self, step=1):
        """camera.py:763-800: image coordinates along the image edges, clockwise from (0, 0), `step` apart (one number
        or one per axis)."""
        if isinstance(step, (int, float)):
            step = (step, step)
        u = np.linspace(0, self.imgsz[0], int(self.imgsz[0] / step[0] + 1))
        v = np.linspace(0, self.imgsz[1], int(self.imgsz[1] / step[1] + 1))
        return np.vstack((
            np.column_stack((u, np.repeat(0, len(u)))),
            np.column_stack((np.repeat(u[-1], len(v) - 2), v[1:-1])),
            np.column_stack((u[::-1], np.repeat(v[-1], len(u)))),
            np.column_stack((np.repeat(0, len(v) - 2), v[::-1][1:-1])),
        ))

    def uv_to_xyz(self, uv, directions=True, depth=1):
        """camera.py:630-663 on the device (`glh_stage_unproject`): closed form for k1 alone, else the Oulu
        fixed point, 20 iterations (camera.py:1198-1337)."""
        uv = np.atleast_2d(np.asarray(uv, dtype=float))
        d = None if (isinstance(depth, (int, float)) and depth == 1) else depth
        return _lib.stage_unproject(self.vector24, uv, depth=d, directions=directions)

    # ---- pixels to terrain (GPU): the reference leaves the ray cast to its users
    def uv_to_dem(self, uv, dem, return_depth=False, return_status=False, block=16):
        """The world points the image coordinates `uv` (n, 2) see on `dem` (a Raster with a 2-D array of elevations):
        xyz (n, 3), NaN where a pixel's ray meets no terrain.  The ray of a pixel is `xyz + t uv_to_xyz(uv,
        directions=True)`, unprojected on the device, so t -- returned beside xyz with `return_depth` -- is the depth
        along the optical axis, the unit of `xyz_to_uv(return_depth=True)` and `project_dem(return_depth=True)`.  The
        surface, the traversal and the hit are `Raster.intersect_rays`' (INPUTS.md, "Ray casting: the rule"); the
        elevation correction is this camera's own.  Without one, `xyz_to_uv` of a hit returns its pixel.  With one, xyz
        is the point of the ray, on the apparent surface: the terrain under it differs by
        helpers.elevation_corrections of its squared horizontal distance, and it is that terrain point `xyz_to_uv`
        projects back to the pixel.  `return_status`: also, per ray, an index into `_lib.RAYCAST_STATUS`.  One thread per
        ray on the GPU (`glh_stage_raycast`)."""
        uv = np.atleast_2d(np.asarray(uv, dtype=float))
        if uv.ndim != 2 or uv.shape[1] != 2:
            raise ValueError(f"uv must be (n, 2), got {uv.shape}")
        if len(uv) == 0:
            t, xyz, status = np.empty(0), np.empty((0, 3)), np.empty(0, dtype=np.uint8)
        else:
            t, xyz, _, status = dem._cast_rays(self.correction, block, cam=self.vector24, uv=uv)
        result = (xyz,) + ((t,) if return_depth else ()) + ((status,) if return_status else ())
        return result[0] if len(result) == 1 else result

    def xyz_map(self, dem, step=1, return_depth=False, block=16):
        """The world point every pixel sees on `dem`: (rows, cols, 3) for the pixel centres (step / 2 + c step,
        step / 2 + r step), c < imgsz[0] // step, r < imgsz[1] // step, NaN where a pixel sees no terrain; with
        `return_depth` also the depth map (rows, cols) along the optical axis.  `uv_to_dem` of those pixel centres, which
        are made on the device: nothing but the DEM is uploaded, and a wave takes an 8 x 8 block of pixels, whose rays
        cross neighbouring patches."""
        if isinstance(step, bool) or int(step) != step or step < 1:
            raise ValueError(f"step must be a positive integer, got {step}")
        step = int(step)
        cols, rows = (int(v) // step for v in self.imgsz)
        if cols < 1 or rows < 1:
            raise ValueError(f"step {step} leaves no pixel of an image of {tuple(int(v) for v in self.imgsz)}")
        if cols * rows >= 2 ** 31:
            raise NotImplementedError(f"{cols} x {rows} pixels: fewer than 2^31 rays are served")
        t, xyz, _, _ = dem._cast_rays(self.correction, block, cam=self.vector24, step=step)
        xyz = xyz.reshape(rows, cols, 3)
        return (xyz, t.reshape(rows, cols)) if return_depth else xyz

    # ---- the halves of the projection either side of the camera coordinates (camera.py:1138-1196, :1435-1519)
    def _distort(self, xy):
        """camera.py:1180-1196 with :1138-1178 on the host (a companion of the classes in `optimize`; `xyz_to_uv`'s own
        distortion is the projection kernel's)."""
        xy = np.asarray(xy, dtype=float)
        if not (self.k.any() or self.p.any()):
            return xy
        r2 = np.sum(xy ** 2, axis=1)
        dxy = xy.copy()
        if self.k.any():
            def series(k):  # 1 + k[0] r2 + k[1] r2 r2 + k[2] r2 r2 r2 over the terms whose k is set, left to right
                total = np.ones(len(r2))
                for i in range(3):
                    if k[i]:
                        term = k[i] * r2
                        for _ in range(i):
                            term = term * r2
                        total = total + term
                return total

            dr = series(self.k[0:3])
            if self.k[3:6].any():
                dr = dr / series(self.k[3:6])
            dxy = dxy * np.reshape(dr, (-1, 1))
        if self.p.any():
            xty = xy[:, 0] * xy[:, 1]
            dtx = 2 * xty * self.p[0] + self.p[1] * (r2 + 2 * xy[:, 0] ** 2)
            dty = self.p[0] * (r2 + 2 * xy[:, 1] ** 2) + 2 * xty * self.p[1]
            dxy = dxy + np.column_stack((dtx, dty))
        return dxy

    def _xyz_to_xy(self, xyz, directions=False, return_depth=False):
        """camera.py:1435-1470 on the host, without the elevation correction (`optimize` passes ray directions)."""
        xyz = np.atleast_2d(np.asarray(xyz, dtype=float))
        if not directions and isinstance(self.correction, dict):
            raise NotImplementedError("_xyz_to_xy with an elevation correction: use xyz_to_uv")
        R = self.R
        d = xyz if directions else xyz - self.xyz
        xyz_c = np.column_stack([R[r, 0] * d[:, 0] + R[r, 1] * d[:, 1] + R[r, 2] * d[:, 2] for r in range(3)])
        with np.errstate(invalid="ignore", divide="ignore"):
            xy = xyz_c[:, 0:2] / xyz_c[:, 2:3]
        xy[xyz_c[:, 2] <= 0] = np.nan
        return (xy, xyz_c[:, 2]) if return_depth else xy

    def _xy_to_xyz(self, xy, directions=True, depth=1):
        """camera.py:1472-1497 on the host: R.T[:, 0:2] @ xy + R.T[:, 2], term by term."""
        xy = np.atleast_2d(np.asarray(xy, dtype=float))
        R = self.R
        xyz = np.column_stack([(R[0, k] * xy[:, 0] + R[1, k] * xy[:, 1]) + R[2, k] for k in range(3)])
        if not isinstance(depth, (int, float)) or depth != 1:
            xyz *= np.atleast_1d(depth).reshape(-1, 1)
        if not directions:
            xyz += self.xyz
        return xyz

    def _xy_to_uv(self, xy):
        """camera.py:1499-1508 on the host."""
        return self._distort(xy) * self.f + (self.imgsz / 2 + self.c)

    def _uv_to_xy(self, uv):
        """camera.py:1510-1519 on the device (`glh_stage_uv_to_xy`): `uv_to_xyz` stopped before the rotation -- the
        closed form for k1 alone, else the Oulu fixed point, 20 iterations."""
        return _lib.stage_uv_to_xy(self.vector24, np.atleast_2d(np.asarray(uv, dtype=float)))

    # ---- rendering (GPU)
    def rasterize(self, uv, values):
        """camera.py:858-883: the image (imgsz[1], imgsz[0]) of the mean of `values` (n,) over the points `uv` (n, 2) that
        truncate to each pixel, NaN where there is none; `values` (n, d) with d > 1 give (imgsz[1], imgsz[0], d).  The
        means are helpers.rasterize_points': float64 sums in the points' order times 1 / count, formed on the device
        (`glh_stage_rasterize`).  A point exactly on the far edge (u == imgsz[0] or v == imgsz[1]), where the reference
        raises, is out of frame."""
        uv, values = np.asarray(uv), np.asarray(values)
        nx, ny = (int(v) for v in self.imgsz)
        keep = self.inframe(uv) & (uv[:, 0] < nx) & (uv[:, 1] < ny)
        columns = 1 if values.ndim == 1 else values.shape[1]
        picked = np.asarray(values[keep], dtype=np.float64).reshape(int(keep.sum()), columns)
        shape = (ny, nx) if columns == 1 else (ny, nx, columns)
        if not keep.any():
            return np.full(shape, np.nan)
        keys = uv[keep, 1].astype(int) * nx + uv[keep, 0].astype(int)
        return _lib.stage_rasterize(keys, picked, nx * ny).reshape(shape)

    def project_dem(self, dem, values=None, mask=None, tile_size=(256, 256), tile_overlap=(1, 1), scale=1,
                    scale_limits=(1, 1), parallel=False, return_depth=False):
        """camera.py:967-1129: the image (imgsz[1], imgsz[0], layers) this camera records of the `values` (one per cell,
        2-D or with layers along a third axis) draped over the `dem` (a Raster), with the depth of the surface along the
        optical axis appended as the last layer when `return_depth`; NaN where no cell lands.  `mask`: the cells to
        include (default: those with an elevation).  Computed on the GPU (`glh_stage_project_dem`) with the reference's
        semantics: the DEM is cut into `dem.tile_indices(tile_size, tile_overlap)`; within a tile a pixel is the mean of
        the cells that truncate to it (float64 sum in row-major order, times 1 / count); across tiles there is no depth
        test -- the last tile that reaches a pixel overwrites it, so the tiling is part of the answer.  The value layers
        equal the reference's bit for bit.  `scale` has no effect and `parallel` is ignored; `scale_limits` other than
        (1, 1) -- the per-tile rescaling, which fails in the reference itself -- is not built.  A cell exactly on the far
        edge of the frame (u == imgsz[0] or v == imgsz[1]), where the reference raises, is out of frame."""
        if min(scale_limits) != 1 or max(scale_limits) != 1:
            raise NotImplementedError("project_dem rescales no tile: scale_limits must be (1, 1)")
        dem_shape = tuple(int(v) for v in dem.size[::-1])
        if values is not None:
            values = np.atleast_3d(values)
            if values.shape[0:2] != dem_shape:
                raise ValueError("values does not have the same 2-d shape as dem")
        elif not return_depth:
            raise ValueError("values cannot be missing if return_depth is False")
        if mask is not None and np.shape(mask) != dem_shape:
            raise ValueError("mask does not have the same 2-d shape as dem")
        if np.ndim(dem.array) != 2:
            raise ValueError(f"a DEM is two-dimensional, got {np.shape(dem.array)}")
        tiles = dem.tile_indices(size=tile_size, overlap=tile_overlap)
        rows = list(dict.fromkeys((i.start, i.stop) for i, _ in tiles))
        cols = list(dict.fromkeys((j.start, j.stop) for _, j in tiles))
        return _lib.stage_project_dem(
            self.vector24, dem.array, values, mask,
            cols, np.concatenate([dem._tile_coordinates(0, a, b) for a, b in cols]),
            rows, np.concatenate([dem._tile_coordinates(1, a, b) for a, b in rows]), return_depth=return_depth)
