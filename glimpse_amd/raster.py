"""`Raster`: the in-memory part of `glimpse.Raster` that the tracking path samples
(the reference's src/glimpse/raster.py): a gridded surface (DEM, DEM uncertainty, viewshed) defined by
its array and outer x / y limits, sampled at points.

Only what `Tracker` / the motion models use is mirrored: the constructor from an array and limits
(raster.py:652-694 with Grid, :25-98), the cell-centre coordinates (`x`, `y`, raster.py:131-165), the
bounds test (`inbounds_xy`, :313-337) and `sample(xy, order in {0, 1})` at points (:913-1027).  Sampling
runs on the GPU (`glh_stage_raster_sample`; inside a tracking run the kernels sample the uploaded
raster themselves).  Of the terrain analysis, `viewshed(origin, correction)` (:1293-1389) is served, on the GPU
(`glh_stage_viewshed`): it makes the `Tracker(viewshed=...)` input from a DEM and a camera position.  So is its sibling
`horizon(origin, headings, correction)` (:1391-1463), the visible horizon as world-coordinate lines for camera calibration
(`glh_stage_horizon`: one workgroup per heading; the rays' start and end cells are computed on the host).
`tile_indices(size, overlap)` (:581-610) cuts the grid into the tiles `Camera.project_dem` walks; it and the tiles' own
coordinates (`__getitem__`, :670-693) are computed on the host and handed to the device.  `fill_crevasses` (:1266-1291),
the smoothed surface handed to the motion models, runs on the GPU too (`glh_stage_fill_crevasses`; glimpse_amd/filters.py).
File I/O (GDAL), resampling, `hillshade`, `gradient` are out of scope.
"""
import warnings

import numpy as np

from . import _lib


class Raster:
    def __init__(self, array, x=None, y=None, datetime=None):
        self.array = np.atleast_2d(np.asarray(array))
        ny, nx = self.array.shape[:2]
        self.size = np.array((nx, ny))
        self.xlim = self._limits(x, nx)
        self.ylim = self._limits(y, ny)
        self.datetime = datetime

    @staticmethod
    def _limits(value, n):
        """Grid._parse_xy (raster.py:245-272): outer limits (2,), or cell-centre coordinates (n > 2)."""
        if value is None:
            value = (0, n)
        value = np.atleast_1d(np.asarray(value, dtype=float))
        if value.ndim == 1 and len(value) > 2:
            d = value[1] - value[0]
            value = np.array((value[0] - d / 2, value[-1] + d / 2))
        if value.shape != (2,):
            raise ValueError("Could not parse limits from x, y inputs")
        if value[0] == value[1]:
            raise ValueError("Grid limits cannot be equal")
        return value

    @property
    def d(self):
        """Cell size (dx, dy); negative where the coordinate decreases along the array (raster.py:115-118)."""
        return np.hstack((np.diff(self.xlim), np.diff(self.ylim))) / self.size

    @property
    def min(self):
        return np.array((min(self.xlim), min(self.ylim)))

    @property
    def max(self):
        return np.array((max(self.xlim), max(self.ylim)))

    def _centres(self, dim):
        d = abs(self.d[dim])
        value = np.linspace(start=self.min[dim] + d / 2, stop=self.max[dim] - d / 2, num=self.size[dim])
        return value[::-1] if self.d[dim] < 0 else value

    @property
    def x(self):
        """Cell-centre x from the first to the last column (raster.py:131-147)."""
        return self._centres(0)

    @property
    def y(self):
        """Cell-centre y from the first to the last row (raster.py:149-165)."""
        return self._centres(1)

    # ---- a Raster as an Observer image (orthophoto tracking; observer.py:26, :113, :129, :144)
    @property
    def vector24(self):
        """GLH_CAM_LEN layout in its georeferenced-raster form (include/glimpse_hip.h, entry [23] = 1)."""
        v = np.zeros(_lib.CAM_LEN)
        v[0], v[1] = self.xlim[0], self.ylim[0]
        v[6:8] = self.size
        v[8:10] = self.d
        v[23] = 1.0
        return v

    def xyz_to_uv(self, xyz):
        """Grid.xyz_to_uv (raster.py:423-445), evaluated by the projection kernel."""
        xyz = np.atleast_2d(np.asarray(xyz, dtype=float))
        if xyz.shape[1] == 2:
            xyz = np.column_stack((xyz, np.zeros(len(xyz))))
        return _lib.stage_project(self.vector24, xyz)

    def inbounds(self, uv):
        """Grid.inbounds (raster.py:339-341)."""
        uv = np.atleast_2d(np.asarray(uv, dtype=float))
        return np.all((uv >= 0) & (uv <= self.size), axis=1)

    def read(self, box=None, cache=True):
        """Raster.read of an in-memory array (raster.py:763-837): the window [top:bottom, left:right]."""
        if box is None:
            return self.array
        return self.array[box[1]:box[3], box[0]:box[2]]

    def inbounds_xy(self, xy):
        """raster.py:313-337 (points)."""
        xy = np.atleast_2d(np.asarray(xy, dtype=float))
        return np.all((xy >= self.min[0:2]) & (xy <= self.max[0:2]), axis=1)

    def device_args(self):
        """Arguments of glh_set_raster / glh_stage_raster_sample after `which` / `device_id`."""
        sx, sy = (1 if v > 0 else -1 for v in self.d)
        gx, gy = np.ascontiguousarray(self.x[::sx]), np.ascontiguousarray(self.y[::sy])
        z = np.ascontiguousarray(self.array, dtype=np.float64)
        nx, ny = (int(v) for v in self.size)
        return z, nx, ny, gx, gy, sx, sy, float(self.min[0]), float(self.max[0]), float(self.min[1]), float(self.max[1])

    def tile_indices(self, size, overlap=(0, 0)):
        """Grid.tile_indices (raster.py:581-610): (rows, columns) slice pairs that chop the grid into tiles of about
        `size` = (nx, ny) cells, row-major.  Per axis: round(cells / size) tiles (none rounds to one tile over the whole
        axis, through the reference's division by zero), cell i in tile floor(i / ceil(cells / tiles)); every tile but
        the first starts `overlap` cells early, so overlapping cells belong to both neighbours."""
        axes = []
        for cells, target, lap in zip((int(v) for v in self.size), size, overlap):
            tiles = int(np.round(cells / target))
            with np.errstate(divide="ignore"):
                label = np.floor(np.arange(cells) / np.ceil(np.float64(cells) / tiles))
            ends = np.concatenate(([0], np.searchsorted(label, np.unique(label), side="right")))
            starts = ends.copy()
            starts[1:-1] -= lap
            axes.append([slice(int(a), int(b)) for a, b in zip(starts[:-1], ends[1:])])
        return tuple((i, j) for i in axes[1] for j in axes[0])

    def _tile_coordinates(self, dim, start, stop):
        """Grid.x (dim 0) or Grid.y (dim 1) of the tile `self[start:stop]` along that axis (raster.py:670-693): a tile of
        three or more cells is built from the slice of this raster's coordinates and keeps them; a narrower one is built
        from its outer limits and spaces its own."""
        c = self._centres(dim)[start:stop]
        if len(c) >= 3:
            return c
        lim = c[[0, -1]] + np.array((-0.5, 0.5)) * self.d[dim]
        d = (lim[1] - lim[0]) / len(c)
        value = np.linspace(start=min(lim) + abs(d) / 2, stop=max(lim) - abs(d) / 2, num=len(c))
        return value[::-1] if d < 0 else value

    def viewshed(self, origin, correction=False):
        """The binary viewshed from a point (raster.py:1293-1389): bool, shape of `array`, True where a cell is seen from
        `origin` (x, y, z).  `correction`: False / None, True (default arguments) or the arguments of
        helpers.elevation_corrections (`radius`, `refraction`; helpers.py:1771-1790).  Computed on the GPU
        (`glh_stage_viewshed`) by the reference's own algorithm -- cells ordered by distance ring and heading, rings swept
        outwards against the interpolated running maximum of the elevation ratio -- with its quirks: the cell under an
        origin that sits on a cell centre is never tested (False), a raster whose cells all lie within half a cell of
        the origin is all True."""
        if not all(abs(self.d[0]) == abs(self.d)):
            warnings.warn(
                "DEM cells not square "
                + str(tuple(abs(self.d)))
                + " - "
                + "may lead to unexpected results"
            )
        if not self.inbounds_xy(np.atleast_2d(origin[0:2])):
            warnings.warn("Origin not in DEM - may lead to unexpected results")
        _lib.viewshed_correction(correction)  # (a TypeError for an unknown argument comes before anything else)
        if self.array.ndim != 2:
            raise ValueError(f"a DEM is two-dimensional, got {self.array.shape}")
        z, flag = _lib.viewshed_dem(self.array, origin[2])
        # every cell within half a cell of the origin (ring 0 only): "Single co-located pixel, return all visible"
        # (raster.py:1339-1345).  The farthest cell is a corner, and the ring number grows with the distance.
        x, y = self.x, self.y
        dx = max(abs(x[0] - origin[0]), abs(x[-1] - origin[0]))
        dy = max(abs(y[0] - origin[1]), abs(y[-1] - origin[1]))
        if int(np.sqrt(dx ** 2 + dy ** 2) * (1 / abs(self.d[0])) + 0.5) == 0:
            return np.ones(self.array.shape, dtype=bool)
        xyz = np.array([[float(origin[0]), float(origin[1]), float(origin[2])]])
        return _lib.stage_viewshed(self, xyz, correction, float32=flag == _lib.VIEWSHED_F32)[0]

    def _snapped_colrow(self, xy):
        """Grid.xy_to_rowcol(xy, snap=True) (raster.py:478-500 through snap_xy, :343-388) as (col, row): the cell each point
        falls in, a point on a cell edge in the higher one, an exact hit on the far outer edges in the last one."""
        corner = np.append(self.xlim[0], self.ylim[0])
        nxy = (xy - corner) / self.d
        nxy -= 0.5
        nxy = np.floor(nxy + 0.5)
        nxy[xy == np.append(self.xlim[1], self.ylim[1])] -= 1
        nxy += 0.5
        snapped = nxy * self.d + corner
        return ((snapped - corner) / self.d - 0.5).astype(int)

    def _horizon_rays(self, origin, headings):
        """(start (2,), ends (n, 2)) of Raster.horizon's lines as (col, row) (raster.py:1418-1434): the origin's cell, and
        per heading (degrees clockwise from north) the cell where the ray leaves the raster's box -- the exits of
        helpers.intersect_rays_box (helpers.py:955-1001) in two dimensions, snapped.  The end cells are then clamped into
        the grid: an exit that lies a rounding error outside the box snaps to row or column -1 or `size`, where the
        reference raises (its snap repairs only exact hits on the far edges)."""
        headings = np.array(headings, dtype=float)
        thetas = -(headings - 90) * (np.pi / 180)
        directions = np.column_stack((np.cos(thetas), np.sin(thetas)))
        with np.errstate(divide="ignore", invalid="ignore"):
            invdir = 1 / directions
            neg = invdir < 0
            tmin = (np.where(neg[:, 0], self.max[0], self.min[0]) - origin[0]) * invdir[:, 0]
            tmax = (np.where(neg[:, 0], self.min[0], self.max[0]) - origin[0]) * invdir[:, 0]
            tymin = (np.where(neg[:, 1], self.max[1], self.min[1]) - origin[1]) * invdir[:, 1]
            tymax = (np.where(neg[:, 1], self.min[1], self.max[1]) - origin[1]) * invdir[:, 1]
            misses = (tmin > tymax) | (tymin > tmax)
            tmax[misses] = np.nan
            y_first = tymax < tmax
            tmax[y_first] = tymax[y_first]
            tmax[tmax < 0] = np.nan
        xy_ends = np.array((origin[0], origin[1])) + tmax[:, None] * directions
        if not np.isfinite(xy_ends).all():
            raise ValueError("a ray from the origin does not leave the raster's box at a finite point")
        start = self._snapped_colrow(np.array([[origin[0], origin[1]]]))[0]
        ends = self._snapped_colrow(xy_ends)
        nx, ny = (int(v) for v in self.size)
        return start, np.column_stack((np.clip(ends[:, 0], 0, nx - 1), np.clip(ends[:, 1], 0, ny - 1)))

    def _horizon_points(self, origin, headings, correction):
        """hxyz (n, 3) of Raster.horizon before it is split into runs (raster.py:1436-1459): per heading the horizon point
        [x, y, z], NaN where the heading has none."""
        _lib.viewshed_correction(correction)  # (a TypeError for an unknown argument comes before anything else)
        if self.array.ndim != 2:
            raise ValueError(f"a DEM is two-dimensional, got {self.array.shape}")
        z, flag = _lib.viewshed_dem(self.array, origin[2])
        n = len(headings)
        if n == 0:
            return np.full((0, 3), np.nan)
        origin_xyz = tuple(float(v) for v in origin[0:3])
        if not self.inbounds_xy(np.atleast_2d(origin_xyz[0:2]))[0]:
            raise ValueError(f"origin {origin_xyz[0:2]} is outside the raster (x {tuple(self.xlim)}, y {tuple(self.ylim)}): "
                             "the horizon is computed from a position inside the DEM")
        start, ends = self._horizon_rays(origin_xyz, headings)
        cell, dz = _lib.stage_horizon(self, np.array([origin_xyz]), start[None, :], ends[None, :, :], correction,
                                      float32=flag == _lib.VIEWSHED_F32)
        cell, dz = cell[0], dz[0]
        found = cell[:, 0] >= 0
        hxyz = np.full((n, 3), np.nan)
        hxyz[found, 0:2] = (cell[found] + 0.5)[:, ::-1] * self.d + np.array((self.xlim[0], self.ylim[0]))
        hxyz[found, 2] = dz[found]
        hxyz[:, 2] += origin_xyz[2]
        return hxyz

    def horizon(self, origin, headings=range(360), correction=False):
        """The horizon from a point (raster.py:1391-1463): a list of (k, 3) float64 arrays, each an unbroken run of horizon
        points [x, y, z] in heading order.  `headings`: degrees clockwise from north; `correction` as in `viewshed`.  Per
        heading the cells of the Bresenham line from the origin's cell to the cell where the ray leaves the raster are
        taken (the origin's cell skipped, NaN cells ignored), and the horizon point is the centre of the cell of greatest
        elevation ratio, with its own elevation -- unless that cell is the line's last with a value, which is no horizon.
        Runs are split where a heading has no point, circularly: the last run joins the first.  The lines are computed on
        the GPU (`glh_stage_horizon`), bit for bit what the reference computes.  `origin` must lie inside the raster (the
        reference raises for one outside, too).  One departure: the end cell of every ray is clamped into the grid, where
        the reference raises for the many headings whose exit lies a rounding error outside the box."""
        hxyz = self._horizon_points(origin, headings, correction)
        if len(hxyz) == 0:
            return []
        # helpers.boolean_split(hxyz, mask, axis=0, circular=True)[mask[0]::2] (helpers.py:799-803)
        mask = np.isnan(hxyz[:, 0])
        cuts = np.nonzero(mask[1:] != mask[:-1])[0] + 1
        splits = np.split(hxyz, cuts, axis=0)
        if len(splits) > 1 and mask[0] == mask[-1]:
            splits[0] = np.concatenate((splits[-1], splits[0]), axis=0)
            splits.pop(-1)
        return splits[int(mask[0])::2]

    def fill_crevasses(self, maximum={"size": 5}, gaussian={"sigma": 5}, mask=None, fill=False):
        """A maximum filter of the values, then Gaussian smoothing (raster.py:1266-1291), in place: `array` becomes
        gaussian_filter(maximum_filter(array, **maximum, mask, fill), **gaussian, mask, fill) of glimpse_amd.filters, bit
        for bit the reference's.  `mask`: True where a cell is included, or a callable that makes it from `array`; the
        same mask goes to both filters.  `fill`: excluded cells take interpolated values (NaN where no included cell is
        in reach) instead of keeping their own.  One library call (`glh_stage_fill_crevasses`): the maximum never leaves
        the device.  What is served and refused: glimpse_amd/filters.py."""
        from . import filters

        if callable(mask):
            mask = mask(self.array)
        self.array = filters.fill_crevasses(self.array, maximum, gaussian, mask=mask, fill=fill)

    def sample(self, xy, grid=False, order=1, bounds_error=True, fill_value=np.nan):
        """Values at points (n, 2): bilinear (order 1) or nearest cell (order 0) (raster.py:913-1027)."""
        if grid or order not in (0, 1):
            raise NotImplementedError("only point sampling with order 0 or 1 is built")
        xy = np.atleast_2d(np.asarray(xy, dtype=float))
        values, oob = _lib.stage_raster_sample(self, xy, order)
        if oob.any():
            if bounds_error:
                raise ValueError("Some of the sampling coordinates are out of bounds")
            values[oob] = fill_value
        return values
