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
Resampling is served on the GPU as well: `sample(xy, grid=True, order 1 .. 5)` (:961-999, :1042-1070), the interpolating
`RectBivariateSpline` of the reference evaluated on a grid (`glh_stage_raster_regrid`: banded LU factors made on the host,
one kernel substituting down the columns, one along the rows through LDS tiles, one evaluating), `resample(grid)`
(:1072-1083), `resize(scale)` (:1178-1187, `glh_stage_zoom_linear`), and `RasterInterpolant` (:1528-1771), the DEM and
its uncertainty for a day between two DEMs (`glh_stage_raster_interpolate`: the regridding of the second raster and the
blend in one call).  Their host-only companions are restated here: `copy`, `grid` (a `Grid`, equal to another by shape and
limits), `box2d`, `crop_extent` / `crop`.
The rest of the raster tooling is served too: `gradient` (:1465-1474, `glh_stage_gradient`) and `hillshade` (:1249-1264,
`glh_stage_hillshade`: matplotlib's LightSource.hillshade without matplotlib) are one stencil kernel each over the DEM;
`rasterize_polygons` (:1121-1147) makes masks with `helpers.polygons_to_mask` (`glh_stage_polygon_mask`), by a stated
even-odd rule on cell centres where the reference calls GDAL; `rasterize` (:1103-1119) takes its per-cell means from
`glh_stage_rasterize`.  `fill_circle`, `shift`, `data_extent` and `crop_to_data` are restated on the host.
`intersect_rays(origin, directions, correction)`, which the reference leaves to its users, casts rays onto the bilinear
surface between the cell centres (`glh_stage_raycast`, by the rule of INPUTS.md); `Camera.uv_to_dem` and `xyz_map` use it.
File I/O (GDAL), `plot`, masked arrays and rasters with a singleton dimension (the reference's 1-D `interp1d` path) are out
of scope.
"""
import copy
import datetime
import numbers
import warnings
from pathlib import Path

import numpy as np

from . import _lib, helpers


class SplineOrderError(Exception):
    """`sample(grid=True)` with an order outside 1 .. 5.  The reference hands the order to FITPACK, whose f2py wrapper raises
    its module's own `error`, a direct subclass of Exception: neither a ValueError nor a NotImplementedError, and so is
    this."""


class Grid:
    """Grid (raster.py:23-610) as far as RasterInterpolant needs it: dimensions `size` (nx, ny) and outer limits; two
    grids are equal when their shapes and limits are (raster.py:60-66)."""

    def __init__(self, size, x=None, y=None):
        self.size = np.atleast_1d(size)
        self.xlim = Raster._limits(x, self.size[0])
        self.ylim = Raster._limits(y, self.size[1])

    def __eq__(self, other):
        return bool(self.shape == other.shape and (self.xlim == other.xlim).all() and (self.ylim == other.ylim).all())

    __hash__ = None

    @property
    def shape(self):
        return int(self.size[1]), int(self.size[0])

    @property
    def d(self):
        return np.hstack((np.diff(self.xlim), np.diff(self.ylim))) / self.size

    @property
    def min(self):
        return np.array((min(self.xlim), min(self.ylim)))

    @property
    def max(self):
        return np.array((max(self.xlim), max(self.ylim)))

    @property
    def box2d(self):
        return np.hstack((self.min, self.max))

    @property
    def x(self):
        return Raster._centres(self, 0)

    @property
    def y(self):
        return Raster._centres(self, 1)

    def copy(self):
        return Grid(self.size.copy(), x=self.xlim.copy(), y=self.ylim.copy())


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

    def _cast_rays(self, correction, block, return_times=False, **rays):
        """(t, xyz, patch, status) of `_lib.stage_raycast` for rays cast onto this raster as a DEM, after the checks that
        come before any library call.  `rays`: `origins` and `directions`, or `cam` (a vector24) with `uv` or `step`."""
        if np.ndim(self.array) != 2:
            raise ValueError(f"a DEM is two-dimensional, got {np.shape(self.array)}")
        if min(self.array.shape) < 2:
            raise NotImplementedError(f"a DEM of {self.array.shape} cells has no patch between cell centres "
                                      "(rasters with a singleton dimension are not served)")
        block = int(block)
        if block < 0 or block & (block - 1):
            raise ValueError(f"block is 0 or a power of two, got {block}")
        listed = rays.get("directions", rays.get("uv"))
        if listed is not None and len(listed) >= 2 ** 31:
            raise NotImplementedError(f"{len(listed)} rays: fewer than 2^31 are served")
        _lib.viewshed_correction(correction)  # (a TypeError for an unknown argument comes before anything else)
        array = np.asarray(self.array)
        if array.dtype.kind not in "iuf" or array.dtype.itemsize > 8 or array.dtype == np.float16:
            raise TypeError(f"a DEM of dtype {array.dtype}: float64, float32 or integers")
        z = array if array.dtype == np.float32 else np.asarray(array, dtype=np.float64)
        return _lib.stage_raycast(z, self.x, self.y, self.d, correction=correction, block=block, return_times=return_times,
                                  **rays)

    def intersect_rays(self, origin, directions, correction=False, return_depth=False, return_status=False, block=16):
        """Where rays hit this raster as a DEM: xyz (n, 3) of the first intersection of each ray `origin + t directions`
        (t >= 0) with the surface, NaN where there is none.  `origin`: (3,) for every ray, or (n, 3) one each (sun rays
        for a shadow map); `directions` (n, 3), of any length.  The surface is the bilinear patches between the cell
        centres -- what `sample(order=1)` interpolates -- over the rectangle of the outer cell centres; the half-cell rim
        beyond them is not part of it.  The reference has the parts (helpers.intersect_rays_box, intersect_rays_plane,
        bresenham_line) and no such function; the rule is INPUTS.md, "Ray casting: the rule".  `correction` as in
        `viewshed`: the apparent surface sinks by helpers.elevation_corrections of the squared horizontal distance along
        the ray, as Camera.xyz_to_uv sees it.  `return_depth`: also t (n,), in units of the directions' length;
        `return_status`: also, per ray, an index into `_lib.RAYCAST_STATUS` (hit, misses the domain, enters below the
        surface, leaves without a hit, invalid).  `block`: the side, in patches, of the blocks whose highest cell lets a
        ray skip them (0: every patch is marched); the result does not depend on it.  One thread per ray on the GPU
        (`glh_stage_raycast`).  A ray that dips under the surface and comes back out within one patch is not seen."""
        directions = np.asarray(directions, dtype=np.float64)
        if directions.ndim == 1:
            directions = directions[None, :]
        if directions.ndim != 2 or directions.shape[1] != 3:
            raise ValueError(f"directions must be (n, 3), got {directions.shape}")
        origin = np.asarray(origin, dtype=np.float64)
        if origin.shape not in ((3,), (1, 3), (len(directions), 3)):
            raise ValueError(f"origin must be (3,) or ({len(directions)}, 3), got {origin.shape}")
        if len(directions) == 0:
            t, xyz, status = np.empty(0), np.empty((0, 3)), np.empty(0, dtype=np.uint8)
        else:
            t, xyz, _, status = self._cast_rays(correction, block, origins=origin, directions=directions)
        result = (xyz,) + ((t,) if return_depth else ()) + ((status,) if return_status else ())
        return result[0] if len(result) == 1 else result

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

    # ---- terrain tooling: gradient, hillshade, masks (raster.py:1103-1147, :1189-1264, :1465-1525)
    def _terrain_values(self, what):
        """`array` as the gradient kernels take it: two-dimensional with two or more cells on each axis (np.gradient's
        ValueError otherwise), float64 or float32; integers and bool are widened to float64 as np.gradient does."""
        a = self.array
        if a.ndim != 2:
            raise ValueError(f"a raster is two-dimensional, got {a.shape}")
        if min(a.shape) < 2:
            raise ValueError("Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) "
                             "elements are required.")
        if a.dtype.kind in "biu":
            return a.astype(np.float64)
        if a.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise NotImplementedError(f"{what} of a {a.dtype} array: float64 and float32 are built (integers are widened)")
        return a

    def gradient(self):
        """(dzdx, dzdy): the derivatives of `array` with respect to x and y (raster.py:1465-1474),
        np.gradient(array, d[1], d[0]) with the signed cell sizes, on the GPU (`glh_stage_gradient`): central differences
        (f[i+1] - f[i-1]) / (2 h) inside, one-sided (f[1] - f[0]) / h at the two ends of a line.  A float64 array comes
        back bit for bit NumPy's; a float32 array comes back float32 (the difference in float32, the quotient against
        the float64 cell size rounded to float32, as NumPy 2 does); integers and bool are widened to float64."""
        z = self._terrain_values("gradient")
        d = self.d
        return _lib.stage_gradient(z, d[0], d[1])

    def hillshade(self, azimuth=315, altitude=45, **kwargs):
        """The illumination of the surface, float64 in [0, 1] in the shape of `array` (raster.py:1249-1264):
        matplotlib.colors.LightSource(azimuth, altitude).hillshade(array, dx=d[0], dy=d[1], **kwargs) with `kwargs` among
        `vert_exag` and `fraction`, on the GPU (`glh_stage_hillshade`) and without matplotlib.  `azimuth`: degrees clockwise
        from north; `altitude`: degrees above the horizon.  The normal of vert_exag * array (gradients with dy negated)
        is dotted with the light direction; the intensity is scaled by `fraction`, stretched from its own minimum and
        maximum to [0, 1] when they differ by more than 1e-6, and clipped.  matplotlib's quirks are kept: with any NaN
        cell nothing is stretched, and a NaN cell makes its four edge neighbours NaN, not itself.  It differs from
        matplotlib's bytes only through the three-term dot product (summed left to right here, BLAS there): by at most
        a few 2^-52 of the stretch.  `dx` or `dy` among the kwargs is the TypeError the reference raises; masked arrays
        (a Raster holds a plain array) and LightSource.shade are not built."""
        for name in ("dx", "dy"):
            if name in kwargs:
                raise TypeError(f"hillshade() got multiple values for keyword argument '{name}'")
        unknown = sorted(set(kwargs) - {"vert_exag", "fraction"})
        if unknown:
            raise TypeError(f"hillshade() got an unexpected keyword argument '{unknown[0]}'")
        z = self._terrain_values("hillshade")
        az, alt = np.radians(90 - azimuth), np.radians(altitude)
        direction = np.array([np.cos(az) * np.cos(alt), np.sin(az) * np.cos(alt), np.sin(alt)])
        d = self.d
        return _lib.stage_hillshade(z, d[0], -d[1], float(kwargs.get("vert_exag", 1)), direction,
                                    float(kwargs.get("fraction", 1.0)))

    def rasterize(self, xy, values):
        """A copy of `array` with the mean of the `values` (n,) of the points `xy` (n, 2) that fall in each cell written
        over it (raster.py:1103-1119); cells without a point keep their value, points outside the raster are dropped.  The
        points snap to cells on the host; the means are helpers.rasterize_points' on the GPU (`glh_stage_rasterize`: the
        sum in the points' order times 1 / count) and are written to the cells that received a point, so a mean of NaN
        values is told from no point."""
        xy = np.atleast_2d(np.asarray(xy, dtype=float))
        values = np.asarray(values)
        if values.ndim != 1 or len(values) != len(xy):
            raise ValueError(f"one value per point: {len(xy)} points, values of shape {values.shape}")
        if self.array.ndim != 2:
            raise ValueError(f"a raster is two-dimensional, got {self.array.shape}")
        inside = self.inbounds_xy(xy)
        array = self.array.copy()
        if not inside.any():
            return array
        colrow = self._snapped_colrow(xy[inside])
        cells, labels = np.unique(colrow[:, 1] * int(self.size[0]) + colrow[:, 0], return_inverse=True)
        means = _lib.stage_rasterize(labels.ravel(), values[inside].astype(np.float64)[:, None], len(cells))[:, 0]
        array.flat[cells] = means
        return array

    def rasterize_polygons(self, polygons, holes=None):
        """Boolean array in the shape of `array`: the cells inside `polygons` [[(x, y), ...], ...] and outside `holes`
        (raster.py:1121-1147), on the GPU through helpers.polygons_to_mask, whose even-odd rule on cell centres stands in
        for GDAL's.  The vertices go to continuous cell coordinates on the host, as the reference's xy_to_rowcol does."""
        corner = np.append(self.xlim[0], self.ylim[0])
        to_cells = lambda rings, what: [((ring - corner) / self.d - 0.5) + 0.5  # noqa: E731
                                        for ring in helpers.polygon_rings(rings, what)]
        return helpers.polygons_to_mask(to_cells(polygons, "polygon"), self.size,
                                        holes=None if holes is None else to_cells(holes, "hole"))

    def shift(self, dx=None, dy=None, dz=None):
        """Shift the position in place (raster.py:1189-1219)."""
        if dx is not None:
            self.xlim = self.xlim + dx
        if dy is not None:
            self.ylim = self.ylim + dy
        if dz is not None:
            self.array += dz

    def fill_circle(self, center, radius, value=np.nan):
        """Fill a circle around `center` (x, y) with `value`, in place (raster.py:1221-1247): the cells on and inside
        helpers.bresenham_circle around the centre's cell, `radius` / d[0] cells wide (rounded), rows and columns clipped
        to the grid.  On the host.  A raster whose x decreases along the array has a negative radius in cells, which is
        bresenham_circle's ValueError, as in the reference."""
        col, row = self._snapped_colrow(np.atleast_2d(np.asarray(center, dtype=float)[0:2]))[0]
        r = np.round(radius / self.d[0])
        xyi = helpers.bresenham_circle((col, row), r).astype(int)
        nx, ny = (int(v) for v in self.size)
        ind = []
        for yi in np.unique(xyi[:, 1]):
            if not -1 < yi < ny:
                continue
            xb = xyi[xyi[:, 1] == yi, 0]
            xi = np.arange(max(xb.min(), 0), min(xb.max(), nx - 1) + 1)
            ind.append(yi * nx + xi)
        self.array.flat[np.concatenate(ind) if ind else np.zeros(0, dtype=int)] = value

    def data_extent(self):
        """(row slice, column slice) of the region bounding all cells that are not NaN (raster.py:1492-1514); ValueError
        when every cell is NaN."""
        data = ~np.isnan(self.array)
        data_row, data_col = np.any(data, axis=1), np.any(data, axis=0)
        if not data_row.any():
            raise ValueError("No non-missing values present")
        first_row, last_row = np.argmax(data_row), data_row.size - np.argmax(data_row[::-1])
        first_col, last_col = np.argmax(data_col), data_col.size - np.argmax(data_col[::-1])
        return slice(first_row, last_row), slice(first_col, last_col)

    def crop_to_data(self):
        """Crop in place to `data_extent()` (raster.py:1516-1525): the limits are put half a cell beyond the first and last
        kept cell centre."""
        rows, cols = self.data_extent()
        x, y, d = self.x[cols], self.y[rows], self.d
        self._set_array(self.array[rows, cols])
        self.xlim = x[[0, -1]] + np.array((-0.5, 0.5)) * d[0]
        self.ylim = y[[0, -1]] + np.array((-0.5, 0.5)) * d[1]

    # ---- host-only companions of the resampling (restated from the reference)
    def _set_array(self, array):
        self.array = np.atleast_2d(array)
        ny, nx = self.array.shape[:2]
        self.size = np.array((nx, ny))

    def copy(self):
        """raster.py:904-911."""
        return self.__class__(self.array.copy(), x=self.xlim.copy(), y=self.ylim.copy(), datetime=copy.copy(self.datetime))

    @property
    def shape(self):
        return self.array.shape

    @property
    def grid(self):
        """The raster's Grid (raster.py:884-887)."""
        return Grid(self.size, x=self.xlim, y=self.ylim)

    @property
    def box2d(self):
        """(xmin, ymin, xmax, ymax) (raster.py:134-137)."""
        return np.hstack((self.min, self.max))

    def crop_extent(self, xlim=None, ylim=None):
        """Grid.crop_extent (raster.py:526-574): the outer limits (xlim, ylim) and the first and last (rows, cols) of the
        cells a crop to the box keeps: the box is cut to the raster's, its corners snap to the cells they fall in, and a
        far corner that lies exactly on an inner cell edge snaps down, into the cell before it."""
        if xlim is None:
            xlim = self.xlim
        if ylim is None:
            ylim = self.ylim
        box = helpers.intersect_boxes(np.vstack((np.hstack((min(xlim), min(ylim), max(xlim), max(ylim))),
                                                 np.hstack((self.min[0:2], self.max[0:2])))))
        xlim = box[0::2]
        if self.xlim[0] > self.xlim[1]:
            xlim = xlim[::-1]
        ylim = box[1::2]
        if self.ylim[0] > self.ylim[1]:
            ylim = ylim[::-1]
        xy = np.column_stack((xlim, ylim))
        rowcol = self._snapped_colrow(xy)[:, ::-1].copy()
        bottom_right = np.append(self.xlim[1], self.ylim[1])
        is_edge = (bottom_right - xy[1, :]) % self.d == 0
        is_outer_edge = xy[1, :] == bottom_right
        snap_down = is_edge & ~is_outer_edge
        rowcol[1, snap_down[::-1]] -= 1
        new_xy = (rowcol + 0.5)[:, ::-1] * self.d + np.array((self.xlim[0], self.ylim[0]))
        new_xlim = new_xy[:, 0] + np.array([-0.5, 0.5]) * self.d[0]
        new_ylim = new_xy[:, 1] + np.array([-0.5, 0.5]) * self.d[1]
        return new_xlim, new_ylim, rowcol[:, 0], rowcol[:, 1]

    def crop(self, xlim=None, ylim=None, zlim=None):
        """Crop in place (raster.py:1149-1176): to the cells of `crop_extent(xlim, ylim)`; values outside `zlim` become NaN
        (an integer array is cast to float, with the reference's warning)."""
        if xlim is not None or ylim is not None:
            xlim, ylim, rows, cols = self.crop_extent(xlim=xlim, ylim=ylim)
            self._set_array(self.array[rows[0]:rows[1] + 1, cols[0]:cols[1] + 1])
            self.xlim = xlim
            self.ylim = ylim
        if zlim is not None:
            outbounds = (self.array < min(zlim)) | (self.array > max(zlim))
            if np.count_nonzero(outbounds) and not issubclass(self.array.dtype.type, np.floating):
                warnings.warn("array cast to float to accommodate NaN")
                self.array = self.array.astype(float)
            self.array[outbounds] = np.nan

    def resize(self, scale, order=1):
        """Resize `array` in place by the fraction `scale` (raster.py:1178-1187): scipy.ndimage.zoom(array, scale, order=1),
        on the GPU (`glh_stage_zoom_linear`).  The limits stay, so the cell size changes.  Only order 1 and floating
        arrays are built."""
        if order != 1:
            raise NotImplementedError(f"resize with order {order}: only order 1 is built")
        if not issubclass(self.array.dtype.type, np.floating):
            raise NotImplementedError(f"resize of a {self.array.dtype} array: only floating arrays are built")
        if self.array.ndim != 2:
            raise ValueError(f"a raster is two-dimensional, got {self.array.shape}")
        shape = tuple(int(round(n * float(scale))) for n in self.array.shape)
        self._set_array(_lib.stage_zoom_linear(self.array, shape).astype(self.array.dtype, copy=False))

    def resample(self, grid, **kwargs):
        """Resample in place onto the cell centres of `grid`, anything with x, y, xlim, ylim (raster.py:1072-1083);
        `kwargs` go to `sample`."""
        array = self.sample((grid.x, grid.y), grid=True, **kwargs)
        self._set_array(array)
        self.xlim, self.ylim = self._limits(grid.xlim, 0), self._limits(grid.ylim, 0)

    def _grid_source(self, xy, order, bounds_error, fill_value):
        """The host part of `sample(xy, grid=True)` (raster.py:961-999, :1042-1070), in the reference's order: the bounds
        test first, then the shape, the order and the NaN cells.  Returns (source, xo, yo, xout, yout): the
        _lib.regrid_src of this raster with its axes flipped to ascending and the output directions taken from the first
        two requested coordinates; the ascending coordinates; the out-of-bounds columns and rows (None without a test).
        `source` is None for a 1 x 1 raster (a constant)."""
        x, y = (np.atleast_1d(np.asarray(v, dtype=float)) for v in xy)
        if x.ndim != 1 or y.ndim != 1:
            raise ValueError(f"with grid=True the coordinates are two vectors, got {x.shape} and {y.shape}")
        xout = yout = None
        if bounds_error or fill_value is not None:
            xout = ~((x >= self.min[0]) & (x <= self.max[0]))
            yout = ~((y >= self.min[1]) & (y <= self.max[1]))
            if bounds_error and (xout.any() or yout.any()):
                raise ValueError("Some of the sampling coordinates are out of bounds")
        if self.array.ndim != 2:
            raise ValueError(f"a raster is two-dimensional, got {self.array.shape}")
        singleton = int((self.size == 1).sum())
        if singleton == 2:
            return None, x, y, xout, yout
        if singleton == 1:
            raise NotImplementedError("a raster with one singleton dimension is sampled in 1-D by the reference "
                                      "(scipy.interpolate.interp1d): the 1-D case is not built")
        if not isinstance(order, numbers.Integral) or not 1 <= order <= 5:
            raise SplineOrderError(f"order {order!r} with grid=True: the spline orders 1 .. 5 are served (order 0 is point "
                                   "sampling: grid=False)")
        nx, ny = (int(v) for v in self.size)
        if nx <= order or ny <= order:
            raise ValueError(f"order {order} needs more than {order} cells on each axis, the raster has {nx} x {ny}")
        sx, sy = (1 if v > 0 else -1 for v in self.d)
        z = np.asarray(self.array[::sy, ::sx], dtype=np.float64)
        is_nan = np.isnan(z)
        nan_mask = None
        zmin = None
        if is_nan.any():
            if order != 1:
                raise ValueError(f"the raster has {int(is_nan.sum())} NaN cells: they are served at order 1 only.  Above it "
                                 "the fit is global: the reference's stand-in value for a NaN cell rings through every "
                                 "sample, and most of them come back NaN")
            nan_mask = is_nan
            z = np.where(is_nan, 0.0, z)
            if not is_nan.all():
                zmin = float(np.min(self.array[::sy, ::sx][~is_nan]))
        else:
            zmin = float(np.min(self.array))
        if not np.isfinite(z).all():
            raise ValueError("the raster holds infinite values: a spline through them is not defined")
        xdir = 1 if len(x) < 2 or x[1] > x[0] else -1
        ydir = 1 if len(y) < 2 or y[1] > y[0] else -1
        xo, yo = x[::xdir], y[::ydir]
        if (np.diff(xo) <= 0).any() or (np.diff(yo) <= 0).any() or not (np.isfinite(xo).all() and np.isfinite(yo).all()):
            raise ValueError("x and y must be strictly increasing or strictly decreasing when `grid` is True")
        source = _lib.regrid_src(z, self.x[::sx], self.y[::sy], (self.min[0], self.max[0], self.min[1], self.max[1]),
                                 order, order, nan_mask=nan_mask, zmin=zmin, flip_x=xdir < 0, flip_y=ydir < 0)
        return source, xo, yo, xout, yout

    def _sample_grid(self, xy, order, bounds_error, fill_value):
        source, x, y, xout, yout = self._grid_source(xy, order, bounds_error, fill_value)
        if source is None:
            samples = np.full((len(y), len(x)), float(self.array.flat[0]))
        else:
            samples = _lib.stage_raster_regrid(source, x, y)
        if not bounds_error and fill_value is not None:
            samples[yout, :] = fill_value
            samples[:, xout] = fill_value
        return samples

    def sample(self, xy, grid=False, order=1, bounds_error=True, fill_value=np.nan):
        """Values at points (n, 2): bilinear (order 1) or nearest cell (order 0) (raster.py:913-1027).

        With `grid=True`, `xy` = (x (n,), y (m,)) coordinate vectors and the result is float64 (m, n): the reference's
        interpolating scipy.interpolate.RectBivariateSpline of `order` 1 .. 5 over the raster's outer limits, evaluated on
        the grid on the GPU (`glh_stage_raster_regrid`).  The bounds test runs first, per axis.  A descending raster axis is
        flipped; the result follows the order of the requested coordinates, which are strictly monotonic (their direction
        is read off the first two).  `bounds_error=False`: out-of-bounds rows and columns take `fill_value`, or with
        `fill_value=None` the spline's value at the nearest limit (FITPACK clamps).  As in the reference, samples below
        the raster's minimum come back NaN (that is how it marks the reach of a NaN cell, and it also blanks a spline's
        undershoot).  A 1 x 1 raster returns its constant (as (m, n), where the reference returns (n, m)); a raster with one
        singleton dimension is not built.  NaN cells are served at order 1 only, by a rule that is local where the
        reference's stand-in value is not: a sample is NaN exactly when a cell of nonzero weight in its support is NaN --
        the two neighbouring cells per axis, and in the end segment, where the first coefficient is extrapolated from
        cells 0 and 1, both of them.  (The reference's own answer differs from this only where a NaN sits in the second or
        second-to-last cell of a line, through float64 overflow of the stand-in.)"""
        if grid:
            return self._sample_grid(xy, order, bounds_error, fill_value)
        if order not in (0, 1):
            raise NotImplementedError("only point sampling with order 0 or 1 is built")
        xy = np.atleast_2d(np.asarray(xy, dtype=float))
        values, oob = _lib.stage_raster_sample(self, xy, order)
        if oob.any():
            if bounds_error:
                raise ValueError("Some of the sampling coordinates are out of bounds")
            values[oob] = fill_value
        return values


class RasterInterpolant:
    """Interpolation of a raster time series (raster.py:1528-1771): `means` and `sigmas` hold Rasters or numbers (infinite
    rasters; `sigmas=None` is 0), `x` their coordinates, numbers or datetimes (default: the means' `datetime`).  A call
    takes the two rasters nearest `xi`, crops them to their common box, brings the second onto the first's grid
    (`Raster.resample`, order 1) and blends them linearly in `xi`; with `return_sigma` the two uncertainty rasters are
    propagated the same way.  The regridding and the blend are one library call (`glh_stage_raster_interpolate`) in
    float64 (float32 rasters are widened, where the reference blends them in float32).  A path among the means or sigmas
    raises NotImplementedError: file I/O is out of scope.

    The reference's quirks are kept: `d` resizes by `d / mean|d|`, which REFINES a raster asked for a coarser cell (a 10 m
    raster with d=20 comes back at 5 m); `d` and the limits are compared by exact float equality; the returned rasters
    carry `means[0]`'s limits."""

    def __init__(self, means, sigmas=None, x=None):
        self.means = means
        if x is None:
            x = [raster.datetime for raster in means]
        self.x = np.asarray(x)
        self.sigmas = sigmas

    def _parse_as_raster(self, obj, xi=None, d=None, xlim=None, ylim=None):
        """raster.py:1555-1592."""
        t = xi if isinstance(xi, datetime.datetime) else None
        if isinstance(obj, numbers.Number):
            if xlim is None:
                xlim = (-np.inf, np.inf)
            if ylim is None:
                ylim = (-np.inf, np.inf)
            return Raster(obj, x=xlim, y=ylim, datetime=t)
        if isinstance(obj, Raster):
            d_change = d is not None and d != np.abs(obj.d).mean()
            xlim_change = xlim is not None and sorted(xlim) != sorted(obj.xlim)
            ylim_change = ylim is not None and sorted(ylim) != sorted(obj.ylim)
            if any((d_change, xlim_change, ylim_change)):
                obj = obj.copy()
            if xlim_change or ylim_change:
                obj.crop(xlim=xlim, ylim=ylim)
            if d_change:
                scale = d / np.abs(obj.d).mean()
                obj.resize(scale)
            return obj
        if isinstance(obj, (str, Path)):
            raise NotImplementedError(f"a raster file ({obj}): file I/O is out of scope, read it into a Raster first")
        raise ValueError("Cannot cast as Raster: " + str(type(obj)))

    def _read_mean(self, index, d=None, xlim=None, ylim=None, zlim=None, fun=None, **kwargs):
        """raster.py:1594-1614: `fun` is called on a copy, on the host."""
        xi = self.x[index]
        obj = self.means[index]
        raster = self._parse_as_raster(obj, xi, d=d, xlim=xlim, ylim=ylim)
        if (zlim is not None or fun is not None) and raster is obj:
            raster = raster.copy()
        if zlim is not None:
            raster.crop(zlim=zlim)
        if fun is not None:
            fun(raster, **kwargs)
        return raster

    def _read_sigma(self, index, d=None, xlim=None, ylim=None):
        """raster.py:1616-1629."""
        xi = self.x[index]
        obj = 0 if self.sigmas is None else self.sigmas[index]
        return self._parse_as_raster(obj, xi, d=d, xlim=xlim, ylim=ylim)

    def _read_mean_grid(self, index):
        """raster.py:1631-1640."""
        obj = self.means[index]
        if isinstance(obj, Raster):
            return obj.grid
        if isinstance(obj, (str, Path)):
            raise NotImplementedError(f"a raster file ({obj}): file I/O is out of scope, read it into a Raster first")
        if isinstance(obj, numbers.Number):
            return Grid((1, 1), x=(-np.inf, np.inf), y=(-np.inf, np.inf))
        raise ValueError("Cannot cast as Grid: " + str(type(obj)))

    def nearest(self, xi, extrapolate=False):
        """Indices of the two nearest rasters, in the order of their coordinates (raster.py:1642-1671): one on either side
        of `xi`, or with `extrapolate` the two nearest wherever they lie."""
        dx = self.x - xi
        zero = type(dx[0])(0)
        if extrapolate:
            i, j = abs(dx).argsort()[:2]
        else:
            before = np.where(dx <= zero)[0]
            after = np.where(dx >= zero)[0]
            if not before.size or not after.size:
                raise ValueError("Not bounded on both sides by a Raster")
            i = before[np.argmin(abs(dx[before]))]
            j = after[np.argmin(dx[after])]
        ij = [i, j]
        ij.sort(key=lambda index: self.x[index])
        return tuple(ij)

    @staticmethod
    def _second(pair, originals):
        """What the blend takes for the second raster of `pair`: its array when the grids are equal, else the source of its
        regridding onto the first's grid (Raster.resample with the default arguments, raster.py:1757-1760), with the
        ascending centres of that grid.  A raster that is not two-dimensional in extent (a number) is resampled here."""
        first, second = pair
        if first.grid == second.grid:
            return second.array, None, None
        if (second.size > 1).all():
            source, xo, yo, _, _ = second._grid_source((first.x, first.y), 1, True, np.nan)
            return source, xo, yo
        if any(second is o for o in originals):
            second = second.copy()
        second.resample(first)
        return second.array, None, None

    def _interpolate(self, means, x, xi, sigmas=None):
        """raster.py:1673-1700, the arrays' arithmetic on the device in the reference's operation order."""
        dx = x[1] - x[0]
        scale = (xi - x[0]) / dx
        t = xi if isinstance(xi, datetime.datetime) else None
        m1, xo, yo = self._second(means, self.means)
        m0 = np.asarray(means[0].array, dtype=np.float64)
        if not isinstance(m1, tuple):
            m0, m1 = (np.ascontiguousarray(a) for a in np.broadcast_arrays(m0, np.asarray(m1, dtype=np.float64)))
        s0 = s1 = None
        scale2 = ratio = 0.0
        if sigmas is not None:
            scale2 = scale ** 2
            nearest_dx = np.min(np.abs(np.subtract(xi, x)))
            ratio = nearest_dx / dx
            if sigmas[0].grid != sigmas[1].grid and sigmas[0].grid != means[0].grid:
                # the sigmas have a grid of their own: regrid them in a call of their own
                if self.sigmas is not None and any(sigmas[1] is o for o in self.sigmas):
                    sigmas[1] = sigmas[1].copy()
                sigmas[1].resample(sigmas[0])
            s1, sxo, syo = self._second(sigmas, self.sigmas if self.sigmas is not None else ())
            if isinstance(s1, tuple):
                xo, yo = sxo, syo
                s0 = np.asarray(sigmas[0].array, dtype=np.float64)
                if s0.shape != m0.shape:
                    raise ValueError(f"the sigma rasters ({s0.shape}) and the mean rasters ({m0.shape}) differ in shape")
            else:
                s0 = np.ascontiguousarray(np.broadcast_to(np.asarray(sigmas[0].array, dtype=np.float64), m0.shape))
                s1 = np.ascontiguousarray(np.broadcast_to(np.asarray(s1, dtype=np.float64), m0.shape))
        z, sigma = _lib.stage_raster_interpolate(m0, m1, scale, scale2, ratio, s0=s0, s1=s1, xo=xo, yo=yo)
        raster = means[0].__class__(z, x=means[0].xlim, y=means[0].ylim, datetime=t)
        if sigmas is not None:
            return raster, raster.__class__(sigma, x=means[0].xlim, y=means[0].ylim, datetime=t)
        return raster

    def __call__(self, xi, d=None, xlim=None, ylim=None, zlim=None, return_sigma=False, extrapolate=False, fun=None,
                 **kwargs):
        """The raster interpolated at `xi`, and with `return_sigma` its standard deviation (raster.py:1702-1771).  `d`:
        target cell size (default: the largest of the two rasters); `xlim`, `ylim`: crop bounds (default: the rasters'
        intersection); `zlim`: values of the means outside it become NaN; `fun(raster, **kwargs)` modifies each mean in
        place before the blend."""
        ij = self.nearest(xi, extrapolate=extrapolate)
        grids = [self._read_mean_grid(k) for k in ij]
        if d is None:
            d = np.max(np.abs(np.stack([grid.d for grid in grids])))
        if xlim is None:
            xlim = (-np.inf, np.inf)
        if ylim is None:
            ylim = (-np.inf, np.inf)
        boxes = [grid.box2d for grid in grids]
        boxes.append([min(xlim), min(ylim), max(xlim), max(ylim)])
        box = helpers.intersect_boxes(boxes)
        xlim, ylim = box[0::2], box[1::2]
        means = [self._read_mean(k, d=d, xlim=xlim, ylim=ylim, zlim=zlim, fun=fun, **kwargs) for k in ij]
        sigmas = [self._read_sigma(k, d=d, xlim=xlim, ylim=ylim) for k in ij] if return_sigma else None
        return self._interpolate(means=means, sigmas=sigmas, x=self.x[list(ij)], xi=xi)
