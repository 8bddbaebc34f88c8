"""`optimize`: orienting the images of an `Observer` from point matches between image pairs
(the reference's optimize.py: `Matches` :462-740, `RotationMatches*` :743-975, `ObserverCameras` :1974-2083).

`ObserverCameras.fit` finds one view direction per image, with one or more anchor images held in place, by minimising the
L1 distance between the matched unit ray directions with BFGS.  Its objective and gradient -- a map over every match of
every pair and a segmented sum -- are evaluated on the GPU (`glh_orient_eval`): the matches are uploaded once per fit and
the callback sends 36 doubles per image (R and Rprime, made on the host by `camera.rotations` so that their bits are
NumPy's) and receives 3 per image and the objective.  The summation order is fixed, so a fit is reproducible
to the bit.  The match classes predict through the projection kernels.

Not served: detecting and matching keypoints (`KeypointMatcher`: SIFT and FLANN of `cv2`) -- matches are passed in --
and `Cameras.fit`, `Points`, `Lines`, `ransac`, `Polynomial` and plotting.
"""
import sys

import numpy as np

from . import _lib
from .camera import rotations

_NO_MATCHER = ("keypoint detection and matching (SIFT and FLANN of cv2) are not served: pass the matches to "
               "ObserverCameras(observer, matches=...)")


class Matches:
    """optimize.py:462-740: point matches `uvs` = [(n, 2), (n, 2)] between the two cameras `cams` at one position."""

    def __init__(self, cams, uvs, weights=None):
        self.cams = cams
        self.uvs = [np.asarray(uv, dtype=float) for uv in uvs]
        self.weights = weights
        self._test_matches()
        self._test_position()
        self._imgszs = [cam.imgsz.copy() for cam in cams]

    @property
    def size(self):
        return len(self.uvs[0])

    def _test_matches(self):
        if self.cams[0] is self.cams[1]:
            raise ValueError("Both cameras are the same object")
        uvs = self.uvs or self.xys  # (subclasses with camera coordinates and optional uvs)
        if len(self.cams) != 2 or len(uvs) != 2:
            raise ValueError("Cameras and point coordinates do not have two elements each")
        if len(uvs[0]) != len(uvs[1]):
            raise ValueError("Camera point coordinates do not have the same length")

    def _test_position(self):
        if any(self.cams[0].xyz != self.cams[1].xyz):
            raise ValueError("Cameras have different positions")

    def _cam_index(self, cam):
        if isinstance(cam, int):
            if cam >= len(self.cams):
                raise IndexError("Camera index out of range")
            return cam
        return [c is cam for c in self.cams].index(True)

    def observed(self, cam=0, index=slice(None)):
        return self.uvs[self._cam_index(cam)][index]

    def predicted(self, cam=0, index=slice(None)):
        """Image coordinates in `cam` of the other camera's points (unprojection and projection kernels)."""
        self._test_position()
        ci = self._cam_index(cam)
        co = 0 if ci else 1
        dxyz = self.cams[co].uv_to_xyz(self.uvs[co][index])
        return self.cams[ci].xyz_to_uv(dxyz, directions=True)

    def plot(self, *args, **kwargs):
        raise NotImplementedError("plotting is out of scope")

    def to_type(self, mtype):
        if mtype is type(self):
            return self
        return mtype(cams=self.cams, uvs=self.uvs, weights=self.weights)

    def resize(self, size=None, force=False):
        """optimize.py:653-675: resize the cameras (unless `size` is None) and scale the image coordinates to them."""
        for i, cam in enumerate(self.cams):
            if size is not None:
                cam.resize(size=size, force=force)
            scale = cam.imgsz / self._imgszs[i]
            if np.any(scale != 1):
                self.uvs[i] = self.uvs[i] * scale
                self._imgszs[i] = cam.imgsz.copy()

    def filter(self, n_best=None, min_weight=None, cam=0, max_error=None, max_distance=None, scaled=False):
        """optimize.py:677-740.  Where a subclass holds both image and camera coordinates, both are filtered (the
        reference filters the image coordinates alone and leaves the two out of step)."""
        selected = np.ones(self.size, dtype=bool)
        if (n_best or min_weight) and self.weights is None:
            raise ValueError("Filtering on weights failed since these are missing")
        if self.weights is not None:
            if n_best:
                order = np.argsort(-self.weights)
                selected[order[min(n_best, self.size):]] = False
            if min_weight:
                selected &= self.weights >= min_weight
        ci = self._cam_index(cam)
        co = 0 if ci else 1
        if max_error and selected.any():
            if scaled:
                max_error = max_error * self.cams[ci].imgsz[0]
            errors = np.linalg.norm(self.observed(ci, index=selected) - self.predicted(ci, index=selected), axis=1)
            selected[selected] &= errors <= max_error
        if max_distance and selected.any():
            if scaled:
                max_distance = max_distance * self.cams[ci].imgsz[0]
            scale = self.cams[ci].imgsz / self.cams[co].imgsz
            distances = np.linalg.norm(self.observed(co, index=selected) * scale - self.observed(ci, index=selected), axis=1)
            selected[selected] &= distances <= max_distance
        if self.uvs:
            self.uvs = [uv[selected] for uv in self.uvs]
        if getattr(self, "xys", None):
            self.xys = [xy[selected] for xy in self.xys]
        if self.weights is not None:
            self.weights = self.weights[selected]


class RotationMatches(Matches):
    """optimize.py:743-832: as `Matches`, with the normalised camera coordinates `xys` computed once (on the GPU), so the
    cameras' internal parameters must not change afterwards."""

    def __init__(self, cams, uvs=None, xys=None, weights=None):
        self.cams = cams
        self.uvs, self.xys = self._initialize_uvs_xys(uvs, xys)
        self.uvs = self._build_uvs()
        self.xys = self._build_xys()
        self.weights = weights
        self._test_matches()
        self._internals = [cam.to_array()[6:] for cam in self.cams]  # imgsz, f, c, k, p

    def _initialize_uvs_xys(self, uvs=None, xys=None):
        if uvs is None and xys is None:
            raise ValueError("Both uvs and xys are missing")
        if uvs is not None:
            uvs = [np.asarray(uv, dtype=float) for uv in uvs]
        if xys is not None:
            xys = [np.asarray(xy, dtype=float) for xy in xys]
        return uvs, xys

    def _build_xys(self):
        if self.xys is None:
            return [cam._uv_to_xy(uv) for cam, uv in zip(self.cams, self.uvs)]
        return self.xys

    def _build_uvs(self):
        if self.uvs is None:
            return [cam._xy_to_uv(xy) for cam, xy in zip(self.cams, self.xys)]
        return self.uvs

    def _test_internals(self):
        if any((cam._vector[6:] != v).any() for cam, v in zip(self.cams, self._internals)):
            raise ValueError("Camera internal parameters (imgsz, f, c, k, p) have changed")

    def predicted(self, cam=0, index=slice(None)):
        self._test_position()
        self._test_internals()
        ci = self._cam_index(cam)
        co = 0 if ci else 1
        dxyz = self.cams[co]._xy_to_xyz(self.xys[co][index])
        return self.cams[ci].xyz_to_uv(dxyz, directions=True)


class RotationMatchesXY(RotationMatches):
    """optimize.py:835-919: `observed` and `predicted` are normalised camera coordinates; the image coordinates may be
    left out."""

    def __init__(self, cams, uvs=None, xys=None, weights=None):
        self.cams = cams
        self.uvs, self.xys = self._initialize_uvs_xys(uvs, xys)
        self.xys = self._build_xys()
        self.weights = weights
        self._test_matches()
        self._internals = [cam.to_array()[6:] for cam in self.cams]

    @property
    def size(self):
        return len(self.xys[0])

    def observed(self, cam=0, index=slice(None)):
        return self.xys[self._cam_index(cam)][index]

    def predicted(self, cam=0, index=slice(None)):
        self._test_position()
        self._test_internals()
        ci = self._cam_index(cam)
        co = 0 if ci else 1
        dxyz = self.cams[co]._xy_to_xyz(self.xys[co][index])
        return self.cams[ci]._xyz_to_xy(dxyz, directions=True)

    def to_type(self, mtype):
        if mtype is type(self):
            return self
        if mtype is Matches:
            return mtype(cams=self.cams, uvs=self._build_uvs(), weights=self.weights)
        return mtype(cams=self.cams, uvs=self.uvs, xys=self.xys, weights=self.weights)


class RotationMatchesXYZ(RotationMatchesXY):
    """optimize.py:922-974: `predicted` is the unit ray direction of a camera's own points; what `ObserverCameras` takes."""

    def predicted(self, cam=0, index=slice(None)):
        self._test_position()
        self._test_internals()
        c = self._cam_index(cam)
        dxyz = self.cams[c]._xy_to_xyz(self.xys[c][index])
        dxyz *= 1 / np.linalg.norm(dxyz, ord=2, axis=1, keepdims=True)
        return dxyz

    def observed(self, *args, **kwargs):
        raise NotImplementedError()


class KeypointMatcher:
    """optimize.py (`KeypointMatcher`): not served."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(_NO_MATCHER)


def match_pairs(matches):
    """[(RotationMatchesXYZ, i, j)] of `matches` in the order scipy.sparse.coo_matrix lists them ("COO order"): an (n, n)
    object array with None or 0 where there is no pair, read row by row; an object with `data`, `row` and `col`; or a
    dict {(i, j): matches} in insertion order."""
    if matches is None:
        raise ValueError("matches are missing")
    if isinstance(matches, dict):
        return [(m, int(i), int(j)) for (i, j), m in matches.items()]
    if all(hasattr(matches, name) for name in ("data", "row", "col")):
        return [(m, int(i), int(j)) for m, i, j in zip(matches.data, matches.row, matches.col)]
    grid = np.asarray(matches, dtype=object)
    if grid.ndim != 2 or grid.shape[0] != grid.shape[1]:
        raise ValueError(f"matches as an array are (n, n), got {grid.shape}")
    return [(grid[i, j], i, j) for i in range(grid.shape[0]) for j in range(grid.shape[1])
            if not (grid[i, j] is None or (isinstance(grid[i, j], (int, float)) and grid[i, j] == 0))]


class ObserverCameras:
    """optimize.py:1974-2083: the view directions of the images of `observer` that best align the `matches` between
    them, with the `anchors` (image indices, default the first) held at their original view directions."""

    def __init__(self, observer, matches=None, anchors=None):
        self.observer = observer
        if anchors is None:
            anchors = [0]
        self.anchors = anchors
        self.matches = matches
        self.matcher = None  # (a KeypointMatcher in the reference)
        self.device_id = 0
        self.viewdirs = np.vstack([img.cam.viewdir.copy() for img in self.observer.images])

    def set_cameras(self, viewdirs):
        for i, img in enumerate(self.observer.images):
            img.cam.viewdir = viewdirs[i]

    def reset_cameras(self):
        self.set_cameras(viewdirs=self.viewdirs.copy())

    def build_keypoints(self, **kwargs):
        raise NotImplementedError(_NO_MATCHER)

    def build_matches(self, **kwargs):
        raise NotImplementedError(_NO_MATCHER)

    def upload(self):
        """The matches on the device, as `_lib.Orient` (what `fit` evaluates; close it after use)."""
        pairs = match_pairs(self.matches)
        cams = [img.cam for img in self.observer.images]
        for m, i, j in pairs:
            if not (0 <= i < len(cams) and 0 <= j < len(cams)) or m.cams[0] is not cams[i] or m.cams[1] is not cams[j]:
                raise ValueError(f"matches ({i}, {j}) are not between the cameras of images {i} and {j} of the observer")
            m._test_position()
            m._test_internals()
        offsets = np.concatenate(([0], np.cumsum([m.size for m, _, _ in pairs]))).astype(np.int64)
        xy_i = np.concatenate([np.empty((0, 2))] + [np.asarray(m.xys[0], dtype=float).reshape(-1, 2) for m, _, _ in pairs])
        xy_j = np.concatenate([np.empty((0, 2))] + [np.asarray(m.xys[1], dtype=float).reshape(-1, 2) for m, _, _ in pairs])
        return _lib.Orient(len(cams), [i for _, i, _ in pairs], [j for _, _, j in pairs], offsets, xy_i, xy_j,
                           device_id=self.device_id)

    def evaluate(self, handle, viewdirs, anchor_weight=1e6):
        """(objective, gradient (n, 3)) at `viewdirs` (n, 3): the anchor term (host, first, as in the reference) plus the
        matches' (device).  The reference's formula, quirks included: the gradient uses Rprime of a pair's first image
        only and ignores the normalisation of the rays; match weights play no part."""
        viewdirs = np.asarray(viewdirs, dtype=float).reshape(-1, 3)
        objective = 0
        gradients = np.zeros(viewdirs.shape)
        for i in self.anchors:
            objective += (anchor_weight / 2.0) * np.sum((viewdirs[i] - self.viewdirs[i]) ** 2)
            gradients[i] += anchor_weight * (viewdirs[i] - self.viewdirs[i])
        R, Rprime = rotations(viewdirs)
        match_objective, match_gradients = handle.eval(R, Rprime)
        return objective + match_objective, gradients + match_gradients

    def fit(self, anchor_weight=1e6, method="bfgs", **kwargs):
        """optimize.py:2024-2083: scipy.optimize.minimize (`method`, `kwargs`) from the images' current view directions,
        on the objective and gradient of `evaluate`.  Returns its OptimizeResult (`x` flat: reshape to (-1, 3)).  The
        cameras are not written during the evaluations (nothing reads them: R and Rprime come from the view directions
        directly) and are at their original view directions afterwards, as after the reference's."""
        import scipy.optimize

        with self.upload() as handle:

            def fun(viewdirs):
                objective, gradients = self.evaluate(handle, viewdirs, anchor_weight=anchor_weight)
                sys.stdout.write("\r" + str(objective))
                sys.stdout.flush()
                return objective, gradients.ravel()

            viewdirs_0 = np.array([img.cam.viewdir for img in self.observer.images], dtype=float).ravel()
            result = scipy.optimize.minimize(fun=fun, x0=viewdirs_0, jac=True, method=method, **kwargs)
        self.reset_cameras()
        if not result.success:
            sys.stdout.write("\n")
            print(result.message)
        return result
