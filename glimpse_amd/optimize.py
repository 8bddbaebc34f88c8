"""`optimize`: fitting camera models to observations (the reference's optimize.py: `Points` :46-236, `Lines` :239-459,
`Matches` :462-740, `RotationMatches*` :743-975, `Polynomial` :985-1130, `Cameras` :1133-1971, `ObserverCameras`
:1974-2083, `ransac` :2091-2188, `match_keypoints` :2234-2309, `KeypointMatcher` :2312-2773).

`Cameras.fit` finds camera parameters (position, view direction, focal length, distortion ...; per camera or shared by a
group) that minimise the reprojection residuals of its controls -- surveyed points, traced lines, point matches between
cameras -- with scipy.optimize.least_squares.  The residual function, which the optimiser needs once per step and once per
Jacobian column, is evaluated on the GPU (`glh_calib_eval`): the controls are uploaded once per fit and one call
evaluates every (control, perturbed parameter) block of a Jacobian.  What stays on the host is the vertex-level work of
`Lines` (projecting, splitting and clipping the world polylines: the segment table) and the optimiser itself.

`ObserverCameras.fit` finds one view direction per image, with one or more anchor images held in place, by minimising the
L1 distance between the matched unit ray directions with BFGS.  Its objective and gradient -- a map over every match of
every pair and a segmented sum -- are evaluated on the GPU (`glh_orient_eval`): the matches are uploaded once per fit and
the callback sends 36 doubles per image (R and Rprime, made on the host by `camera.rotations` so that their bits are
NumPy's) and receives 3 per image and the objective.  The summation order is fixed, so a fit is reproducible
to the bit.  The match classes predict through the projection kernels.

`match_keypoints` and `KeypointMatcher.build_matches` match the keypoint descriptors of image pairs on the GPU
(`glh_match_knn2`): for every descriptor the two nearest of the other image by exact brute force, equal distances going to
the lower index.  uint8 descriptors (SIFT) are compared in exact integers on the int8 matrix cores, anything else in
float32 summed in element order; both are restated bit for bit in NumPy (tests/matcher_restated.py).  This is the exact
answer that the reference's default matcher, the approximate and unseeded `cv2.FlannBasedMatcher`, approximates: it is
pinned to the stated rule, not to FLANN's output.  The descriptors of an image are uploaded once per `build_matches` call
and stay on the device until the last pair that needs them.

`detect_keypoints(array, method=optimize.SIFT)` and `KeypointMatcher.build_keypoints(method=optimize.SIFT)` detect and
describe SIFT keypoints on the GPU (`glh_sift_detect`): Lowe 2004 with the structure and constants of OpenCV's
implementation, pinned to the rule written out in INPUTS.md ("SIFT: the rule") and to its NumPy restatement
(tests/sift_restated.py) in every bit, not to OpenCV's bytes.  The descriptors are uint8, so they take the matcher's integer
path.  The reference's default `method` (`cv2.SIFT`) is still refused: `cv2` is not a dependency.

`CLAHE(...).apply(array)` and `KeypointMatcher(images, clahe=optimize.CLAHE(...))` equalise an 8-bit image's contrast
tile by tile on the GPU (`glh_stage_clahe`) before detection, which is what finds keypoints on snow and ice: OpenCV's CLAHE
for 8-bit input, pinned to the rule written out in INPUTS.md ("CLAHE: the rule") and to its NumPy restatement
(tests/clahe_restated.py) in every bit.  The matcher hands the stage the image's channels, and their mean is formed on the
device.  The reference's own forms (`clahe=True`, a `dict` for `cv2.createCLAHE`) are still refused.

`ransac(model, ..., batched=True)` over a `Cameras` model with one fitted camera runs Random Sample Consensus with the loop
over the samples on the GPU (`glh_calib_fit_sets`): one call fits every sample by a damped Gauss-Newton, one workgroup per
sample, and scores every row under every fit; a second call refits every distinct consensus set.  The device only decides
which set wins: the values returned come from `Cameras.fit` on that set, as on the host path (`batched=False`, the
reference's loop, unchanged).  Point and match controls are served; everything else is refused, not run on the host
(INPUTS.md, "Camera calibration").

`ransac_pairs(pairs, ...)` and `KeypointMatcher.ransac_matches(...)` run that RANSAC over every image pair of a sequence in
one device pass (`glh_calib_ransac_groups`): each pair's second (or first) camera fitted from its own vector, the other
held, every hypothesis of every pair fitted, scored over its pair's rows and refitted where accepted, the winner and the
final inliers chosen on the device.  The values returned are the device's refit values, not SciPy's (INPUTS.md).

Not served: `cv2.SIFT` itself (the default `method` of `detect_keypoints` and `build_keypoints`), `cv2.createCLAHE` (`clahe=True`
or a `dict`), a `mask` for the GPU matcher, the lmfit methods other than "least_squares" (lmfit is not a dependency) and
plotting.
"""
import collections
import datetime
import math
import sys
from pathlib import Path

import numpy as np

from . import _lib, helpers
from .camera import Camera, rotations

_NO_MATCHER = ("keypoint detection and matching (SIFT and FLANN of cv2) are not served: pass the matches to "
               "ObserverCameras(observer, matches=...)")


_NO_PLOT = "plotting is out of scope"
_NO_DETECT = ("keypoint detection (SIFT of cv2) is not served: give KeypointMatcher.keypoints, or a directory of "
              "keypoint files, as (points, descriptors) per image, or pass method=optimize.SIFT (SIFT on the GPU)")
_NO_CLAHE = ("CLAHE by cv2.createCLAHE (clahe=True or a dict of its arguments) is not served: pass clahe=False, or an "
             "optimize.CLAHE(clipLimit=..., tileGridSize=...) (CLAHE on the GPU)")
_NO_MASK = ("a knnMatch mask is not served by the GPU matcher (the reference's own code cannot index the short lists "
            "cv2 returns for one): pass mask=None, or a matcher object of your own")


class Points:
    """optimize.py:46-236: image-world point correspondences of one camera: world coordinates `xyz` (n, 3) (ray directions
    if `directions`; the camera must not move then) whose projections should be the image coordinates `uv` (n, 2)."""

    def __init__(self, cam, uv, xyz, directions=False):
        if len(uv) != len(xyz):
            raise ValueError("Image and world coordinates have different length")
        self.cam = cam
        self.uv = np.asarray(uv, dtype=float)
        self.xyz = np.asarray(xyz, dtype=float)
        self.directions = directions
        self._position = cam.xyz.copy()
        self._imgsz = cam.imgsz.copy()

    @property
    def size(self):
        return len(self.uv)

    def observed(self, index=slice(None)):
        return self.uv[index]

    def _test_position(self):
        if self.directions and any(self.cam.xyz != self._position):
            raise ValueError("Camera position has changed and world coordinates are ray directions")

    def predicted(self, index=slice(None)):
        """Image coordinates of the world coordinates (the projection kernel)."""
        self._test_position()
        return self.cam.xyz_to_uv(self.xyz[index], directions=self.directions)

    def plot(self, *args, **kwargs):
        raise NotImplementedError(_NO_PLOT)

    def _scale(self, scale):
        if np.any(scale != 1):
            self.uv = self.uv * scale

    def resize(self, size=None, force=False):
        """optimize.py:202-236: resize the camera (unless `size` is None) and scale the image coordinates to it."""
        if size is not None:
            self.cam.resize(size=size, force=force)
        self._scale(self.cam.imgsz / self._imgsz)
        self._imgsz = self.cam.imgsz.copy()


def _clip_box(cam):
    """The box of camera coordinates that holds the image: Lines._xyzs_to_uvs (optimize.py:328-330)."""
    xy_edges = cam._uv_to_xy(cam.edges(step=cam.imgsz / 2))
    return np.hstack((np.min(xy_edges, axis=0), np.max(xy_edges, axis=0)))


def segment_table(cam, xyzs, directions=False, density=1, xy_box=None):
    """What `glh_calib_eval` takes of a Lines job: the world polylines `xyzs` projected into camera coordinates, split at
    vertices behind the camera, clipped to `xy_box` (default: the camera's own, `_clip_box`) and measured -- the vertex
    half of Lines._xyzs_to_uvs (optimize.py:320-353); the pixel half (a point every 1 / density pixels along each clipped
    segment, distorted) is the device's.  Returns (seg_vertex (S + 1,), seg_count (S,), seg_par (S, 5), vertex (V, 3)):
    segment s has vertices seg_vertex[s] .. seg_vertex[s + 1] of `vertex` (x, y, cumulative distance) and seg_count[s]
    points (helpers.interpolate_line's count; a segment whose count rounds to 0 is left out) at the distances
    np.linspace(start, stop, count), of which seg_par[s] = (start, stop, step, stop - start, count - 1).  With no line in
    frame, every vertex in front of the camera is a segment of one point (the reference's fallback)."""
    xy_step = (1 / density) / cam.f.max()
    if xy_box is None:
        xy_box = _clip_box(cam)
    segments, inlines, clipped = [], [], False
    for xyz in xyzs:
        xy = cam._xyz_to_xy(xyz, directions=directions)
        for line in helpers.boolean_split(xy, np.isnan(xy[:, 0]), include="false"):
            inlines.append(line)
            for cline in helpers.clip_polyline_box(line, xy_box):
                clipped = True
                cline = np.array(cline)
                x = helpers.line_distances(cline)
                n = helpers.line_count(x, xy_step)
                if n > 0:
                    segments.append((cline, x, n))
    if not clipped:
        segments = [(line[k:k + 1], np.zeros(1), 1) for line in inlines for k in range(len(line))]
    if not segments:
        raise ValueError("No world line vertices project into the image or in front of the camera")
    seg_vertex = np.concatenate(([0], np.cumsum([len(v) for v, _, _ in segments]))).astype(np.int64)
    seg_count = np.array([n for _, _, n in segments], dtype=np.int64)
    seg_par = np.empty((len(segments), 5))
    for s, (_, x, n) in enumerate(segments):
        delta = x[-1] - x[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            seg_par[s] = (x[0], x[-1], delta / (n - 1) if n > 1 else np.nan, delta, n - 1)
    vertex = np.vstack([np.column_stack((v, x)) for v, x, _ in segments])
    return seg_vertex, seg_count, seg_par, vertex


class Lines(Points):
    """optimize.py:239-459: image-world line correspondences of one camera.  The image polylines `uvs` are merged into
    the points `uv`; the world polylines `xyzs` are projected onto the image at `density` points per pixel, and each image
    point is matched to the nearest projected point.  `predicted` runs on the GPU (`glh_calib_eval` with one job) from the
    segment table the host makes (`segment_table`).  A camera with an elevation correction is not served (the host half
    of the projection, `Camera._xyz_to_xy`, has none) unless `directions`."""

    def __init__(self, cam, uvs, xyzs, directions=False, density=1):
        self.cam = cam
        self.uvs = [np.asarray(uv, dtype=float) for uv in uvs]
        self.uv = np.vstack(self.uvs)
        self.xyzs = xyzs
        self.directions = directions
        self.density = density
        self._position = cam.xyz.copy()
        self._imgsz = cam.imgsz.copy()
        self._boxes = {}  # the camera's internal parameters -> its clip box (a device call)

    def _xy_box(self):
        key = self.cam._vector[6:].tobytes()
        if key not in self._boxes:
            if len(self._boxes) >= 64:
                self._boxes.clear()
            self._boxes[key] = _clip_box(self.cam)
        return self._boxes[key]

    def _segment_table(self):
        return segment_table(self.cam, self.xyzs, directions=self.directions, density=self.density, xy_box=self._xy_box())

    def _xyzs_to_uvs(self):
        """optimize.py:320-353 on the host: the projected world lines as image coordinates [(ni, 2), ...], one array per
        clipped segment (per line in front of the camera when none is in frame)."""
        xy_step = (1 / self.density) / self.cam.f.max()
        xy_box = self._xy_box()
        puvs, inlines = [], []
        for xyz in self.xyzs:
            xy = self.cam._xyz_to_xy(xyz, directions=self.directions)
            for line in helpers.boolean_split(xy, np.isnan(xy[:, 0]), include="false"):
                inlines.append(line)
                for cline in helpers.clip_polyline_box(line, xy_box):
                    puvs.append(self.cam._xy_to_uv(helpers.interpolate_line(np.array(cline), dx=xy_step)))
        if puvs:
            return puvs
        return [self.cam._xy_to_uv(line) for line in inlines]

    def predicted(self, index=slice(None)):
        """For each observed point (of `index`), the nearest point of the projected world lines."""
        self._test_position()
        observed = np.ascontiguousarray(self.observed(index=index))
        if not len(observed):
            return np.empty((0, 2))
        table = self._segment_table()
        with _lib.Calib(1, [_lib.CALIB_KINDS["lines"]], [0], [0], [int(bool(self.directions))], [0, len(observed)], observed,
                        np.zeros((len(observed), 3))) as handle:
            return handle.eval(self.cam.vector24[None, None], self.cam.R[None, None], [0], [0], tables=[table])

    def _scale(self, scale):
        if np.any(scale != 1):
            for i, uv in enumerate(self.uvs):
                self.uvs[i] = uv * scale
            self.uv *= scale


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
        raise NotImplementedError(_NO_PLOT)

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


KeyPoint = collections.namedtuple("KeyPoint", "pt size angle response octave class_id")  # the fields of a cv2.KeyPoint


class SIFT:
    """SIFT on the GPU, shaped like a cv2.Feature2D: `SIFT.create(...).detectAndCompute(array, mask=None)`.  The rule is
    INPUTS.md's "SIFT: the rule".  Keypoints are `KeyPoint`s with float64 fields, descriptors uint8 (n, 128) (cv2 stores the
    same integers as float32); an image too small for an octave gives ([], None)."""

    def __init__(self, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6, device_id=0):
        self.nfeatures = int(nfeatures)
        self.nOctaveLayers = int(nOctaveLayers)
        self.contrastThreshold = float(contrastThreshold)
        self.edgeThreshold = float(edgeThreshold)
        self.sigma = float(sigma)
        self.device_id = int(device_id)
        self._handle = None

    @classmethod
    def create(cls, nfeatures=0, nOctaveLayers=3, contrastThreshold=0.04, edgeThreshold=10, sigma=1.6):
        return cls(nfeatures, nOctaveLayers, contrastThreshold, edgeThreshold, sigma)

    def detect_arrays(self, array, mask=None):
        """(keypoints float64 (n, 6): pt x, pt y, size, angle, response, octave; descriptors uint8 (n, 128)) after the
        host-side steps, or (None, None) when the image holds no octave."""
        array = np.asarray(array)
        if array.ndim != 2:
            raise NotImplementedError("SIFT takes a two-dimensional array: cv2 would weigh the channels of a colour image "
                                      "as BGR; KeypointMatcher.build_keypoints takes their mean first")
        array = np.asarray(array, dtype=np.uint8)
        if min(array.shape) < 6:  # the doubled image has no octave of 12 cells a side
            return None, None
        if self._handle is None:
            self._handle = _lib.Sift(self.device_id)
        kps, desc = self._handle.detect(array, self.nOctaveLayers, self.contrastThreshold, self.edgeThreshold, self.sigma)
        keep = np.ones(len(kps), bool)
        if len(kps) > 1:  # a keypoint equal to its predecessor in pt, size and angle is dropped
            keep[1:] = np.any(kps[1:, :4] != kps[:-1, :4], axis=1)
        if mask is not None:
            mask = np.asarray(mask, dtype=np.uint8)
            v, u = (kps[:, 1] + 0.5).astype(np.int64), (kps[:, 0] + 0.5).astype(np.int64)
            inside = (v >= 0) & (v < mask.shape[0]) & (u >= 0) & (u < mask.shape[1])
            keep &= inside
            keep[inside] &= mask[v[inside], u[inside]] != 0
        kps, desc = kps[keep], desc[keep]
        if self.nfeatures > 0 and len(kps) > self.nfeatures:  # the largest responses, ties to the earlier, order kept
            order = np.sort(np.argsort(-kps[:, 4], kind="stable")[:self.nfeatures])
            kps, desc = kps[order], desc[order]
        return kps, desc

    def close(self):
        """Frees the device handle and its pyramid (a later call makes a new one)."""
        if self._handle is not None:
            handle, self._handle = self._handle, None
            handle.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def detectAndCompute(self, array, mask=None):
        kps, desc = self.detect_arrays(array, mask)
        if kps is None:
            return [], None
        keypoints = [KeyPoint((row[0], row[1]), row[2], row[3], row[4], int(row[5]), -1) for row in kps.tolist()]
        return keypoints, desc


class CLAHE:
    """Contrast-limited adaptive histogram equalisation on the GPU, shaped like a cv2.CLAHE: `CLAHE(clipLimit,
    tileGridSize).apply(array)` of a two-dimensional uint8 array.  The rule is INPUTS.md's "CLAHE: the rule".
    `tileGridSize` is (tilesX, tilesY); a `clipLimit` of 0 or less does not clip.  It holds no device handle: it pickles and
    copies as the three numbers it is."""

    def __init__(self, clipLimit=40.0, tileGridSize=(8, 8), device_id=0):
        self.setClipLimit(clipLimit)
        self.setTilesGridSize(tileGridSize)
        self.device_id = int(device_id)

    def getClipLimit(self):
        return self.clipLimit

    def setClipLimit(self, clipLimit):
        clipLimit = float(clipLimit)
        if not math.isfinite(clipLimit):
            raise ValueError(f"clipLimit {clipLimit} is not finite")
        self.clipLimit = clipLimit

    def getTilesGridSize(self):
        return self.tileGridSize

    def setTilesGridSize(self, tileGridSize):
        grid = tuple(tileGridSize)
        if len(grid) != 2 or any(int(t) != t or t < 1 for t in grid):
            raise ValueError(f"tileGridSize {tileGridSize!r}: (tilesX, tilesY), whole numbers of at least 1")
        self.tileGridSize = (int(grid[0]), int(grid[1]))

    def collectGarbage(self):
        """cv2's frees its buffers; nothing is kept here between calls."""

    def _stage(self, array):
        """`array` uint8 (h, w) or (h, w, c <= 4) -> uint8 (h, w): the channel mean and the rule, one stage call."""
        h, w = array.shape[:2]
        tiles_x, tiles_y = self.tileGridSize
        if tiles_x > w or tiles_y > h:
            raise ValueError(f"a grid of {tiles_x} x {tiles_y} tiles is larger than the image of {w} x {h} pixels")
        return _lib.stage_clahe(array, self.clipLimit, self.tileGridSize, device_id=self.device_id)

    def apply(self, array):
        if not isinstance(array, np.ndarray) or array.dtype != np.uint8:
            what = array.dtype if isinstance(array, np.ndarray) else type(array).__name__
            raise TypeError(f"CLAHE.apply takes a two-dimensional uint8 array (got {what}): 16-bit CLAHE is not served")
        if array.ndim != 2 or array.size == 0:
            raise ValueError(f"CLAHE.apply takes a two-dimensional uint8 array that is not empty (got shape {array.shape})")
        return self._stage(array)


def createCLAHE(clipLimit=40.0, tileGridSize=(8, 8)):
    """An `optimize.CLAHE`, as cv2.createCLAHE makes a cv2.CLAHE."""
    return CLAHE(clipLimit, tileGridSize)


def detect_keypoints(array, mask=None, method=None, root=False, **kwargs):
    """optimize.py:2194-2231 with `method=optimize.SIFT` (SIFT on the GPU; `kwargs` go to `SIFT.create`).  The reference's
    default method, cv2.SIFT (`method=None` here), is not served, nor is any other."""
    with _create_detector(method, kwargs) as detector:
        return _detect(detector, array, mask, root)


def _create_detector(method, kwargs):
    if method is None:
        raise NotImplementedError(_NO_DETECT)
    if method is not SIFT:
        raise NotImplementedError(f"method {method!r} is not served: optimize.SIFT is")
    return method.create(**kwargs)


def _detect(detector, array, mask, root):
    """What `detect_keypoints` returns, from a detector that is already made (`build_keypoints` keeps one for all its
    images, so that frames of one size share the pyramid's device memory)."""
    keypoints, descriptors = detector.detectAndCompute(array, mask=mask)
    # Empty result: ([], None)
    if root and descriptors is not None:
        descriptors = descriptors.astype(np.float32)  # (what cv2 returns)
        descriptors = np.sqrt(descriptors / (descriptors.sum(axis=1, keepdims=True) + 1e-7))
    return keypoints, descriptors


DMatch = collections.namedtuple("DMatch", "queryIdx trainIdx distance")  # what the logic below reads of a cv2.DMatch


def _point(keypoint):
    """(u, v) of a keypoint: a row of an (n, 2) array, or an object with `.pt` (cv2.KeyPoint)."""
    return keypoint.pt if hasattr(keypoint, "pt") else keypoint


def _device_knn(handle, slots, descriptors, k):
    """[[DMatch] * k] for every row of `descriptors[0]` among `descriptors[1]`, which `handle` (a `_lib.Matcher`) holds or
    will hold under `slots`: the distance is np.sqrt of the float32 squared distance, as a Python float (cv2's is one).
    Sets that took different paths are searched on the float path."""
    for slot, d in zip(slots, descriptors):
        if handle.path(slot) is None:
            handle.put(slot, d)
    paths = [handle.path(slot) for slot in slots]
    if paths[0] != paths[1]:
        for slot, d, path in zip(slots, descriptors, paths):
            if path == "integer":
                handle.put(slot, d, path="float")
    idx, d2 = handle.knn2(slots[0], slots[1])
    distance = np.sqrt(d2).tolist()
    idx = idx.tolist()
    return [[DMatch(q, idx[q][r], distance[q][r]) for r in range(k)] for q in range(len(idx))]


def _match_keypoints(ka, kb, knn, cross_check, max_ratio, max_distance, return_ratios):
    """optimize.py:2270-2309 after the matcher: `knn(False)` is knnMatch(ka, kb), `knn(True)` knnMatch(kb, ka)."""
    def _build_empty(return_ratios):
        empty = np.array([], dtype=float).reshape(0, 2)
        uva, uvb = empty, empty.copy()
        ratios = np.array([], dtype=float)
        if return_ratios:
            return uva, uvb, ratios
        return uva, uvb

    compute_ratios = max_ratio or return_ratios
    n = 2 if compute_ratios else 1
    if len(ka[0]) >= n and len(kb[0]) >= n:
        matches = knn(False)
        if cross_check:
            matches_ba = knn(True)
            ba = {(m[0].trainIdx, m[0].queryIdx) for m in matches_ba}  # (a list in the reference: the same members)
            matches = [m for m in matches if (m[0].queryIdx, m[0].trainIdx) in ba]
        if max_ratio:
            matches = [m for m in matches if m[0].distance / m[1].distance < max_ratio]
        if not matches:
            return _build_empty(return_ratios)
        uva = np.asarray([_point(ka[0][m[0].queryIdx]) for m in matches])
        uvb = np.asarray([_point(kb[0][m[0].trainIdx]) for m in matches])
        if return_ratios:
            ratios = np.array([m.distance / n.distance for m, n in matches])
        if max_distance:
            valid = np.linalg.norm(uva - uvb, axis=1) < max_distance
            uva, uvb = uva[valid], uvb[valid]
            if return_ratios:
                ratios = ratios[valid]
    else:
        return _build_empty(return_ratios)
    if return_ratios:
        return uva, uvb, ratios
    return uva, uvb


def match_keypoints(ka, kb, mask=None, cross_check=False, max_ratio=None, max_distance=None, return_ratios=False,
                    matcher=None, device_id=0, resident=None):
    """optimize.py:2234-2309: the image coordinates (n, 2), (n, 2) of the matched keypoints of two images, and with
    `return_ratios` the ratio (n,) of the best to the second best descriptor distance of each.  A keypoint set is
    (points, descriptors): `points` an (n, 2) array or a sequence of objects with `.pt`, `descriptors` (n, dim).

    With `matcher=None` the nearest neighbours are searched on the GPU (`_lib.Matcher`): the exact two nearest by
    brute force, equal distances going to the lower index -- the exact answer that the reference's default, the
    approximate and unseeded cv2.FlannBasedMatcher, approximates; pinned to that rule, not to FLANN's output.  The
    distance is np.sqrt of the float32 squared distance.  `cross_check` runs the same search the other way round.  The
    reference's logic follows unchanged: cross-check, then the ratio test (<), then `max_distance` (<); the ratios are
    quotients of Python floats, so a second best distance of 0 raises ZeroDivisionError as it does there.  `mask` with
    the GPU matcher raises NotImplementedError.

    Any other `matcher` with knnMatch(query, train, k=, mask=) is used on the host exactly as the reference uses it.

    Two parameters beyond the reference's, for the GPU matcher only: `device_id`, the device a search of its own runs
    on; `resident` = (a `_lib.Matcher`, (slot of ka, slot of kb)), a handle of the caller's that holds, or will hold,
    the two descriptor sets under those slots and stays open (what `KeypointMatcher.build_matches` passes)."""
    if mask is not None:
        mask = np.asarray(mask, dtype=np.uint8)
    n = 2 if (max_ratio or return_ratios) else 1
    if matcher is not None:
        def knn(swap):
            q, t = (kb[1], ka[1]) if swap else (ka[1], kb[1])
            return matcher.knnMatch(q, t, k=n, mask=mask)
        return _match_keypoints(ka, kb, knn, cross_check, max_ratio, max_distance, return_ratios)
    if mask is not None:
        raise NotImplementedError(_NO_MASK)
    handle, slots = resident if resident is not None else (None, (0, 1))
    own = handle is None
    if own and len(ka[0]) >= n and len(kb[0]) >= n:
        handle = _lib.Matcher(device_id=device_id)
    try:
        def knn(swap):
            order = (1, 0) if swap else (0, 1)
            return _device_knn(handle, [slots[o] for o in order], [(ka[1], kb[1])[o] for o in order], n)
        return _match_keypoints(ka, kb, knn, cross_check, max_ratio, max_distance, return_ratios)
    finally:
        if own and handle is not None:
            handle.close()


class PairMatches:
    """The matches of image pairs as `KeypointMatcher.matches` keeps them: `data` (an object array of `Matches`), `row`
    and `col` (the images of each) and `shape` (n, n) -- the attributes of the scipy.sparse.coo_matrix the reference
    builds, which the installed SciPy cannot build of objects (INPUTS.md).  `match_pairs` reads it."""

    def __init__(self, data, row, col, shape):
        self.data = np.empty(len(data), dtype=object)
        for k, m in enumerate(data):
            self.data[k] = m
        self.row, self.col = np.asarray(row, dtype=int), np.asarray(col, dtype=int)
        self.shape = tuple(shape)

    def eliminate_zeros(self):
        """scipy's: drops the entries whose data is False / 0."""
        keep = np.array([not (isinstance(m, (bool, int, float)) and m == 0) for m in self.data], dtype=bool)
        self.data, self.row, self.col = self.data[keep], self.row[keep], self.col[keep]


class KeypointMatcher:
    """optimize.py:2312-2773: matches the keypoints of `images` (in ascending temporal order) pair by pair, on the GPU
    (`build_matches`).  `keypoints`: per image (points, descriptors) as `match_keypoints` takes them; they are passed in
    or read from files, or detected with `build_keypoints(method=optimize.SIFT)`.  `clahe`: False, or an `optimize.CLAHE`,
    which `build_keypoints` applies to every image before it detects; True and a dict (cv2.createCLAHE) are not served."""

    def __init__(self, images=None, clahe=False):
        if images is None:
            raise NotImplementedError(_NO_MATCHER)
        dts = np.diff([img.datetime for img in images])
        if np.any(dts < datetime.timedelta(0)):
            raise ValueError("Images are not in ascending temporal order")
        self.images = np.empty(len(images), dtype=object)
        for i, img in enumerate(images):
            self.images[i] = img
        if clahe is False:
            self.clahe = None
        elif isinstance(clahe, CLAHE):
            self.clahe = clahe
        else:
            raise NotImplementedError(_NO_CLAHE)
        self.device_id = 0
        self.keypoints = None
        self.matches = None

    def _prepare_image_basenames(self):
        basenames = [helpers.strip_path(img.path) for img in self.images]
        if len(basenames) != len(set(basenames)):
            raise ValueError("Image basenames are not unique")
        return basenames

    def _prepare_image(self, array):
        """optimize.py:2358-2365: the channel mean, then uint8, then CLAHE if the matcher has one.  A uint8 image of up to
        four channels goes to the CLAHE stage as it is: the stage forms the same mean on the device."""
        if self.clahe is not None and array.dtype == np.uint8 and (
                array.ndim == 2 or (array.ndim == 3 and 1 <= array.shape[2] <= 4)):
            return self.clahe._stage(array)
        if array.ndim > 2:
            array = array.mean(axis=2)
        array = array.astype(np.uint8, copy=False)
        if self.clahe is not None:
            array = self.clahe.apply(array)
        return array

    def build_keypoints(self, masks=None, path=None, overwrite=False, clear_images=True, clear_keypoints=False,
                        parallel=False, **kwargs):
        """optimize.py:2367-2445: the reading, writing and cached branches (`basename.pkl` under `path`), and with
        `method=optimize.SIFT` in `kwargs` the detecting branch (`detect_keypoints` on the channel mean as uint8, `masks`
        one array for all images or one per image).  Without it an image whose keypoints would have to be detected raises
        NotImplementedError.  `parallel` is accepted and ignored."""
        if path:
            path = Path(path)
        if clear_keypoints and not path:
            raise ValueError("path is required when clear_keypoints is True")
        if path and path.is_file():
            raise ValueError("path must be a directory")
        basenames = self._prepare_image_basenames()
        if masks is None or isinstance(masks, np.ndarray):
            masks = [masks] * len(self.images)
        if not self.keypoints:
            self.keypoints = [None] * len(self.images)
        result = []
        detector = None  # made for the first image that has to be detected, kept until the last
        try:
            for i, img in enumerate(self.images):
                print(img.path)
                if path:
                    outpath = path / f"{basenames[i]}.pkl"
                    written = outpath.exists()
                else:
                    written = False
                keypoints = self.keypoints[i]
                read = keypoints is not None
                if not read and written and not clear_keypoints:
                    keypoints = helpers.read_pickle(outpath)
                elif read and not written and path:
                    helpers.write_pickle(keypoints, path=outpath)
                elif (not read and not written) or overwrite:
                    if kwargs.get("method") is None:
                        raise NotImplementedError(_NO_DETECT)
                    if detector is None:
                        create = {k: v for k, v in kwargs.items() if k not in ("method", "root")}
                        detector = _create_detector(kwargs["method"], create)
                    array = self._prepare_image(img.read())
                    keypoints = _detect(detector, array, masks[i], kwargs.get("root", False))
                    if path:
                        helpers.write_pickle(keypoints, path=outpath)
                    if clear_images:
                        img.array = None
                if clear_keypoints:
                    keypoints = None
                result.append(keypoints)
        finally:
            if detector is not None:
                detector.close()
        self.keypoints = result

    def _matching_images(self, maxdt=None, seq=None, imgs=None):
        """optimize.py:2513-2537: for every image the later images it is matched with."""
        n = len(self.images)
        if maxdt is None and seq is None:
            matching_images = [np.arange(i + 1, n) for i in range(n)]
        elif maxdt is not None:
            datetimes = np.array([img.datetime for img in self.images])
            ends = np.searchsorted(datetimes, datetimes + maxdt, side="right")
            matching_images = [np.arange(i + 1, end) for i, end in enumerate(ends)]
        elif seq is not None:
            matching_images = [np.array([], dtype=int) for i in range(n)]
        if seq is not None:
            seq = np.asarray(seq)
            seq = np.unique(seq[seq > 0])
            for i, m in enumerate(matching_images):
                iseq = seq + i
                iseq = iseq[: np.searchsorted(iseq, n)]
                matching_images[i] = np.unique(np.concatenate((m, iseq)))
        if imgs is not None:
            for i, m in enumerate(matching_images):
                if i in imgs:
                    matching_images[i] = m
                else:
                    matching_images[i] = m[np.isin(m, imgs)]
        return matching_images

    def build_matches(self, maxdt=None, seq=None, imgs=None, keypoints_path=None, path=None, overwrite=False,
                      clear_keypoints=True, clear_matches=False, parallel=False, weights=False, mtype=None, filter=None,
                      **kwargs):
        """optimize.py:2447-2622, every argument as there: the pairs (i, j > i) named by `maxdt`, `seq` and `imgs` are
        matched with `match_keypoints(**kwargs)`, read from and written to `basenames[i]-basenames[j].pkl` under `path`,
        and kept in `self.matches` (a `PairMatches`) unless `clear_matches`.  `parallel` is accepted and ignored: the
        GPU is the parallelism.  One `_lib.Matcher` serves the whole call: the descriptors of an image are uploaded when
        the first pair needs them and dropped after the last row that does."""
        if path:
            path = Path(path)
        if keypoints_path:
            keypoints_path = Path(keypoints_path)
        if clear_matches and not path:
            raise ValueError("path is required when clear_matches is True")
        if path and path.is_file():
            raise ValueError("path must be a directory")
        kwargs = {**kwargs, **{"return_ratios": weights}}
        basenames = self._prepare_image_basenames()
        if self.keypoints is None:
            self.keypoints = [None] * len(self.images)
        if any(k is None for k in self.keypoints) and not keypoints_path:
            raise ValueError("Missing keypoints so keypoints_path is required")
        matching_images = self._matching_images(maxdt=maxdt, seq=seq, imgs=imgs)
        last_row = {}  # image -> the last row that searches its descriptors
        for i, js in enumerate(matching_images):
            for j in js:
                last_row[int(j)] = i
            if len(js):
                last_row[i] = max(last_row.get(i, i), i)
        on_device = kwargs.get("matcher") is None and kwargs.get("mask") is None
        handle = None  # (opened when the first pair has to be searched: cached pairs need no device)
        matches = []
        try:
            for i, js in enumerate(matching_images):
                if len(js) > 0:
                    print("Matching", i, "->", ", ".join(js.astype(str)))
                row = []
                imgA = self.images[i]
                if self.keypoints[i] is None:
                    self.keypoints[i] = helpers.read_pickle(keypoints_path / f"{basenames[i]}.pkl")
                for j in js:
                    imgB = self.images[j]
                    if self.keypoints[j] is None:
                        self.keypoints[j] = helpers.read_pickle(keypoints_path / f"{basenames[j]}.pkl")
                    if path:
                        outfile = path / f"{basenames[i]}-{basenames[j]}.pkl"
                    if path and not overwrite and outfile.exists():
                        if not clear_matches:
                            match = helpers.read_pickle(outfile)
                            match.cams = (imgA.cam, imgB.cam)  # (the cameras of this sequence, not the file's copies)
                            if mtype is not None:
                                match = match.to_type(mtype)
                            row.append(match)
                    else:
                        if on_device and handle is None:
                            handle = _lib.Matcher(device_id=self.device_id)
                        resident = (handle, (i, int(j))) if on_device else None
                        result = match_keypoints(self.keypoints[i], self.keypoints[j], resident=resident, **kwargs)
                        match = Matches(cams=(imgA.cam, imgB.cam), uvs=result[0:2],
                                        weights=(1 / result[2]) if weights else None)
                        if path is not None:
                            helpers.write_pickle(match, outfile)
                        if not clear_matches:
                            if mtype is not None:
                                match = match.to_type(mtype)
                            row.append(match)
                if clear_keypoints:
                    self.keypoints[i] = None
                if handle is not None:
                    for slot in handle.slots():
                        if last_row.get(slot, -1) <= i:
                            handle.drop(slot)
                if filter and not clear_matches:
                    for match in row:
                        if match:
                            match.filter(**filter)
                matches.append(row)
        finally:
            if handle is not None:
                handle.close()
        if clear_matches:
            self.matches = None
            return
        rows = np.concatenate([np.asarray([i] * len(row), dtype=int) for i, row in enumerate(matching_images)])
        cols = np.concatenate(matching_images)
        # (the shape scipy.sparse.coo_matrix infers from the indices, as the reference's does; (0, 0) without a pair, where
        # the reference's constructor fails)
        shape = (int(rows.max()) + 1, int(cols.max()) + 1) if len(rows) else (0, 0)
        self.matches = PairMatches([m for row in matches for m in row], rows, cols, shape)

    def _test_matches(self):
        if self.matches is None:
            raise ValueError("Matches have not been initialized. Run build_matches()")

    def _assign_cameras(self):
        for m, i, j in zip(self.matches.data, self.matches.row, self.matches.col):
            m.cams = self.images[i].cam, self.images[j].cam

    def convert_matches(self, mtype, clear_uvs=False, parallel=False):
        """optimize.py:2634-2671 (`parallel` is accepted and ignored)."""
        self._test_matches()
        for i, m in enumerate(self.matches.data):
            m = m.to_type(mtype)
            if clear_uvs and mtype in (RotationMatchesXY, RotationMatchesXYZ):
                m.uvs = None
            self.matches.data[i] = m

    def filter_matches(self, clear_weights=False, parallel=False, **kwargs):
        """optimize.py:2673-2707 (`parallel` is accepted and ignored)."""
        self._test_matches()
        for i, m in enumerate(self.matches.data):
            if kwargs:
                m.filter(**kwargs)
            if clear_weights:
                m.weights = None
            self.matches.data[i] = m

    def ransac_matches(self, n, max_error, min_inliers, iterations=100, cam_params=None, samples=None, seed=None, **kwargs):
        """Frees every pair's matches of outliers by `ransac_pairs` over `self.matches` (all pairs in one device pass; the
        arguments are its own): a pair keeps its inliers -- `uvs`, `xys` and `weights` filtered together, as
        `Matches.filter` does -- and a pair for which no fit is accepted is emptied to size 0 and stays in place, so that
        `matches_per_image`, `images_per_image` and `match_breaks(min_matches)` report it.  `samples="device"` (and `seed`)
        draws the samples on the device as well, which is what a long sequence wants.  Returns the inlier count per pair, -1
        for a rejected pair."""
        self._test_matches()
        results = ransac_pairs(self.matches, n, max_error, min_inliers, iterations=iterations, cam_params=cam_params,
                               samples=samples, seed=seed, **kwargs)
        counts = np.full(len(results), -1, dtype=int)
        for k, (m, result) in enumerate(zip(self.matches.data, results)):
            selected = np.zeros(m.size, dtype=bool)
            if result is not None:
                selected[result[1]] = True
                counts[k] = len(result[1])
            if m.uvs:
                m.uvs = [uv[selected] for uv in m.uvs]
            if getattr(m, "xys", None):
                m.xys = [xy[selected] for xy in m.xys]
            if m.weights is not None:
                m.weights = np.asarray(m.weights)[selected]
        return counts

    def _images_mask(self, imgs):
        if np.iterable(imgs):
            return np.isin(self.matches.row, imgs) | np.isin(self.matches.col, imgs)
        return (self.matches.row == imgs) | (self.matches.col == imgs)

    def _images_matches(self, imgs):
        return self.matches.data[self._images_mask(imgs)]

    def matches_per_image(self):
        """optimize.py:2720-2727: the matched points of every image."""
        self._test_matches()
        image_matches = [self._images_matches(i) for i in range(len(self.images))]
        return np.array([np.sum([mi.size for mi in m]) for m in image_matches])

    def images_per_image(self):
        """optimize.py:2729-2733: the images every image has matches with."""
        self._test_matches()
        image_matches = [self._images_matches(i) for i in range(len(self.images))]
        return np.array([np.sum([mi.size > 0 for mi in m]) for m in image_matches])

    def drop_images(self, imgs):
        """optimize.py:2735-2758: drops the matches of `imgs`, then every image left without a match."""
        self._test_matches()
        mask = self._images_mask(imgs)
        self.matches.data[mask] = False
        self.matches.eliminate_zeros()
        all = np.arange(len(self.images))
        keep = np.union1d(self.matches.row, self.matches.col)
        drop = np.setdiff1d(all, keep)
        _, new_row = np.unique(np.concatenate((self.matches.row, keep)), return_inverse=True)
        self.matches.row = new_row[: -len(keep)]
        _, new_col = np.unique(np.concatenate((self.matches.col, keep)), return_inverse=True)
        self.matches.col = new_col[: -len(keep)]
        n = len(self.images) - len(drop)
        self.matches.shape = (n, n)
        self.images = np.delete(self.images, drop)

    def match_breaks(self, min_matches=0):
        """optimize.py:2760-2773: the images after which the chain of pairwise matches breaks."""
        self._test_matches()
        all_starts = np.arange(len(self.images) - 1)
        starts, counts = np.unique(self.matches.row, return_counts=True)
        breaks = np.setdiff1d(all_starts, starts)
        if min_matches:
            min_matches = np.minimum(min_matches, len(self.images) - np.arange(len(self.images)))
            breaks = np.sort(np.concatenate((breaks, np.where(counts < min_matches)[0])))
        return breaks


class Polynomial:
    """optimize.py:985-1130: a least-squares polynomial of degree `deg` through the points `xy` (n, 2), as a model for
    `ransac`."""

    def __init__(self, xy, deg=1):
        self.xy = np.asarray(xy)
        self.deg = deg

    @property
    def size(self):
        return len(self.xy)

    def predict(self, params, index=slice(None)):
        return np.polyval(params, self.xy[index, 0])

    def errors(self, params, index=slice(None)):
        prediction = self.predict(params, index)
        return np.abs(prediction - self.xy[index, 1])

    def fit(self, index=slice(None)):
        return np.polyfit(self.xy[index, 0], self.xy[index, 1], deg=self.deg)

    def plot(self, *args, **kwargs):
        raise NotImplementedError(_NO_PLOT)


_ATTRIBUTES = ("xyz", "viewdir", "imgsz", "f", "c", "k", "p")
_LENGTHS = (3, 3, 2, 2, 2, 6, 2)
_NO_LMFIT = ("lmfit is not installed: only method='least_squares' is served, through scipy.optimize.least_squares "
             "(got method={!r})")


def _kind_of(control):
    if isinstance(control, Lines):
        return _lib.CALIB_KINDS["lines"]
    if isinstance(control, Points):
        return _lib.CALIB_KINDS["points"]
    if isinstance(control, RotationMatchesXYZ):
        raise NotImplementedError("RotationMatchesXYZ has no observed(): it is ObserverCameras' control, not Cameras'")
    if isinstance(control, RotationMatchesXY):
        return _lib.CALIB_KINDS["rotation_xy"]
    if isinstance(control, RotationMatches):
        return _lib.CALIB_KINDS["rotation"]
    if isinstance(control, Matches):
        return _lib.CALIB_KINDS["matches"]
    raise TypeError(f"not a control: {type(control).__name__}")


class Cameras:
    """optimize.py:1133-1971: the parameters of the cameras `cams` that minimise the reprojection errors of the `controls`
    (`Points`, `Lines`, `Matches` and its rotation subclasses).  `cam_params`: per camera, the parameters to fit
    (`parse_params`); `group_params`: per group of cameras (`group_indices`, default one group of all), parameters that
    take one value for the whole group.  `weights`: one per control point.  `scales`: compute a scale factor per
    parameter (`camera_scales`); `sparsity`: compute the sparsity structure of the Jacobian.

    `params` is an ordered mapping label -> (value, min, max), groups first, where the reference keeps lmfit.Parameters."""

    def __init__(self, cams, controls, cam_params=None, group_indices=None, group_params=None, weights=None, scales=True,
                 sparsity=True):
        cams, controls, cam_params, group_indices, group_params = self._as_lists(cams, controls, cam_params, group_indices,
                                                                                 group_params)
        self.cams = cams
        self.controls = self.prune_controls(controls, cams=self.cams)
        ncams = len(self.cams)
        if cam_params is None:
            cam_params = [{}] * ncams
        self.cam_params = cam_params
        if group_indices is None:
            group_indices = [range(ncams)]
        self.group_indices = group_indices
        if group_params is None:
            group_params = [{}] * len(self.group_indices)
        self.group_params = group_params
        self.weights = weights
        self.device_id = 0
        self._handle = None
        self.update_params()
        self._test()
        self.vectors = [cam.to_array() for cam in self.cams]
        self.scales = None
        if scales:
            self._build_scales()
        self.sparsity = None
        if sparsity:
            self._build_sparsity()

    @property
    def weights(self):
        return self._weights

    @weights.setter
    def weights(self, value):
        if value is None:
            self._weights = value
        else:
            value = np.atleast_2d(value).reshape(-1, 1)
            self._weights = value * len(value) / sum(value)

    @staticmethod
    def _as_lists(cams, controls, cam_params, group_indices, group_params):
        if isinstance(cams, Camera):
            cams = [cams]
        if isinstance(controls, (Points, Lines, Matches)):
            controls = [controls]
        if isinstance(cam_params, dict):
            cam_params = [cam_params]
        if isinstance(group_indices, int):
            group_indices = [group_indices]
        if group_indices is not None and isinstance(group_indices[0], int):
            group_indices = [group_indices]
        if isinstance(group_params, dict):
            group_params = [group_params]
        return cams, controls, cam_params, group_indices, group_params

    @staticmethod
    def _lmfit_labels(mask, cam=None, group=None):
        """The labels of the selected parameters: "f0", "viewdir2" ... behind "cam<i>_" or "group<i>_"."""
        base_labels = np.array([attribute + str(i) for attribute, length in zip(_ATTRIBUTES, _LENGTHS) for i in range(length)])
        labels = base_labels[mask]
        if cam is not None:
            labels = ["cam" + str(cam) + "_" + label for label in labels]
        if group is not None:
            labels = ["group" + str(group) + "_" + label for label in labels]
        return labels

    @staticmethod
    def _get_control_cams(control):
        if isinstance(control, (Points, Lines)):
            return [control.cam]
        return control.cams

    @classmethod
    def prune_controls(cls, controls, cams):
        """The controls that reference one or more of `cams`."""
        return [control for control in controls if len(set(cams) & set(cls._get_control_cams(control))) > 0]

    @staticmethod
    def camera_scales(cam, controls=None):
        """optimize.py:1327-1407: per camera parameter (20), the estimated change that moves an image point by a pixel;
        `controls`: world controls of the camera, for the effect of moving it."""
        dpixels = np.ones(20, dtype=float)
        mean_r_uv = (cam.imgsz.mean() / 6) * (np.sqrt(2) + np.log(1 + np.sqrt(2)))
        mean_r_xy = mean_r_uv / cam.f.mean()
        if controls:
            xyz = []
            for control in controls:
                if isinstance(control, (Points, Lines)) and cam is control.cam and not control.directions:
                    if hasattr(control, "xyz"):
                        xyz.append(control.xyz)
                    elif hasattr(control, "xyzs"):
                        xyz.extend(control.xyzs)
            if xyz:
                dpixels[0:3] = cam.f.mean() / np.linalg.norm(np.vstack(xyz) - cam.xyz).mean()
        imgsz_degrees = (2 * np.arctan(cam.imgsz / (2 * cam.f))) * (180 / np.pi)
        dpixels[3:5] = cam.imgsz / imgsz_degrees
        theta = np.pi / 180
        dpixels[5] = 2 * mean_r_uv * np.sin(theta / 2)
        dpixels[6:8] = 0.5
        dpixels[8:10] = mean_r_xy
        dpixels[10:12] = 1
        dpixels[12:18] = [
            mean_r_xy ** 3 * cam.f.mean() * 2 ** (1 / 2),
            mean_r_xy ** 5 * cam.f.mean() * 2 ** (3 / 2),
            mean_r_xy ** 7 * cam.f.mean() * 2 ** (5 / 2),
            mean_r_xy ** 3 / (1 + cam.k[3] * mean_r_xy ** 2) * cam.f.mean() * 2 ** (1 / 2),
            mean_r_xy ** 5 / (1 + cam.k[4] * mean_r_xy ** 4) * cam.f.mean() * 2 ** (3 / 2),
            mean_r_xy ** 7 / (1 + cam.k[5] * mean_r_xy ** 6) * cam.f.mean() * 2 ** (5 / 2),
        ]
        dpixels[18:20] = np.sqrt(5) * mean_r_xy ** 2 * cam.f.mean()
        return 1 / dpixels

    @staticmethod
    def camera_bounds(cam):
        """optimize.py:1410-1456: default bounds (20, 2) of the camera parameters."""
        k = cam.f.mean() / 4000
        p = cam.f.mean() / 40000
        return np.array([
            [-np.inf, np.inf], [-np.inf, np.inf], [-np.inf, np.inf],
            [-np.inf, np.inf], [-np.inf, np.inf], [-np.inf, np.inf],
            [0, np.inf], [0, np.inf],
            [0, np.inf], [0, np.inf],
            [-0.5, 0.5] * cam.imgsz[0:1], [-0.5, 0.5] * cam.imgsz[1:2],
            [-k, k], [-k / 2, k / 2], [-k / 2, k / 2], [-k, k], [-k, k], [-k, k],
            [-p, p], [-p, p],
        ], dtype=float)

    @staticmethod
    def parse_params(params=None, default_bounds=None):
        """optimize.py:1459-1522: (mask (20,), bounds (20, 2)) of `params`: {"viewdir": True}, {"viewdir": 0},
        {"viewdir": [0, 1]}, or with bounds (indices, min, max), min and max one number or one per index; None or NaN take
        `default_bounds`, else -inf / inf."""
        if params is None:
            params = {}
        indices = (0, 3, 6, 8, 10, 12, 18, 20)
        mask = np.zeros(20, dtype=bool)
        bounds = np.full((20, 2), np.nan)
        for key, value in params.items():
            if key in _ATTRIBUTES:
                selection = value[0] if isinstance(value, tuple) else value
                if selection or selection == 0:
                    i = _ATTRIBUTES.index(key)
                    if selection is True:
                        positions = range(indices[i], indices[i + 1])
                    else:
                        positions = indices[i] + np.atleast_1d(selection)
                    mask[positions] = True
                if isinstance(value, tuple):
                    min_bounds = np.atleast_1d(np.asarray(value[1], dtype=float))
                    if len(min_bounds) == 1:
                        min_bounds = np.repeat(min_bounds, len(positions))
                    max_bounds = np.atleast_1d(np.asarray(value[2], dtype=float))
                    if len(max_bounds) == 1:
                        max_bounds = np.repeat(max_bounds, len(positions))
                    bounds[positions] = np.column_stack((min_bounds, max_bounds))
        if default_bounds is not None:
            missing_min, missing_max = np.isnan(bounds[:, 0]), np.isnan(bounds[:, 1])
            bounds[missing_min, 0] = default_bounds[missing_min, 0]
            bounds[missing_max, 1] = default_bounds[missing_max, 1]
        bounds[np.isnan(bounds[:, 0]), 0] = -np.inf
        bounds[np.isnan(bounds[:, 1]), 1] = np.inf
        return mask, bounds

    def _test(self):
        if not len(self.controls):
            raise ValueError("No controls reference the cameras")
        for i, idx in enumerate(self.group_indices):
            fc = "f" in self.group_params[i] or "c" in self.group_params[i]
            sizes = np.unique(np.vstack([self.cams[j].imgsz for j in idx]), axis=0)
            if fc and len(sizes) > 1:
                raise ValueError("Group " + str(i) + ": 'f' or 'c' in parameters but image sizes not equal")
        M = np.vstack(self.group_masks)
        overlaps = np.nonzero(np.count_nonzero(M, axis=0) > 1)[0]
        for i in overlaps:
            groups = np.nonzero(M[:, i])[0]
            idx = np.concatenate([self.group_indices[group] for group in groups])
            if len(np.unique(idx)) < len(idx):
                raise ValueError("Some cameras are in multiple groups with overlapping masks")
        control_cams = [cam for control in self.controls for cam in self._get_control_cams(control)]
        cams_with_params = [cam for i, cam in enumerate(self.cams)
                            if self.cam_params[i]
                            or any([self.group_params[j] for j, idx in enumerate(self.group_indices) if i in idx])]
        if set(cams_with_params) - set(control_cams):
            raise ValueError("Not all cameras with params appear in controls")

    def _build_scales(self):
        scales = [self.camera_scales(cam, self.controls) for cam in self.cams]
        cam_scales = [scale[mask] for scale, mask in zip(scales, self.cam_masks)]
        group_scales = [np.nanmean(np.vstack([scales[i][mask] for i in idx]), axis=0)
                        for mask, idx in zip(self.group_masks, self.group_indices)]
        self.scales = np.hstack((np.hstack(group_scales), np.hstack(cam_scales)))

    def _build_sparsity(self):
        """optimize.py:1580-1613: which residuals (two per control point) depend on which parameter."""
        import scipy.sparse

        m_control = [2 * control.size for control in self.controls]
        n = self.cam_breaks[-1]
        groups = np.zeros((len(self.cams), len(self.group_indices)), dtype=bool)
        for i, idx in enumerate(self.group_indices):
            groups[list(idx), i] = True
        S = scipy.sparse.lil_matrix((sum(m_control), n), dtype=int)
        control_breaks = np.cumsum([0] + m_control)
        for i, control in enumerate(self.controls):
            ctrl_slice = slice(control_breaks[i], control_breaks[i + 1])
            for cam in self._get_control_cams(control):
                try:
                    j = self.cams.index(cam)
                except ValueError:
                    continue
                S[ctrl_slice, slice(self.cam_breaks[j], self.cam_breaks[j + 1])] = 1
                for group in np.nonzero(groups[j])[0]:
                    S[ctrl_slice, slice(self.group_breaks[group], self.group_breaks[group + 1])] = 1
        self.sparsity = S

    def update_params(self):
        """optimize.py:1615-1670: `params` (label -> (value, min, max)) and the masks and breaks `set_cameras` uses, from
        the cameras' current state.  A group parameter starts at the mean over its cameras."""
        self.params = {}
        cam_bounds = [self.camera_bounds(cam) for cam in self.cams]
        self.cam_masks, cam_bounds = zip(*[self.parse_params(params, default_bounds=bounds)
                                           for params, bounds in zip(self.cam_params, cam_bounds)])
        cam_labels = [self._lmfit_labels(mask, cam=i, group=None) for i, mask in enumerate(self.cam_masks)]
        cam_values = [self.cams[i]._vector[mask] for i, mask in enumerate(self.cam_masks)]
        self.group_masks = []
        for group, idx in enumerate(self.group_indices):
            bounds = np.column_stack((np.column_stack([cam_bounds[i][:, 0] for i in idx]).max(axis=1),
                                      np.column_stack([cam_bounds[i][:, 1] for i in idx]).min(axis=1)))
            mask, bounds = self.parse_params(self.group_params[group], default_bounds=bounds)
            labels = self._lmfit_labels(mask, cam=None, group=group)
            values = np.nanmean(np.vstack([self.cams[i]._vector[mask] for i in idx]), axis=0)
            for label, value, bound in zip(labels, values, bounds[mask]):
                self.params[label] = (float(value), float(bound[0]), float(bound[1]))
            self.group_masks.append(mask)
        for i in range(len(self.cams)):
            for label, value, bound in zip(cam_labels[i], cam_values[i], cam_bounds[i][self.cam_masks[i]]):
                self.params[label] = (float(value), float(bound[0]), float(bound[1]))
        self.group_breaks = np.cumsum([0] + [np.count_nonzero(mask) for mask in self.group_masks])
        self.cam_breaks = np.cumsum([self.group_breaks[-1]] + [np.count_nonzero(mask) for mask in self.cam_masks])

    def set_cameras(self, params, save=False):
        """optimize.py:1672-1696: write parameter values ([group0 | group1 | cam0 | cam1 | ...], or a mapping as
        `params`) into the cameras; `save`: also as the state `reset_cameras` returns to."""
        if isinstance(params, dict):
            params = [value[0] if isinstance(value, tuple) else value for value in params.values()]
        for i, idx in enumerate(self.group_indices):
            for j in idx:
                self.cams[j]._vector[self.group_masks[i]] = params[self.group_breaks[i]:self.group_breaks[i + 1]]
                self.cams[j]._vector[self.cam_masks[j]] = params[self.cam_breaks[j]:self.cam_breaks[j + 1]]
        if save:
            self.vectors = [cam.to_array() for cam in self.cams]

    def reset_cameras(self):
        for cam, vector in zip(self.cams, self.vectors):
            cam._vector = vector.copy()

    @property
    def size(self):
        return np.sum([control.size for control in self.controls])

    def observed(self, index=slice(None)):
        if len(self.controls) == 1:
            return self.controls[0].observed(index=index)
        return np.vstack([control.observed() for control in self.controls])[index]

    # ---- the controls on the device
    def upload(self):
        """The controls on the device, as `_lib.Calib`; while it is open, `predicted`, `residuals` and `jacobian` evaluate
        through it (close it after use, or use it as a context manager)."""
        dev_cams = list(self.cams)
        for control in self.controls:
            for cam in self._get_control_cams(control):
                if not any(cam is c for c in dev_cams):
                    dev_cams.append(cam)  # (a camera that is not fitted: it keeps its vector)
        where = lambda cam: [cam is c for c in dev_cams].index(True)  # noqa: E731
        kind, cam_a, cam_b, directions, obs, src = [], [], [], [], [], []
        for control in self.controls:
            k = _kind_of(control)
            kind.append(k)
            cams = self._get_control_cams(control)
            cam_a.append(where(cams[0]))
            cam_b.append(where(cams[-1]))
            directions.append(int(bool(getattr(control, "directions", False))))
            if k in (_lib.CALIB_KINDS["points"], _lib.CALIB_KINDS["lines"]):
                first = control.uv
                second = control.xyz if k == _lib.CALIB_KINDS["points"] else np.zeros((control.size, 3))
            else:
                sides = control.uvs if k == _lib.CALIB_KINDS["matches"] else control.xys
                first, second = sides[0], np.column_stack((sides[1], np.zeros(len(sides[1]))))
            obs.append(np.asarray(first, dtype=float).reshape(-1, 2))
            src.append(np.asarray(second, dtype=float).reshape(-1, 3))
        offsets = np.concatenate(([0], np.cumsum([len(o) for o in obs]))).astype(np.int64)
        handle = _lib.Calib(len(dev_cams), kind, cam_a, cam_b, directions, offsets, np.concatenate(obs), np.concatenate(src),
                            device_id=self.device_id)
        self._handle, self._dev_cams = handle, dev_cams
        return handle

    def _open(self):
        return self._handle if self._handle is not None and self._handle._h else None

    def _job_table(self, control):
        """The checks `control.predicted` makes, at the cameras' current state, and the segment table of a Lines control."""
        control._test_position()
        if isinstance(control, RotationMatches):
            control._test_internals()
        return control._segment_table() if isinstance(control, Lines) else None

    def _evaluate(self, handle, sets, jobs, return_times=False):
        """`predicted` of the `jobs` [(control, set)] under the camera vectors `sets` [[vector (20,) per camera]], as one
        device call: a list of (size, 2) arrays in job order."""
        import time

        saved = [cam._vector for cam in self.cams]
        by_set = {}
        for q, (_, s) in enumerate(jobs):
            by_set.setdefault(s, []).append(q)
        tables = [None] * len(jobs)
        t0 = time.perf_counter()
        try:
            for s, members in by_set.items():
                for cam, vector in zip(self.cams, sets[s]):
                    cam._vector = vector
                for q in members:
                    tables[q] = self._job_table(self.controls[jobs[q][0]])
        finally:
            for cam, vector in zip(self.cams, saved):
                cam._vector = vector
        t1 = time.perf_counter()
        cams24 = np.empty((len(sets), len(self._dev_cams), _lib.CAM_LEN))
        cams24[:] = np.array([cam.vector24 for cam in self._dev_cams])
        cams24[:, :len(self.cams), :20] = np.asarray(sets, dtype=float)
        rot = rotations(cams24[:, :, 3:6].reshape(-1, 3))[0].reshape(len(sets), len(self._dev_cams), 3, 3)
        out = handle.eval(cams24, rot, [i for i, _ in jobs], [s for _, s in jobs], tables=tables, return_times=return_times)
        flat, times = out if return_times else (out, None)
        breaks = np.cumsum([self.controls[i].size for i, _ in jobs])[:-1]
        blocks = np.split(flat, breaks)
        if return_times:
            times["segment_tables_host"] = (t1 - t0) * 1e3
            return blocks, times
        return blocks

    def predicted(self, params=None, index=slice(None)):
        """optimize.py:1721-1746: the controls' predicted coordinates, at `params` if given (the cameras are left as they
        were).  Through the handle of `upload` while it is open -- one device call -- else control by control."""
        if params is not None:
            vectors = [cam.to_array() for cam in self.cams]
            self.set_cameras(params)
        try:
            handle = self._open()
            if handle is not None:
                blocks = self._evaluate(handle, [[cam._vector for cam in self.cams]], [(i, 0) for i in range(len(self.controls))])
                result = np.vstack(blocks)[index]
            elif len(self.controls) == 1:
                result = self.controls[0].predicted(index=index)
            else:
                result = np.vstack([control.predicted() for control in self.controls])[index]
        finally:
            if params is not None:
                for cam, vector in zip(self.cams, vectors):
                    cam._vector = vector
        return result

    def residuals(self, params=None, index=slice(None)):
        """optimize.py:1748-1764: predicted - observed, times the weights."""
        d = self.predicted(params=params, index=index) - self.observed(index=index)
        if self.weights is None:
            return d
        return d * self.weights[index]

    def errors(self, params=None, index=slice(None)):
        return np.linalg.norm(self.residuals(params=params, index=index), axis=1)

    def _values_bounds(self, params=None):
        table = np.array(list(self.params.values()), dtype=float).reshape(-1, 3)
        if params is None:
            x = table[:, 0].copy()
        elif isinstance(params, dict):
            x = np.array([value[0] if isinstance(value, tuple) else value for value in params.values()], dtype=float)
        else:
            x = np.array(params, dtype=float)
        return x, table[:, 1], table[:, 2]

    @staticmethod
    def _steps(x0, lb, ub):
        """scipy.optimize's forward-difference steps (approx_derivative, "2-point", default relative step):
        sqrt(eps) * (+1 if x >= 0 else -1) * max(1, |x|), turned round where x + h leaves the bounds and -h fits, and
        shortened to the wider side where neither fits."""
        h = np.finfo(np.float64).eps ** 0.5 * ((x0 >= 0).astype(float) * 2 - 1) * np.maximum(1.0, np.abs(x0))
        lower_dist, upper_dist = x0 - lb, ub - x0
        x = x0 + h
        violated = (x < lb) | (x > ub)
        fitting = np.abs(h) <= np.maximum(lower_dist, upper_dist)
        h[violated & fitting] *= -1
        forward = (upper_dist >= lower_dist) & ~fitting
        h[forward] = upper_dist[forward]
        backward = (upper_dist < lower_dist) & ~fitting
        h[backward] = -lower_dist[backward]
        return h

    def _jacobian_plan(self, params=None):
        """(sets, dx, jobs) of one Jacobian at `params`: the camera vectors of the base set and of every set with one
        parameter stepped, the steps as the difference quotient divides by them ((x_j + h) - x_j), and the jobs
        [(control, set)]: every control at the base set, then per parameter the controls `self.sparsity` marks."""
        import scipy.sparse

        x0, lb, ub = self._values_bounds(params)
        if np.any((x0 < lb) | (x0 > ub)):
            raise ValueError("`x0` violates bound constraints.")
        h = self._steps(x0, lb, ub)
        n, n_controls = len(x0), len(self.controls)
        breaks = 2 * np.concatenate(([0], np.cumsum([control.size for control in self.controls])))
        if self.sparsity is None:
            marked = [range(n_controls)] * n
        else:
            S = scipy.sparse.csc_matrix(self.sparsity)
            marked = [np.unique(np.searchsorted(breaks, S.indices[S.indptr[j]:S.indptr[j + 1]], side="right") - 1) for j in range(n)]
        saved = [cam._vector for cam in self.cams]
        sets, dx = [], np.empty(n)
        try:
            for j in range(-1, n):
                x = x0.copy()
                if j >= 0:
                    x[j] = x0[j] + h[j]
                    dx[j] = x[j] - x0[j]
                for cam, vector in zip(self.cams, saved):
                    cam._vector = vector.copy()
                self.set_cameras(x)
                sets.append([cam._vector for cam in self.cams])
        finally:
            for cam, vector in zip(self.cams, saved):
                cam._vector = vector
        jobs = [(i, 0) for i in range(n_controls)] + [(int(i), j + 1) for j in range(n) for i in marked[j]]
        return sets, dx, jobs

    def jacobian(self, params=None, index=slice(None), return_times=False):
        """The Jacobian of `residuals(params, index).ravel()` by scipy.optimize's 2-point forward differences, entry
        (f(x + h e_j) - f(x)) / ((x_j + h) - x_j) with the steps of `_steps` inside `params`' bounds -- bit for bit what
        scipy.optimize.least_squares(jac="2-point", jac_sparsity=self.sparsity) computes from the same residuals -- with
        every (control, parameter) block that `self.sparsity` marks (every block without one) evaluated in ONE device call.
        A sparse matrix of that structure (dense without).  Needs the handle of `upload` open."""
        import scipy.sparse

        handle = self._open()
        if handle is None:
            raise RuntimeError("Cameras.jacobian evaluates through the handle of Cameras.upload(): open one first")
        sets, dx, jobs = self._jacobian_plan(params)
        n, n_controls = len(dx), len(self.controls)
        sizes = [control.size for control in self.controls]
        breaks = 2 * np.concatenate(([0], np.cumsum(sizes)))
        out = self._evaluate(handle, sets, jobs, return_times=return_times)
        blocks, times = out if return_times else (out, None)
        weights = None if self.weights is None else np.split(self.weights, np.cumsum(sizes)[:-1])

        def residual(q):
            i = jobs[q][0]
            d = blocks[q] - self.controls[i].observed()
            return (d if weights is None else d * weights[i]).ravel()

        f0 = [residual(i) for i in range(n_controls)]
        rows, cols, values = [], [], []
        for q in range(n_controls, len(jobs)):
            i, j = jobs[q][0], jobs[q][1] - 1
            rows.append(np.arange(breaks[i], breaks[i + 1]))
            cols.append(np.full(2 * sizes[i], j))
            values.append((residual(q) - f0[i]) / dx[j])
        m = int(breaks[-1])
        if self.sparsity is None:  # (every block is there; written in place: a sum into zeros would lose the sign of -0.0)
            J = np.zeros((m, n))
            for r, c, v in zip(rows, cols, values):
                J[r, c] = v
        else:
            J = scipy.sparse.csr_matrix(scipy.sparse.coo_matrix(
                (np.concatenate(values) if values else np.zeros(0), (np.concatenate(rows) if rows else np.zeros(0, int),
                                                                     np.concatenate(cols) if cols else np.zeros(0, int))), shape=(m, n)))
        if not (isinstance(index, slice) and index == slice(None)):
            picked = np.arange(m // 2)[index] if isinstance(index, slice) else np.asarray(index)
            J = J[np.dstack((2 * picked, 2 * picked + 1)).ravel()]
        return (J, times) if return_times else J

    def fit(self, index=slice(None), cam_params=None, group_params=None, full=False, method="least_squares", **kwargs):
        """optimize.py:1781-1878: the parameter values that minimise the residuals (`index`: of which control points), by
        scipy.optimize.least_squares inside the parameters' bounds, with `x_scale=self.scales` and
        `jac_sparsity=self.sparsity` (its rows of `index`) unless `kwargs` say otherwise.  Only this, the reference's
        default method, is served: it is what lmfit.minimize(method="least_squares") runs.  `cam_params`, `group_params`:
        lists of parameter sets to fit one after the other first, each from the previous result (each such fit with its
        own scales and sparsity; the caller's `kwargs` are passed on).  `nan_policy` ("omit", the default: rows with NaN
        are dropped from each evaluation; "raise"; "propagate") is lmfit's -- with a sparsity structure, dropped rows end
        in scipy's shape error, as in the reference.

        Unless `kwargs` has `jac`, the controls are uploaded and the Jacobian is `self.jacobian`: all its columns in one
        device call.  Returns the values as an array, or None (and prints the message) if the fit failed; `full`: scipy's
        OptimizeResult with `params` (label -> (value, min, max)) added."""
        import scipy.optimize

        if method != "least_squares":
            raise NotImplementedError(_NO_LMFIT.format(method))
        user_kwargs = dict(kwargs)
        kwargs = {"nan_policy": "omit", **kwargs}
        nan_policy = kwargs.pop("nan_policy")
        if self.scales is not None and "x_scale" not in kwargs:
            kwargs["x_scale"] = self.scales
        if self.sparsity is not None and "jac_sparsity" not in kwargs:
            if isinstance(index, slice) and index == slice(None):
                kwargs["jac_sparsity"] = self.sparsity
            else:
                jac_index = np.arange(self.size)[index] if isinstance(index, slice) else np.asarray(index)
                jac_index = np.dstack((2 * jac_index, 2 * jac_index + 1)).ravel()
                kwargs["jac_sparsity"] = self.sparsity.tocsr()[jac_index]
        iterations = max(len(cam_params) if cam_params else 0, len(group_params) if group_params else 0)
        if iterations:
            for n in range(iterations):
                model = Cameras(cams=self.cams, controls=self.controls,
                                cam_params=cam_params[n] if cam_params else self.cam_params,
                                group_params=group_params[n] if group_params else self.group_params)
                values = model.fit(index=index, method=method, **user_kwargs)
                if values is not None:
                    model.set_cameras(params=values)
            self.update_params()

        def keep(r):
            if nan_policy == "omit":
                return ~np.isnan(r)
            if nan_policy == "raise" and np.isnan(r).any():
                raise ValueError("NaN values detected in your input data or the output of your objective/model function - "
                                 "fitting algorithms cannot handle this!")
            return np.ones(len(r), dtype=bool)

        def fun(x):
            resid = self.residuals(x, index=index)
            with np.errstate(invalid="ignore"):
                err = np.linalg.norm(resid.reshape(-1, 2), ord=2, axis=1).mean()
            sys.stdout.write("\r" + str(err))
            sys.stdout.flush()
            r = np.asarray(resid).ravel()
            return r[keep(r)]

        def jac(x):
            J = self.jacobian(x, index=index)
            if self.sparsity is None:
                r = np.asarray(self.residuals(x, index=index)).ravel()
                J = J[keep(r)]
            return J

        x0, lb, ub = self._values_bounds()
        own = "jac" not in kwargs
        try:
            if own:
                self.upload()
                kwargs["jac"] = jac
            result = scipy.optimize.least_squares(fun, x0, bounds=(lb, ub), **kwargs)
        finally:
            if own and self._handle is not None:
                self._handle.close()
                self._handle = None
        sys.stdout.write("\n")
        if iterations:
            self.reset_cameras()
            self.update_params()
        if not result.success:
            print(result.message)
        if full:
            result.params = {label: (float(value), bounds[1], bounds[2])
                             for (label, bounds), value in zip(self.params.items(), result.x)}
            return result
        if result.success:
            return np.array(result.x)
        return None

    def plot(self, *args, **kwargs):
        raise NotImplementedError(_NO_PLOT)

    def plot_weights(self, *args, **kwargs):
        raise NotImplementedError(_NO_PLOT)


def ransac(model, n, max_error, min_inliers, iterations=100, batched=False, return_info=False, **kwargs):
    """optimize.py:2091-2150: (parameters, inlier indices) of `model` -- an object with `size`, `fit(index)` and
    `errors(params, index)` -- by Random Sample Consensus: fit to samples of `n`, keep the fit whose members within
    `max_error` number more than `min_inliers` besides the sample and have the smallest mean error.

    `batched`: the same answer with every sample fitted and scored in one device call and every distinct consensus set
    refitted in a second one (`_ransac_batched`); the device decides which set wins, the values returned are
    `model.fit`'s on that set.  `return_info` (with `batched`): a dict of what the device found is returned as well."""
    if batched:
        return _ransac_batched(model, n, max_error, min_inliers, iterations, return_info, kwargs)
    if return_info:
        raise ValueError("return_info describes the batched path: pass batched=True")
    params = None
    err = np.inf
    full = np.arange(model.size)
    for maybe_idx in _ransac_samples(n=n, size=model.size, iterations=iterations):
        maybe_params = model.fit(maybe_idx, **kwargs)
        if maybe_params is None:
            continue
        test_idx = np.delete(full, maybe_idx)
        test_errs = model.errors(maybe_params, test_idx)
        also_idx = test_idx[test_errs < max_error]
        if len(also_idx) > min_inliers:
            better_idx = np.concatenate((maybe_idx, also_idx))
            better_params = model.fit(better_idx, **kwargs)
            if better_params is None:
                continue
            this_err = np.mean(model.errors(better_params, better_idx))
            if this_err < err:
                params = better_params
                err = this_err
    if params is None:
        raise ValueError("Best fit does not meet acceptance criteria")
    inliers = np.where(model.errors(params) <= max_error)[0]
    return params, inliers


def _fit_options(no, kwargs):
    """The device fit's options among `kwargs`; NotImplementedError (`no`: who refuses) for any other keyword or value."""
    for key, value in kwargs.items():
        if key not in ("ftol", "xtol", "gtol", "max_nfev", "nan_policy") or value is None or (key == "nan_policy" and value != "omit"):
            raise NotImplementedError(no + f"{key}={value!r}: the device fit honours numbers for ftol, xtol, gtol and max_nfev "
                                      "(and nan_policy='omit')")
    return {key: kwargs[key] for key in ("ftol", "xtol", "gtol", "max_nfev") if key in kwargs}


def _refuse_held(no, control, slots, position):
    """`slots` fits what `control` holds fixed: internal parameters, or the position (`position` says so; None: it is free)."""
    if isinstance(control, RotationMatches) and (slots >= 6).any():
        raise NotImplementedError(no + "fitted internal parameters (f, c, k, p) under a RotationMatches control, whose "
                                  "camera coordinates hold them fixed")
    if position and (slots < 3).any():
        raise NotImplementedError(no + position)


def _refuse_raster_grid(no, cams):
    if any(cam.vector24[23] != 0 for cam in cams):
        raise NotImplementedError(no + "a camera with a raster grid")


def _check_bounds(x0, lb, ub):
    if np.any(lb >= ub):
        raise ValueError("Each lower bound must be strictly less than each upper bound.")
    if np.any((x0 < lb) | (x0 > ub)):
        raise ValueError("`x0` violates bound constraints.")


def _batched_plan(model, kwargs):
    """What `ransac(batched=True)` hands the device fit of `model`, or NotImplementedError naming what it does not serve
    (there is no host fallback); made before any library call."""
    no = "ransac(batched=True) does not serve "
    if not isinstance(model, Cameras):
        raise NotImplementedError(no + f"a {type(model).__name__} model: a Cameras model with one fitted camera")
    if len(model.cams) != 1:
        raise NotImplementedError(no + f"{len(model.cams)} fitted cameras: one")
    if any(np.any(mask) for mask in model.group_masks):
        raise NotImplementedError(no + "group_params: the parameters of one camera (cam_params)")
    options = _fit_options(no, kwargs)
    slots = np.flatnonzero(model.cam_masks[0])
    if not len(slots):
        raise NotImplementedError(no + "a model without a parameter to fit")
    cams = [model.cams[0]]
    for control in model.controls:
        if isinstance(control, Lines):
            raise NotImplementedError(no + "a Lines control: Points and the match controls")
        _kind_of(control)  # (RotationMatchesXYZ: NotImplementedError)
        held = "a fitted position (xyz) under a match control or ray directions, which hold it fixed"
        _refuse_held(no, control, slots, held if isinstance(control, Matches) or control.directions else None)
        cams += [cam for cam in model._get_control_cams(control) if not any(cam is c for c in cams)]
    _refuse_raster_grid(no, cams)
    for control in model.controls:
        model._job_table(control)  # (the checks `predicted` makes at the cameras' current state)
    x0, lb, ub = model._values_bounds()
    _check_bounds(x0, lb, ub)
    scales = np.ones(len(slots)) if model.scales is None else np.asarray(model.scales, dtype=float)
    weights = None if model.weights is None else np.ascontiguousarray(np.broadcast_to(model.weights, (model.size, 2)))
    # (a RotationMatches control keeps camera coordinates on the device and predicts image coordinates)
    rotation = any(_kind_of(control) == _lib.CALIB_KINDS["rotation"] for control in model.controls)
    observed = np.ascontiguousarray(model.observed(), dtype=float) if rotation else None
    return dict(slots=slots, x0=x0, lb=lb, ub=ub, x_scale=scales, weights=weights, observed=observed, options=options)


def _ransac_batched(model, n, max_error, min_inliers, iterations, return_info, kwargs):
    """`ransac` with the loop over the samples on the device:

    1. the samples H of `_ransac_samples`, drawn as the host path draws them (the same use of np.random);
    2. ONE device call (`_lib.Calib.fit_sets`) fits every sample from the model's current values and scores all rows
       under each fit: per hypothesis the values, a status and the consensus mask error < max_error outside the sample;
    3. the hypotheses with more than `min_inliers` in consensus; sample and consensus as one set; equal sets merged, the
       earliest hypothesis standing for its set;
    4. ONE device call refits every distinct set and returns its mean error over its own rows;
    5. the sets in order of mean error (ties to the earlier hypothesis): `model.fit(better_idx, **kwargs)` on the best,
       `better_idx` built as the host path builds it; the next set if that fit fails.

    The values returned are therefore scipy's, as on the host path; the device picks the set."""
    import time

    plan = _batched_plan(model, kwargs)
    t = [time.perf_counter()]
    samples = list(_ransac_samples(n=n, size=model.size, iterations=iterations))
    set_offset = np.arange(len(samples) + 1, dtype=np.int64) * n
    set_rows = np.array(samples, dtype=np.int64).reshape(-1)
    fit = dict(fit_cam=0, slots=plan["slots"], x0=plan["x0"], lb=plan["lb"], ub=plan["ub"], x_scale=plan["x_scale"],
               weights=plan["weights"], observed=plan["observed"], return_times=True, **plan["options"])
    try:
        handle = model.upload()
        cams24 = np.array([cam.vector24 for cam in model._dev_cams])
        t.append(time.perf_counter())
        (values, status, _, inlier), times_fit = handle.fit_sets(cams24, set_offset=set_offset, set_rows=set_rows,
                                                                 max_error=max_error, **fit)
        t.append(time.perf_counter())
        counts = (inlier == 1).sum(axis=1)
        sets, owner = {}, []
        for h in np.flatnonzero((status > 0) & (counts > min_inliers)):
            members = np.flatnonzero(inlier[h])
            if members.tobytes() not in sets:
                sets[members.tobytes()] = members
                owner.append(int(h))
        sets = list(sets.values())
        refit_offset = np.concatenate(([0], np.cumsum([len(rows) for rows in sets]))).astype(np.int64)
        refit_rows = np.concatenate(sets) if sets else np.zeros(0, np.int64)
        t.append(time.perf_counter())
        (refit_values, refit_status, mean_errors), times_refit = handle.fit_sets(cams24, set_offset=refit_offset,
                                                                                 set_rows=refit_rows, **fit)
        t.append(time.perf_counter())
    finally:
        if model._handle is not None:
            model._handle.close()
            model._handle = None
    # (a set whose refit failed, or with a row that has no prediction, is never chosen on the host path either)
    order = [k for k in np.argsort(mean_errors, kind="stable") if refit_status[k] > 0 and not np.isnan(mean_errors[k])]
    params, winner, full = None, None, np.arange(model.size)
    for k in order:
        maybe_idx = samples[owner[k]]
        test_idx = np.delete(full, maybe_idx)
        also_idx = test_idx[inlier[owner[k], test_idx] == 1]
        better_idx = np.concatenate((maybe_idx, also_idx))
        params = model.fit(better_idx, **kwargs)
        if params is not None:
            winner = int(k)
            break
    t.append(time.perf_counter())
    if params is None:
        raise ValueError("Best fit does not meet acceptance criteria")
    inliers = np.where(model.errors(params) <= max_error)[0]
    if not return_info:
        return params, inliers
    wall = np.diff(t) * 1e3
    device = lambda d: d["fit"] + d["score"]  # noqa: E731
    info = dict(values=values, status=status, consensus=counts, sets=sets, hypothesis=np.array(owner, dtype=int),
                refit_values=refit_values, refit_status=refit_status, mean_errors=mean_errors, winner=winner,
                times_ms=dict(upload=wall[0] + times_fit["upload"] + times_refit["upload"], fit_score=device(times_fit),
                              refit=device(times_refit), download=times_fit["download"] + times_refit["download"],
                              host=wall[2], final_fit=wall[4], calls=wall[1] + wall[3]))
    return params, inliers, info


def _ransac_samples(n, size, iterations=100):
    """optimize.py:2153-2188: up to `iterations` different samples of `n` of `size` indices, drawn by np.random.shuffle
    (at most as many as there are combinations)."""
    if n >= size:
        raise ValueError("Sample size is larger or equal to total size")
    log = math.lgamma(size + 1) - math.lgamma(n + 1) - math.lgamma(size - n + 1)
    if log:
        iterations = min(iterations, np.floor(np.exp(log)))
    samples = set()
    indices = np.arange(size)
    while len(samples) < iterations:
        np.random.shuffle(indices)
        sample = frozenset(indices[:n])
        if sample not in samples:
            yield list(sample)
            samples.add(sample)


RANSAC_PAIRS_BUDGET = 1 << 30  # bytes of consensus masks (hypotheses x rows) one device call of `ransac_pairs` may hold


def _pairs_plan(pairs, fitted, cam_params, kwargs):
    """What `ransac_pairs` hands the device for the pairs [(matches, i, j)]: the fitted entries `slots` of the camera vector
    and per pair (x0, lb, ub, scales) as `Cameras([m.cams[fitted]], [m], cam_params=[cam_params])` makes them -- or
    NotImplementedError / ValueError as `_batched_plan` raises them for that model.  Made before any library call."""
    no = "ransac_pairs does not serve "
    options = _fit_options(no, kwargs)
    if fitted not in (0, 1):
        raise ValueError(f"fitted is 0 (the pair's first camera) or 1 (its second), got {fitted!r}")
    mask = Cameras.parse_params(cam_params)[0]
    slots = np.flatnonzero(mask)
    if not len(slots):
        raise NotImplementedError(no + "cam_params without a parameter to fit")
    known, values = {}, []  # (what depends on the fitted camera alone is made once per camera)
    for m, i, j in pairs:
        if isinstance(m, RotationMatchesXYZ) or not isinstance(m, Matches):
            raise NotImplementedError(no + f"a {type(m).__name__} for pair ({i}, {j}): Matches, RotationMatches and RotationMatchesXY")
        _refuse_held(no, m, slots, "a fitted position (xyz) under a match control, which holds it fixed")
        _refuse_raster_grid(no, [cam for cam in m.cams if id(cam) not in known])
        for cam in m.cams:
            known.setdefault(id(cam))
        m._test_position()
        if isinstance(m, RotationMatches):
            m._test_internals()
        cam = m.cams[fitted]
        if known[id(cam)] is None:
            bounds = Cameras.parse_params(cam_params, default_bounds=Cameras.camera_bounds(cam))[1][mask]
            x0, lb, ub = np.array(cam._vector[mask], dtype=float), bounds[:, 0], bounds[:, 1]
            _check_bounds(x0, lb, ub)
            known[id(cam)] = (x0, lb, ub, Cameras.camera_scales(cam)[mask])
        values.append(known[id(cam)])
    return dict(slots=slots, values=values, options=options)


def _pairs_samples(pairs, n, iterations, samples, on_device):
    """Per pair the (H_k, n) rows of its samples (None: `n` rows or fewer), and whether the device draws them (zeros until then)."""
    drawn, device_drawn = [], np.zeros(len(pairs), dtype=bool)
    if on_device:
        counts, enumerated = _lib.ransac_hypotheses([m.size for m, _, _ in pairs], n, iterations)
        device_drawn = (counts > 0) & ~enumerated
    for k, (m, _, _) in enumerate(pairs):
        if m.size <= n:  # ("Sample size is larger or equal to total size")
            drawn.append(None)
        elif on_device:
            drawn.append(np.zeros((counts[k], n), np.int64) if device_drawn[k] else _lib.ransac_combinations(m.size, n, counts[k]))
        elif samples is None:
            drawn.append(np.array(list(_ransac_samples(n=n, size=m.size, iterations=iterations)), dtype=np.int64).reshape(-1, n))
        else:
            rows = np.asarray(samples[k])
            if rows.ndim != 2 or rows.shape[1] != n or not np.issubdtype(rows.dtype, np.integer) \
                    or (rows.size and (rows.min() < 0 or rows.max() >= m.size)):
                raise ValueError(f"samples[{k}]: an (H, {n}) integer array of row numbers below {m.size}")
            drawn.append(rows.astype(np.int64))
    return drawn, device_drawn


def _pairs_chunk(pairs, members, plan, fitted, drawn, device_drawn, seed, n):
    """One chunk, the pairs `members`: the arguments of `_lib.Calib` (its obs and src per pair, to be concatenated), the leading
    ones and the keywords of its `ransac_groups` (`seed`: None unless the device draws), and where rows and hypotheses lie."""
    ms = [pairs[k][0] for k in members]
    cams = list({id(cam): cam for m in ms for cam in m.cams}.values())  # (each camera once, in the order met)
    where = {id(cam): q for q, cam in enumerate(cams)}
    kind = [_kind_of(m) for m in ms]
    sides = [m.uvs if c == _lib.CALIB_KINDS["matches"] else m.xys for m, c in zip(ms, kind)]
    obs = [np.asarray(s[0], dtype=float).reshape(-1, 2) for s in sides]
    src = [np.column_stack((s[1], np.zeros(len(s[1])))) for s in sides]
    row_offset = np.concatenate(([0], np.cumsum([len(o) for o in obs]))).astype(np.int64)
    hyp_offset = np.concatenate(([0], np.cumsum([len(drawn[k]) for k in members]))).astype(np.int64)
    values = (np.array([plan["values"][k][q] for k in members]).reshape(-1, len(plan["slots"])) for q in range(4))
    keywords = dict(observed=None, **plan["options"])
    if _lib.CALIB_KINDS["rotation"] in kind:  # (a RotationMatches keeps camera coordinates on the device and predicts image coordinates)
        keywords["observed"] = np.concatenate([np.asarray(m.observed(), dtype=float).reshape(-1, 2) for m in ms])
    if seed is not None:
        keywords.update(group_id=members, drawn=device_drawn[members], seed=(seed & 0xFFFFFFFF, seed >> 32), n=n)
    rows = None if seed is not None and device_drawn[members].all() else \
        np.concatenate([drawn[k] + row_offset[g] for g, k in enumerate(members)])  # (None: the device draws every sample)
    cam_a, cam_b = ([where[id(m.cams[side])] for m in ms] for side in (0, 1))
    controls = (len(cams), kind, cam_a, cam_b, np.zeros(len(ms), np.int32), row_offset)
    call = (np.array([cam.vector24 for cam in cams]), np.arange(len(ms)), (cam_a, cam_b)[fitted], plan["slots"], *values,
            hyp_offset, rows)
    return controls, (obs, src), call, keywords, row_offset, hyp_offset


def ransac_pairs(pairs, n, max_error, min_inliers, iterations=100, cam_params=None, fitted=1, samples=None, budget=None,
                 return_info=False, seed=None, **kwargs):
    """Random Sample Consensus over every image pair of `pairs` (whatever `match_pairs` accepts: `KeypointMatcher.matches`, a
    dict {(i, j): matches}, an (n, n) object array; each entry a `Matches`, `RotationMatches` or `RotationMatchesXY`) in ONE
    device pass per chunk of pairs (`glh_calib_ransac_groups`).  Returns a list in pair order of `(params, inliers)` as
    `ransac` returns them, or None where `ransac` would raise for that pair (no fit meets the acceptance criteria, or the
    pair has `n` rows or fewer): one bad pair does not end a sequence.

    Pair k is treated as `ransac(Cameras([m.cams[fitted]], [m], cam_params=[cam_params]), n, max_error, min_inliers,
    iterations, **kwargs)` treats it: the pair's second (`fitted=1`) or first (0) camera is fitted from its own current
    vector with that model's bounds and scales, the other camera is held; consensus is error < max_error outside the
    sample; a hypothesis with more than `min_inliers` in consensus is refitted on sample and consensus; the smallest mean
    error wins, the earlier hypothesis of equal ones; the inliers are error <= max_error under the winner.  The pairs are
    independent: a camera fitted in one pair and held in another is seen at its original vector by both, and no camera is
    modified.

    The samples are drawn on the host by `_ransac_samples`, pair after pair, so under one `np.random.seed` they are the
    samples a loop of `ransac` over the pairs draws.  `samples`: instead, per pair an (H_k, n) integer array of row numbers
    within the pair.  `samples="device"`: the samples are drawn on the device, in the pass that fits them (INPUTS.md,
    "Device samples: the rule"): pair k gets min(iterations, C(size, n)) hypotheses, the binomial coefficient exact -- all
    combinations in lexicographic order if there are no more than `iterations`, else each hypothesis drawn independently
    (Floyd's algorithm on a Philox stream) as a function of (`seed`, k, the hypothesis's number, size, n) alone, so that
    the result depends neither on the other pairs nor on `budget`; two hypotheses of a pair may then be the same sample,
    which changes nothing but the count.  `seed`: an integer of 0 .. 2^64 - 1 for that mode; None takes two 32-bit words
    from one call of `np.random.randint`, so that `np.random.seed` still makes a run reproducible.  The other modes do not
    touch it, and their use of np.random is what it was.

    `params` are the DEVICE's refit values on the winning set (a damped Gauss-Newton, `glh_lm.h`), not scipy's: they agree with `Cameras.fit` on that set to well within 1e-3 of each parameter's scale, and the host fit per
    pair is the cost this call removes.  `budget`: an upper bound in bytes (default RANSAC_PAIRS_BUDGET) on the device memory
    for the consensus masks, hypotheses x rows bytes per pair: the pairs are processed in consecutive chunks that stay
    below it, a pair whose own masks exceed it in a chunk of its own; the result does not depend on the chunking.
    `return_info`: also a dict with, per hypothesis, `values`, `status`, `consensus`, `refit_values`, `refit_status`,
    `mean_errors` (hypotheses of pair k: hyp_offset[k] .. hyp_offset[k + 1]); per pair `winner` (counted from the pair's
    first hypothesis, -1: none); `samples`, per pair the (H_k, n) rows sampled or None for a pair too short; `seed` in
    device mode; and `times_ms` (with `draw` in device mode).

    Refused with NotImplementedError, before any library call: what `_batched_plan` refuses for such a model (a fitted
    position, internal parameters under a RotationMatches, a raster-grid camera, kwargs other than numeric ftol / xtol /
    gtol / max_nfev and nan_policy="omit") and any control that is not one of the three match kinds.  ValueError: x0
    outside its bounds, or a lower bound that is not below the upper; a string for `samples` other than "device", a `seed`
    outside 0 .. 2^64 - 1, or a `seed` without samples="device"."""
    import time

    t = [time.perf_counter()]
    on_device = isinstance(samples, str)
    if on_device and samples != "device":
        raise ValueError(f"samples: 'device', None or one array per pair, got {samples!r}")
    if seed is not None:
        if not on_device:
            raise ValueError("seed: the seed of samples='device'; the other samples are np.random's or the caller's")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
            raise ValueError(f"seed: an integer of 0 .. 2^64 - 1, got {seed!r}")
    cam_params = {"viewdir": True} if cam_params is None else cam_params
    pairs = [] if isinstance(pairs, (list, tuple)) and not len(pairs) else match_pairs(pairs)
    plan = _pairs_plan(pairs, fitted, cam_params, kwargs)
    if not pairs:
        return ([], dict(winner=np.zeros(0, np.int32), hyp_offset=np.zeros(1, np.int64), samples=[], times_ms={})) if return_info else []
    if samples is not None and not on_device and len(samples) != len(pairs):
        raise ValueError(f"samples: one array per pair ({len(pairs)}), got {len(samples)}")
    if on_device and seed is None:  # (after the plan's checks, and the only use of np.random in this mode)
        words = np.random.randint(0, 2 ** 32, size=2, dtype=np.uint64)
        seed = int(words[0]) | int(words[1]) << 32
    seed = None if seed is None else int(seed)
    t.append(time.perf_counter())
    drawn, device_drawn = _pairs_samples(pairs, n, iterations, samples, on_device)
    t.append(time.perf_counter())
    served = [k for k, rows in enumerate(drawn) if rows is not None]
    budget = min(max(RANSAC_PAIRS_BUDGET if budget is None else int(budget), 0), 2 ** 31 - 1)
    chunk_of = _lib.ransac_chunks([pairs[k][0].size for k in served], [len(drawn[k]) for k in served], budget) if served else np.zeros(0, np.int32)
    chunks = int(chunk_of.max()) + 1 if served else 0
    winner = np.full(len(pairs), -1, dtype=np.int32)
    results, outs = [None] * len(pairs), []
    device_times = _lib.CALIB_RANSAC_TIMES[1:] + (("draw",) if on_device else ())
    host, times = 0.0, dict.fromkeys(("upload",) + device_times, 0.0)
    for chunk in range(chunks):
        t0 = time.perf_counter()
        members = [served[q] for q in np.flatnonzero(chunk_of == chunk)]
        controls, obs_src, call, keywords, row_offset, hyp_offset = _pairs_chunk(pairs, members, plan, fitted, drawn, device_drawn, seed, n)
        t1 = time.perf_counter()
        handle = _lib.Calib(*controls, *(np.concatenate(v) for v in obs_src))  # (the copies: counted with the upload)
        try:
            t2 = time.perf_counter()
            out, device = handle.ransac_groups(*call, max_error, min_inliers, return_times=True, **keywords)
        finally:
            handle.close()
        outs.append(out)
        for g, k in enumerate(members):
            if device_drawn[k]:
                drawn[k] = out["samples"][hyp_offset[g]:hyp_offset[g + 1]] - row_offset[g]
            winner[k] = out["winner"][g]
            if winner[k] >= 0:
                inliers = np.flatnonzero(out["inlier"][row_offset[g]:row_offset[g + 1]])
                results[k] = (out["refit_values"][hyp_offset[g] + winner[k]].copy(), inliers)
        host += t1 - t0
        times["upload"] += (t2 - t1) * 1e3 + device["upload"]
        for key in device_times:
            times[key] += device[key]
    if not return_info:
        return results
    info = {key: (np.concatenate([out[key] for out in outs]) if outs else np.zeros((0, len(plan["slots"])) if "values" in key else 0))
            for key in ("values", "status", "consensus", "refit_values", "refit_status", "mean_errors")}
    info["winner"] = winner
    info["hyp_offset"] = np.concatenate(([0], np.cumsum([0 if rows is None else len(rows) for rows in drawn]))).astype(np.int64)
    info["chunks"] = chunks
    info["samples"] = drawn
    if on_device:
        info["seed"] = seed
    info["times_ms"] = dict(sampling=(t[2] - t[1]) * 1e3, host=(t[1] - t[0] + host) * 1e3, **times)
    return results, info


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
        self.matcher = None  # (set it to a KeypointMatcher(observer.images) for build_keypoints / build_matches)
        self.device_id = 0
        self.viewdirs = np.vstack([img.cam.viewdir.copy() for img in self.observer.images])

    def set_cameras(self, viewdirs):
        for i, img in enumerate(self.observer.images):
            img.cam.viewdir = viewdirs[i]

    def reset_cameras(self):
        self.set_cameras(viewdirs=self.viewdirs.copy())

    def build_keypoints(self, **kwargs):
        if self.matcher is None:
            raise NotImplementedError(_NO_MATCHER)
        self.matcher.build_keypoints(**kwargs)

    def build_matches(self, **kwargs):
        """optimize.py:2018-2022, with `self.matcher` a `KeypointMatcher` of the observer's images."""
        if self.matcher is None:
            raise NotImplementedError(_NO_MATCHER)
        self.matcher.build_matches(**kwargs)
        self.matcher.convert_matches(RotationMatchesXYZ)
        self.matches = self.matcher.matches

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
