"""`Image`: `glimpse.Image` (/root/reference/src/glimpse/image.py) for the tracking path.

Holds a `Camera`, a capture datetime and the pixels: an in-memory array (the reference's cached read,
image.py:180-186, :211-213) or a file that is decoded on first use (the reference reads it band by band
through GDAL, image.py:187-210; here Pillow decodes it, which for the 8-bit JPEG / PNG / TIFF files of a
time-lapse camera gives the same samples).  A read at another size than the file's (`cam.resize(...)`, image.py:188-193)
is GDAL's default RasterIO resampling -- nearest neighbour, destination pixel i from source column
floor((i + 0.5) * src / dst) -- on the decoded array; GDAL itself is absent here, and for JPEG files it would first pick
one of the decoder's built-in 1/2, 1/4, 1/8 overviews, which this does not reproduce (parity unpinned for resized
reads).  `project` (image.py:301-361) resamples the frame into another camera on the GPU; `orthorectify`, which the reference
leaves to its users, resamples it onto a DEM's grid there.  EXIF parsing, `write` and `plot` are out of scope (SURVEY.md
section 2).
"""
import numpy as np

from . import _lib
from .camera import Camera


class Image:
    def __init__(self, path=None, cam=None, datetime=None, exif=None, array=None):
        self.path = None if path is None else str(path)
        if isinstance(cam, dict):
            cam = Camera(**cam)
        if cam is None:
            raise ValueError("cam is required (EXIF / file metadata are out of scope here)")
        if path is None and array is None:
            raise ValueError("either path or array is required")
        self.cam = cam
        if not datetime:
            raise ValueError("datetime is required (EXIF parsing is out of scope here)")
        self.datetime = datetime
        self.exif = exif
        self.array = None if array is None else np.asarray(array)

    @property
    def size(self):
        """image.py:121-124."""
        return self.cam.imgsz

    def _decode(self):
        """The whole file as (h, w) or (h, w, bands), like np.dstack of GDAL's bands (image.py:200-206)."""
        if self.path is None:
            raise ValueError("the image has neither an array nor a path")
        try:
            from PIL import Image as _PILImage
        except ImportError as e:  # pragma: no cover
            raise NotImplementedError("reading image files needs Pillow; assign Image.array instead") from e
        with _PILImage.open(self.path) as im:
            if im.mode == "P":
                im = im.convert("RGB")
            a = np.asarray(im)
        if a.ndim == 3 and a.shape[2] == 1:
            a = a[:, :, 0]
        return a

    @staticmethod
    def _nearest(n_src, n_dst, offset=0.0, count=None):
        """Source index of every destination pixel under GDAL's default (nearest neighbour) RasterIO resampling of a
        window of `count` source pixels starting at `offset` into `n_dst` pixels."""
        count = n_src if count is None else count
        idx = np.floor(offset + (np.arange(n_dst) + 0.5) * (count / n_dst) + 1e-10).astype(np.int64)
        return np.clip(idx, 0, n_src - 1)

    def read(self, box=None, cache=True):
        """image.py:137-214: the cached array, or the file (decoded once and kept when `cache`), at the camera's image
        size: an array of another size is resampled to it (and the resampled array is what is cached, like the
        reference caches what GDAL returned; for an image without a file the caller's array is kept and the resampled
        copy cached beside it).  `box` = (left, top, right, bottom) in camera image coordinates; with `cache=False`
        the box is read straight from the file's own pixels and resampled to the BOX's size -- the reference hands GDAL
        buf_xsize / buf_ysize = the camera's whole image size for that window (image.py:192-201), so its output has
        another shape there; tracking never reads that way (Observer.extract_tile passes the observer's cache flag,
        and a cached image is sliced)."""
        cw, ch = (int(v) for v in self.cam.imgsz)
        array = self.array
        kept = getattr(self, "_resized", None)
        if kept is not None and self.path is None and array is not None and kept[0] == (cw, ch) \
                and array.shape[1::-1] != (cw, ch):
            array = kept[1]  # (the copy of an in-memory image resampled to this camera size)
        if array is not None and array.shape[1::-1] != (cw, ch) and self.path is not None:
            array = None  # (a cached read of another size is not reused: image.py:183-187)
        from_file = array is None
        if from_file:
            array = self._decode()
        h, w = array.shape[:2]
        if (w, h) != (cw, ch):
            if box is not None and not cache and from_file:
                # the window of the file that the box covers, resampled to the box's size (image.py:196-201)
                xs, ys = w / cw, h / ch
                x0, y0 = int(round(box[0] * xs)), int(round(box[1] * ys))
                nx, ny = int(round((box[2] - box[0]) * xs)), int(round((box[3] - box[1]) * ys))
                cols = self._nearest(w, box[2] - box[0], x0, nx)
                rows = self._nearest(h, box[3] - box[1], y0, ny)
                return array[rows][:, cols]
            array = array[self._nearest(h, ch)][:, self._nearest(w, cw)]
        if from_file and cache:
            self.array = array
        elif not from_file and array is not self.array and cache and self.path is not None:
            self.array = array  # (image.py:207-209: a cached array of another size is replaced by the resized read)
        elif not from_file and array is not self.array and cache:
            # an in-memory image (no file to go back to: the reference would fail on gdal.Open(None) here): the caller's
            # pixels stay, the resampled copy is kept beside them for this camera size -- a later cam.resize(1) reads the
            # original again instead of upsampling a decimated copy
            self._resized = ((cw, ch), array)
        if box is not None:
            return array[box[1]:box[3], box[0]:box[2]]
        return array

    def xyz_to_uv(self, xyz, **kwargs):
        """image.py:279-285."""
        return self.cam.xyz_to_uv(xyz, **kwargs)

    def uv_to_xyz(self, uv, directions=False, **kwargs):
        return self.cam.uv_to_xyz(uv, directions=directions, **kwargs)

    def uv_to_dem(self, uv, dem, **kwargs):
        """`Camera.uv_to_dem` of this image's camera: the world points its pixels `uv` see on `dem`.  An image whose
        camera is a raster grid (an orthophoto) has no position to cast rays from."""
        if np.asarray(self.cam.vector24)[23] != 0:
            raise NotImplementedError("The image's camera is a raster grid, which has no position to cast rays from")
        return self.cam.uv_to_dem(uv, dem, **kwargs)

    def inbounds(self, uv):
        """image.py:297-299."""
        return self.cam.inframe(uv)

    def _check_project(self, cam, method, name="Source"):
        """The argument checks of `project`, made before anything touches the library."""
        if not all(np.asarray(cam.xyz) == self.cam.xyz):
            raise ValueError(f"{name} and target cameras have different positions ('xyz')")
        if method not in ("linear", "nearest"):
            raise ValueError(f"Method '{method}' is not defined")  # (scipy's RegularGridInterpolator says the same)

    def _project_frame(self):
        """The pixels `project` samples: `read()` with a third axis."""
        array = self.read()
        return array[:, :, None] if array.ndim < 3 else array

    def project(self, cam, method="linear"):
        """image.py:301-361: this image seen by `cam`, a camera at the same position (another view direction, focal
        length, distortion or image size) -- every pixel centre of `cam` is cast out as a ray, projected into this
        image's camera and sampled there with `method` = "linear" (bilinear) or "nearest", as
        scipy.interpolate.RegularGridInterpolator over the pixel centres does.  Returns (cam.imgsz[1], cam.imgsz[0],
        channels) in the dtype of the pixels (uint8, uint16, float32 or float64; one or three channels; a one-channel
        image comes back with a third axis of 1, like the reference).  Target pixels that see nothing of this image are
        NaN for float pixels.  For integer pixels the reference casts that NaN to the integer dtype, which NumPy calls
        an invalid cast and which stores 0 on x86: 0 is written here.  One kernel on the GPU (`glh_stage_reproject`);
        `Observer.project` is the batch form."""
        self._check_project(cam, method)
        frame = self._project_frame()
        return _lib.stage_reproject(frame[None], self.cam.vector24[None], cam.vector24, cam.imgsz, method)[0]

    def _check_orthorectify(self, dem, viewshed, mask, method, name="The image"):
        """The argument checks of `orthorectify`, made before anything touches the library."""
        if method not in ("linear", "nearest"):
            raise ValueError(f"Method '{method}' is not defined")  # (scipy's RegularGridInterpolator says the same)
        if np.ndim(dem.array) != 2:
            raise ValueError(f"a DEM is two-dimensional, got {np.shape(dem.array)}")
        if mask is not None and np.shape(mask) != np.shape(dem.array):
            raise ValueError("mask does not have the same 2-d shape as dem")
        if viewshed is not None and not isinstance(viewshed, (bool, np.bool_)) and np.shape(viewshed) != np.shape(dem.array):
            raise ValueError("viewshed does not have the same 2-d shape as dem")
        if np.asarray(self.cam.vector24)[23] != 0:
            raise ValueError(f"{name}'s camera is a raster grid, which has no position to see from")

    def orthorectify(self, dem, viewshed=None, mask=None, method="linear"):
        """This image on the grid of `dem` (a Raster with a 2-D array of elevations): the orthophoto of one oblique frame,
        the inverse of `Camera.project_dem`.  The reference has no single function for it; the rule (INPUTS.md,
        "Orthorectification: the rule") is composed of its calls.  For every cell (r, c): xyz = (dem.x[c], dem.y[r],
        dem.array[r, c]), the cell's centre in whichever direction the raster's axes run; uv = `cam.xyz_to_uv(xyz)`; the
        cell is seen when its elevation is not NaN, `cam.inframe(uv)`, `mask[r, c]` (where a mask is given) and
        `viewshed[r, c]` (where one is given); a seen cell's value is RegularGridInterpolator over the pixel centres,
        `method` = "linear" or "nearest", bounds_error=False, at uv, channel by channel -- the interpolator of `project`,
        so a seen cell within half a pixel of the frame's edge is NaN; every other cell is NaN.  `viewshed`: None (no
        visibility test), a boolean array of the DEM's shape, or True for `dem.viewshed(cam.xyz, correction=
        cam.correction)`.  Returns (dem rows, dem columns, channels), float32 for float32 pixels (the interpolator's
        float64 rounded once, as `project` returns them) and float64 for uint8, uint16 and float64 pixels; nothing is cast back to integers, so NaN always means
        "not seen".  One kernel on the GPU (`glh_stage_orthorectify`); `Observer.orthorectify` is the batch form."""
        self._check_orthorectify(dem, viewshed, mask, method)
        return orthorectify([self], dem, viewshed, mask, method)[0]

    def displacements(self, other, uv, **kwargs):
        """`glimpse_amd.displacements(self.read(), other.read(), uv, **kwargs)`: where the surroundings of this image's
        points `uv` are in the image `other` -- (duv, score, status), the position in `other` being uv + duv."""
        from .displacements import displacements
        return displacements(self.read(), other.read(), uv, **kwargs)


def orthorectify(images, dem, viewshed, mask, method):
    """`Image.orthorectify` of `images` (checked by their `_check_orthorectify`, one pixel shape and dtype) as one array
    (images, dem rows, dem columns, channels), through one library call.  The caller's mask and the viewshed are combined
    here, one boolean per cell; with `viewshed=True` one viewshed is computed per distinct camera position (and
    elevation correction) among the images."""
    frames = [img._project_frame() for img in images]
    if len({(f.shape, f.dtype) for f in frames}) != 1:
        raise ValueError("Images differ in shape or dtype: " + str(sorted({(f.shape, str(f.dtype)) for f in frames})))
    array = np.asarray(dem.array)
    z = array if array.dtype == np.float32 else np.asarray(array, dtype=np.float64)  # (what xyz_to_uv makes of a cell)
    allowed = None if mask is None else np.asarray(mask, dtype=bool)
    seen = seen_of = None
    if isinstance(viewshed, (bool, np.bool_)):
        viewshed = True if viewshed else None  # (False: no visibility test either)
    if viewshed is True:
        masks, seen_of = {}, []
        for img in images:
            corr = img.cam.correction
            key = (tuple(img.cam.xyz), tuple(sorted(corr.items())) if isinstance(corr, dict) else bool(corr))
            if key not in masks:
                visible = dem.viewshed(img.cam.xyz, correction=corr)
                masks[key] = (len(masks), visible if allowed is None else visible & allowed)
            seen_of.append(masks[key][0])
        seen = np.stack([m for _, m in masks.values()])
    elif viewshed is not None:
        visible = np.asarray(viewshed, dtype=bool)
        seen = (visible if allowed is None else visible & allowed)[None]
    elif allowed is not None:
        seen = allowed[None]
    return _lib.stage_orthorectify(frames[0][None] if len(frames) == 1 else np.stack(frames),
                                   np.stack([img.cam.vector24 for img in images]), z, dem.x, dem.y, seen, seen_of, method)
