"""ctypes binding of libglimpse_hip.so (include/glimpse_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, every
entry point raises.  Build it with `python -m glimpse_amd.build` (hipcc, gfx950).
"""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GLH_LIB") or os.path.join(HERE, "lib", "libglimpse_hip.so")  # GLH_LIB: experimental builds

CAM_LEN = 24
MOTION_LEN = 18
MOTION_FULL_LEN = 24
MOTION_KINDS = {"cartesian": 0, "cylindrical": 1, "tangent_cartesian": 2, "tangent_cylindrical": 3, "external": 4}
RNG_HOST, RNG_PHILOX = 0, 1
MATH_EXACT, MATH_FAST = 0, 1
RESAMPLE = {"systematic": 0, "stratified": 1, "choice": 2, "residual": 3}
OK = 0
E_STATE = -4  # GLH_E_STATE (include/glimpse_hip.h); here: a call on a closed handle
PT_NAN, PT_TEMPLATE_OOB, PT_SAMPLE_OUTSIDE, PT_RESAMPLE_CLAMP, PT_CONST_TILE = 1, 2, 4, 8, 16
PT_RASTER_OOB, PT_NOT_VISIBLE = 32, 64
RASTER_DEM, RASTER_DEM_SIGMA, RASTER_VIEWSHED = 0, 1, 2
OBS_OK, OBS_SKIPPED, OBS_OUT_OF_BOUNDS, OBS_TILE_TOO_LARGE, OBS_NO_TEMPLATE = 0, 1, 2, 3, 4
NO_ERROR_FRAME = 0x7F7F7F7F
COMM_ID_BYTES = 128


class GlhError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libglimpse_hip error {code}: {message}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("device_id", C.c_int32),
        ("max_points", C.c_int32),
        ("max_particles", C.c_int32),
        ("n_observers", C.c_int32),
        ("max_tile", C.c_int32),
        ("max_search_dim", C.c_int32),
        ("max_frames", C.c_int32),
        ("reserved", C.c_int32),
    ]


_P = C.c_void_p
_I = C.c_int
_D = C.c_double
_U64 = C.c_uint64

# name -> (restype, argtypes); mirrors include/glimpse_hip.h one to one
SIGNATURES = {
    "glh_version": (_I, []),
    "glh_last_error": (C.c_char_p, []),
    "glh_device_count": (_I, [_P]),
    "glh_device_compute_units": (_I, [_I, _P]),
    "glh_device_memory": (_I, [_I, _P, _P]),
    "glh_create": (_I, [_P, _P]),
    "glh_destroy": (_I, [_P]),
    "glh_sync": (_I, [_P]),
    "glh_get_stream": (_I, [_P, _P]),
    "glh_observer_init": (_I, [_P, _I, _I, _I, _I, _I, _D]),
    "glh_observer_set_cameras": (_I, [_P, _I, _I, _I, _P]),
    "glh_observer_set_depth": (_I, [_P, _I, _I]),
    "glh_observer_upload_frame": (_I, [_P, _I, _I, _P]),
    "glh_observer_upload_frame_async": (_I, [_P, _I, _I, _P]),
    "glh_host_register": (_I, [_P, _U64]),
    "glh_host_unregister": (_I, [_P]),
    "glh_observer_upload_frame_pinned": (_I, [_P, _I, _I, _P, _P]),
    "glh_upload_done": (_I, [_P, C.c_int64, _I, _P]),
    "glh_observer_set_frame_device": (_I, [_P, _I, _I, _P]),
    "glh_begin_sequence": (_I, [_P, _I, _I, _I, _I]),
    "glh_set_motion_cartesian": (_I, [_P, _P]),
    "glh_set_motion": (_I, [_P, _P]),
    "glh_set_raster": (_I, [_P, _I, _P, _I, _I, _P, _P, _I, _I, _D, _D, _D, _D]),
    "glh_set_point_offset": (_I, [_P, _I]),
    "glh_set_observer_mask": (_I, [_P, _P]),
    "glh_set_active": (_I, [_P, _P]),
    "glh_set_particles": (_I, [_P, _P]),
    "glh_get_particles": (_I, [_P, _P]),
    "glh_set_weights": (_I, [_P, _P]),
    "glh_get_weights": (_I, [_P, _P]),
    "glh_set_extra_log_likelihoods": (_I, [_P, _P]),
    "glh_get_point_status": (_I, [_P, _P]),
    "glh_get_point_error_frame": (_I, [_P, _P]),
    "glh_get_observer_status": (_I, [_P, _P]),
    "glh_get_search_boxes": (_I, [_P, _P]),
    "glh_get_observer_status_frames": (_I, [_P, _I, _I, _P]),
    "glh_get_point_state": (_I, [_P, _I, _P, _P]),
    "glh_set_frame": (_I, [_P, _I]),
    "glh_init_particles": (_I, [_P, _I, _P, _U64]),
    "glh_evolve": (_I, [_P, _D, _I, _P, _U64, _U64]),
    "glh_init_templates": (_I, [_P, _I, _I]),
    "glh_update_weights": (_I, [_P, _P]),
    "glh_resample": (_I, [_P, _I, _P, _U64, _U64]),
    "glh_resample_method": (_I, [_P, _I, _I, _P, _U64, _U64]),
    "glh_get_residual_draws": (_I, [_P, _P]),
    "glh_record_covariances": (_I, [_P, _I]),
    "glh_get_covariances": (_I, [_P, _I, _I, _P]),
    "glh_record_moments": (_I, [_P, _I]),
    "glh_step": (_I, [_P, _I, _D, _P, _I, _P, _P, _U64]),
    "glh_track": (_I, [_P, _I, _P, _P, _P, _U64]),
    "glh_track_covariances": (_I, [_P, _I]),
    "glh_set_track_streams": (_I, [_P, _I]),
    "glh_set_fused": (_I, [_P, _I]),
    "glh_set_math": (_I, [_P, _I]),
    "glh_set_highpass": (_I, [_P, _I, _I]),
    "glh_set_highpass_mode": (_I, [_P, _I]),
    "glh_set_interpolation": (_I, [_P, _I, _I]),
    "glh_debug_phase_stamps": (_I, [_P, _P]),
    "glh_debug_draws": (_I, [_P, _I, _U64, _U64, _P]),
    "glh_debug_last_variant": (_I, [_P, _P]),
    "glh_debug_last_track_streams": (_I, [_P, _P]),
    "glh_get_moments": (_I, [_P, _I, _I, _P]),
    "glh_get_tracks": (_I, [_P, _I, _I, _P, _P]),
    "glh_get_moments_device": (_I, [_P, _P, _P]),
    "glh_get_template": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "glh_get_likelihood_debug": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "glh_set_debug": (_I, [_P, _I]),
    "glh_get_resample_indices": (_I, [_P, _P]),
    "glh_get_log_likelihoods": (_I, [_P, _I, _P]),
    "glh_profile_enable": (_I, [_P, _I]),
    "glh_profile_reset": (_I, [_P]),
    "glh_stage_count": (_I, []),
    "glh_stage_name": (C.c_char_p, [_I]),
    "glh_profile_get": (_I, [_P, _P, _P]),
    "glh_profile_get_launches": (_I, [_P, _I, _P, _I, _P]),
    "glh_profile_get_span": (_I, [_P, _I, _P]),
    "glh_comm_unique_id": (_I, [_P]),
    "glh_comm_init": (_I, [_P, _P, _I, _I]),
    "glh_comm_destroy": (_I, [_P]),
    "glh_comm_barrier": (_I, [_P]),
    "glh_comm_max_f64": (_I, [_P, _P]),
    "glh_gather_moments": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "glh_get_gathered": (_I, [_P, _P, _P]),
    "glh_measure_copy_bandwidth": (_I, [_P, _U64, _I, _P]),
    "glh_stage_project": (_I, [_I, _P, _P, _I, _P]),
    "glh_stage_project_directions": (_I, [_I, _P, _P, _I, _P]),
    "glh_stage_project_depth": (_I, [_I, _P, _P, _I, _I, _P, _P]),
    "glh_stage_project_fast": (_I, [_I, _P, _P, _I, _I, _I, _P]),
    "glh_stage_fast_math": (_I, [_I, _I, _P, _I, _P]),
    "glh_stage_unproject": (_I, [_I, _P, _P, _I, _P, _I, _I, _P]),
    "glh_stage_reproject": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P]),
    "glh_stage_template": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "glh_stage_search_tile": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _I, _P]),
    "glh_stage_template_highpass": (_I, [_I, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "glh_stage_search_tile_highpass": (_I, [_I, _P, _I, _I, _I, _P, _P, _P, _I, _I, _I, _I, _P]),
    "glh_stage_ssd": (_I, [_I, _P, _I, _I, _P, _I, _I, _P]),
    "glh_stage_sample": (_I, [_I, _P, _I, _I, _P, _P, _I, _P, _P]),
    "glh_stage_sample_orders": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P]),
    "glh_stage_resample": (_I, [_I, _P, _I, _D, _P]),
    "glh_stage_raster_sample": (_I, [_I, _P, _I, _I, _P, _P, _I, _I, _D, _D, _D, _D, _P, _I, _I, _P, _P]),
    "glh_stage_viewshed": (_I, [_I, _P, _I, _I, _I, _P, _P, _D, _P, _I, _I, _D, _D, _P, _P]),
    "glh_stage_horizon": (_I, [_I, _P, _I, _I, _I, _D, _D, _D, _D, _P, _P, _P, _I, _I, _I, _D, _D, _P, _P, _P]),
    "glh_stage_raster_regrid": (_I, [_I, _P, _P, _I, _P, _I, _P, _P]),
    "glh_stage_zoom_linear": (_I, [_I, _P, _I, _I, _I, _I, _P, _P]),
    "glh_stage_raster_interpolate": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _D, _D, _D, _D, _P, _P, _P]),
    "glh_stage_project_dem": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _P, _P, _I, _P, _P]),
    "glh_stage_rasterize": (_I, [_I, _P, _I, _P, _I, _I, _P, _P]),
    "glh_stage_orthorectify": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P, _P]),
    "glh_stage_raycast": (_I, [_I, _P, _I, _I, _I, _P, _P, _D, _D, _I, _P, _P, _I, _P, _I, _I, _I, _D, _D, _I, _P, _P, _P, _P,
                               _P]),
    "glh_stage_displacements": (_I, [_I, _P, _I, _I, _I, _I, _P, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P,
                                     _P]),
    "glh_stage_velocity_field": (_I, [_I, _P, _P, _P, _I, _I, _I, _I, _P, _D, _D, _D, _I, _I, _I, _D, _D, _I, _P, _P, _P, _P,
                                      _P]),
    "glh_stage_max_filter": (_I, [_I, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P]),
    "glh_stage_gaussian_filter": (_I, [_I, _P, _I, _I, _I, _P, _I, _P, _I, _P, _I, _I, _P, _P]),
    "glh_stage_fill_crevasses": (_I, [_I, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _P]),
    "glh_stage_clahe": (_I, [_I, _P, _I, _I, _I, _D, _I, _I, _P, _P, _P]),
    "glh_stage_gradient": (_I, [_I, _P, _I, _I, _I, _D, _D, _P, _P, _P]),
    "glh_stage_hillshade": (_I, [_I, _P, _I, _I, _I, _D, _D, _D, _P, _D, _P, _P]),
    "glh_stage_polygon_mask": (_I, [_I, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "glh_stage_uv_to_xy": (_I, [_I, _P, _P, _I, _P]),
    "glh_orient_create": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "glh_orient_eval": (_I, [_P, _P, _P, _P, _P, _P]),
    "glh_orient_destroy": (_I, [_P]),
    "glh_calib_create": (_I, [_I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "glh_calib_eval": (_I, [_P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P]),
    "glh_calib_fit_sets": (_I, [_P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I, C.c_double, C.c_double, C.c_double, _I,
                                C.c_double, _P, _P, _P, _P, _P]),
    "glh_calib_ransac_groups": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, C.c_double, C.c_double,
                                     C.c_double, C.c_double, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "glh_calib_ransac_groups_drawn": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _I, C.c_double,
                                           C.c_double, C.c_double, C.c_double, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                           C.c_uint32, C.c_uint32, _P, _P]),
    "glh_ransac_chunks": (_I, [_I, _P, _P, C.c_int64, _P, _P]),
    "glh_ransac_hypotheses": (_I, [_I, _P, _I, C.c_int64, _P, _P]),
    "glh_ransac_combinations": (_I, [C.c_int64, _I, C.c_int64, _P]),
    "glh_stage_ransac_samples": (_I, [_I, _I, _P, _P, _P, _I, C.c_uint32, C.c_uint32, _P, _P]),
    "glh_calib_destroy": (_I, [_P]),
    "glh_match_create": (_I, [_I, _P]),
    "glh_match_put": (_I, [_P, _I, _I, _I, _I, _P]),
    "glh_match_drop": (_I, [_P, _I]),
    "glh_match_knn2": (_I, [_P, _I, _I, _P, _P, _P]),
    "glh_match_destroy": (_I, [_P]),
    "glh_sift_create": (_I, [_I, _P]),
    "glh_sift_detect": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "glh_sift_read": (_I, [_P, _P, _P]),
    "glh_sift_counts": (_I, [_P, _P]),
    "glh_sift_layer": (_I, [_P, _I, _I, _I, _P]),
    "glh_sift_destroy": (_I, [_P]),
}

_lib = None


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GlhError(
            -100,
            f"{LIB_PATH} not found: the HIP library is required (no CPU fallback). "
            "Build it with `python -m glimpse_amd.build`.",
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and this table ever diverge
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != OK:
        raise GlhError(rc, load().glh_last_error().decode("utf-8", "replace"))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _arr(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected shape {tuple(shape)}, got {a.shape}")
    return a


def host_register(address, nbytes):
    """Page-lock `nbytes` of host memory at `address` for the device (hipHostRegister): uploads from it need no staging
    copy (Context.observer_upload_frame_pinned)."""
    check(load().glh_host_register(C.c_void_p(int(address)), int(nbytes)))


def host_unregister(address):
    check(load().glh_host_unregister(C.c_void_p(int(address))))


def device_count():
    n = C.c_int(0)
    check(load().glh_device_count(C.byref(n)))
    return n.value


def device_compute_units(device_id=0):
    n = C.c_int(0)
    check(load().glh_device_compute_units(int(device_id), C.byref(n)))
    return n.value


def device_memory(device_id=0):
    """(free, total) bytes of a device (hipMemGetInfo)."""
    free, total = C.c_uint64(0), C.c_uint64(0)
    check(load().glh_device_memory(int(device_id), C.byref(free), C.byref(total)))
    return free.value, total.value


def comm_unique_id():
    """128-byte RCCL communicator id (ncclGetUniqueId): made by one rank, handed to the others."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    check(load().glh_comm_unique_id(buf))
    return buf.raw


def stage_names():
    lib = load()
    return [lib.glh_stage_name(i).decode() for i in range(lib.glh_stage_count())]


class Context:
    """One device context = one GPU, one HIP stream, resident frames and particle state."""

    def __init__(self, max_points, max_particles, n_observers=1, device_id=0, max_tile=31,
                 max_search_dim=320, max_frames=128):
        self.lib = load()
        self.cfg = Config(device_id, max_points, max_particles, n_observers, max_tile, max_search_dim,
                          max_frames, 0)
        self.handle = C.c_void_p()
        check(self.lib.glh_create(C.byref(self.cfg), C.byref(self.handle)))
        self.O = n_observers
        self.P = self.N = 0
        self.tile = (0, 0)
        self.rank, self.world = 0, 1
        self._keep = []  # device-borrowed frame owners
        self._frame_shape = {}  # observer -> (height, width, channels) the library copies per frame
        self._frame_dtype = {}  # observer -> sample dtype (uint8, or uint16 after observer_set_depth)

    def close(self):
        if getattr(self, "handle", None):
            self.lib.glh_destroy(self.handle)
            self.handle = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- observers
    def observer_init(self, obs, n_images, width, height, channels, sigma):
        check(self.lib.glh_observer_init(self.handle, obs, n_images, width, height, channels, float(sigma)))
        self._frame_shape[obs] = (int(height), int(width), int(channels))
        self._frame_dtype[obs] = np.dtype(np.uint8)

    def set_interpolation(self, kx=3, ky=3):
        """Orders of the surface-sampling spline (rows axis, columns axis), each 1 .. 5; (3, 3) by default."""
        check(self.lib.glh_set_interpolation(self.handle, int(kx), int(ky)))

    def observer_set_depth(self, obs, dtype):
        """Sample type of the observer's frames: uint8 (default), uint16, float32 or float64 (one or three channels);
        before the first upload."""
        dtype = np.dtype(dtype)
        if dtype not in (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"frames are uint8, uint16, float32 or float64 (got {dtype})")
        check(self.lib.glh_observer_set_depth(self.handle, obs, 8 * dtype.itemsize))
        self._frame_dtype[obs] = dtype

    def _frame(self, obs, pixels):
        """The C side copies width * height * channels bytes: refuse anything that is not exactly that."""
        a = np.asarray(pixels)
        if a.dtype != self._frame_dtype[obs]:
            raise TypeError(f"observer {obs}: frames are {self._frame_dtype[obs]} (got {a.dtype}); the library never "
                            "casts pixel data")
        h, w, ch = self._frame_shape[obs]
        want = (h, w) if ch == 1 else (h, w, ch)
        if a.shape != want and not (ch == 1 and a.shape == (h, w, 1)):
            raise ValueError(f"observer {obs}: frame shape {a.shape} != {want} declared by observer_init")
        return np.ascontiguousarray(a)

    def observer_set_cameras(self, obs, cams, first=0):
        cams = _arr(cams, np.float64)
        assert cams.ndim == 2 and cams.shape[1] == CAM_LEN
        check(self.lib.glh_observer_set_cameras(self.handle, obs, first, len(cams), _ptr(cams)))

    def observer_upload_frame(self, obs, image, pixels):
        pixels = self._frame(obs, pixels)
        check(self.lib.glh_observer_upload_frame(self.handle, obs, image, _ptr(pixels)))

    def observer_upload_frame_async(self, obs, image, pixels):
        """Upload without waiting for the device; `pixels` may be reused as soon as the call returns."""
        pixels = self._frame(obs, pixels)
        check(self.lib.glh_observer_upload_frame_async(self.handle, obs, image, _ptr(pixels)))

    def observer_upload_frame_pinned(self, obs, image, pixels):
        """Upload straight from REGISTERED host memory (`host_register`): no staging copy.  Returns the ticket of the copy;
        `pixels` must stay untouched until `upload_done(ticket)`."""
        pixels = self._frame(obs, pixels)
        ticket = C.c_int64(0)
        check(self.lib.glh_observer_upload_frame_pinned(self.handle, obs, image, _ptr(pixels), C.byref(ticket)))
        return ticket.value

    def upload_done(self, ticket, wait=False):
        done = C.c_int(0)
        check(self.lib.glh_upload_done(self.handle, int(ticket), 1 if wait else 0, C.byref(done)))
        return bool(done.value)

    def observer_set_frame_device(self, obs, image, dev_ptr, owner=None):
        if owner is not None:
            self._keep.append(owner)
        check(self.lib.glh_observer_set_frame_device(self.handle, obs, image, C.c_void_p(dev_ptr)))

    # ---- sequence
    def begin_sequence(self, n_points, n_particles, tile_size):
        tw, th = int(tile_size[0]), int(tile_size[1])
        check(self.lib.glh_begin_sequence(self.handle, n_points, n_particles, tw, th))
        self.P, self.N, self.tile = n_points, n_particles, (tw, th)

    def set_motion_cartesian(self, params):
        params = _arr(params, np.float64, (self.P, MOTION_LEN))
        check(self.lib.glh_set_motion_cartesian(self.handle, _ptr(params)))

    def set_motion(self, params):
        """Any mix of motion models: [P][MOTION_FULL_LEN] (include/glimpse_hip.h)."""
        params = _arr(params, np.float64, (self.P, MOTION_FULL_LEN))
        check(self.lib.glh_set_motion(self.handle, _ptr(params)))

    def set_raster(self, which, raster):
        """Upload a glimpse_amd.Raster as the context's dem (0), dem_sigma (1) or viewshed (2); None removes it."""
        if raster is None:
            check(self.lib.glh_set_raster(self.handle, int(which), None, 0, 0, None, None, 1, 1, 0.0, 0.0, 0.0, 0.0))
            return
        z, nx, ny, gx, gy, sx, sy, x0, x1, y0, y1 = raster.device_args()
        check(self.lib.glh_set_raster(self.handle, int(which), _ptr(z), nx, ny, _ptr(gx), _ptr(gy), sx, sy, x0, x1,
                                      y0, y1))

    def set_observer_mask(self, mask):
        m = None if mask is None else _arr(mask, np.uint8, (self.P, self.O))
        check(self.lib.glh_set_observer_mask(self.handle, _ptr(m)))

    def set_active(self, active):
        a = None if active is None else _arr(active, np.uint8, (self.P,))
        check(self.lib.glh_set_active(self.handle, _ptr(a)))

    def set_particles(self, p):
        p = _arr(p, np.float64, (self.P, self.N, 6))
        check(self.lib.glh_set_particles(self.handle, _ptr(p)))

    def get_particles(self):
        out = np.empty((self.P, self.N, 6))
        check(self.lib.glh_get_particles(self.handle, _ptr(out)))
        return out

    def set_weights(self, w):
        w = _arr(w, np.float64, (self.P, self.N))
        check(self.lib.glh_set_weights(self.handle, _ptr(w)))

    def set_extra_log_likelihoods(self, ll):
        """A caller-computed log-likelihood term [P][N] for the next update_weights calls (None removes it)."""
        a = None if ll is None else _arr(ll, np.float64, (self.P, self.N))
        check(self.lib.glh_set_extra_log_likelihoods(self.handle, _ptr(a)))

    def get_weights(self):
        out = np.empty((self.P, self.N))
        check(self.lib.glh_get_weights(self.handle, _ptr(out)))
        return out

    def point_status(self):
        out = np.empty(self.P, dtype=np.uint32)
        check(self.lib.glh_get_point_status(self.handle, _ptr(out)))
        return out

    def point_error_frame(self):
        out = np.empty(self.P, dtype=np.int32)
        check(self.lib.glh_get_point_error_frame(self.handle, _ptr(out)))
        return out

    def observer_status(self):
        out = np.empty((self.O, self.P), dtype=np.int32)
        check(self.lib.glh_get_observer_status(self.handle, _ptr(out)))
        return out

    def observer_status_frames(self, frame0, n_frames):
        out = np.empty((n_frames, self.O, self.P), dtype=np.int32)
        check(self.lib.glh_get_observer_status_frames(self.handle, int(frame0), int(n_frames), _ptr(out)))
        return out

    def get_point_state(self, point):
        """(particles (N, 6), weights (N,)) of one point."""
        p, w = np.empty((self.N, 6)), np.empty(self.N)
        check(self.lib.glh_get_point_state(self.handle, int(point), _ptr(p), _ptr(w)))
        return p, w

    def search_boxes(self):
        out = np.empty((self.O, self.P, 4), dtype=np.int32)
        check(self.lib.glh_get_search_boxes(self.handle, _ptr(out)))
        return out

    # ---- stages
    def set_frame(self, frame):
        check(self.lib.glh_set_frame(self.handle, int(frame)))

    def init_particles(self, normals=None, seed=0):
        if normals is None:
            check(self.lib.glh_init_particles(self.handle, RNG_PHILOX, None, seed))
        else:
            n = _arr(normals, np.float64, (self.P, self.N, 6))
            check(self.lib.glh_init_particles(self.handle, RNG_HOST, _ptr(n), 0))

    def evolve(self, tau, normals=None, seed=0, step=0):
        if normals is None:
            check(self.lib.glh_evolve(self.handle, float(tau), RNG_PHILOX, None, seed, step))
        else:
            n = _arr(normals, np.float64, (self.P, self.N, 3))
            check(self.lib.glh_evolve(self.handle, float(tau), RNG_HOST, _ptr(n), 0, step))

    def init_templates(self, obs, image):
        check(self.lib.glh_init_templates(self.handle, obs, int(image)))

    def _images(self, images):
        im = np.array([-1 if i is None else int(i) for i in images], dtype=np.int32)
        assert im.shape == (self.O,)
        return im

    def update_weights(self, images):
        im = self._images(images)
        check(self.lib.glh_update_weights(self.handle, _ptr(im)))

    def resample(self, u=None, seed=0, step=0, method="systematic"):
        m = RESAMPLE[method]
        if u is None:
            check(self.lib.glh_resample_method(self.handle, m, RNG_PHILOX, None, seed, step))
        else:
            uu = _arr(u, np.float64, (self.P,) if m == 0 else (self.P, self.N))
            check(self.lib.glh_resample_method(self.handle, m, RNG_HOST, _ptr(uu), 0, step))

    def residual_draws(self):
        """Uniforms the last residual resampling consumed per point: n - sum(repetitions) (tracker.py:199-201)."""
        out = np.empty(self.P, dtype=np.int32)
        check(self.lib.glh_get_residual_draws(self.handle, _ptr(out)))
        return out

    def record_covariances(self, frame):
        check(self.lib.glh_record_covariances(self.handle, int(frame)))

    def get_covariances(self, frame0, n_frames):
        out = np.empty((n_frames, self.P, 6, 6))
        check(self.lib.glh_get_covariances(self.handle, frame0, n_frames, _ptr(out)))
        return out

    def record_moments(self, frame):
        check(self.lib.glh_record_moments(self.handle, int(frame)))

    def step(self, frame, tau, images, normals=None, u=None, seed=0):
        im = self._images(images)
        if normals is None:
            check(self.lib.glh_step(self.handle, int(frame), float(tau), _ptr(im), RNG_PHILOX, None, None, seed))
        else:
            n = _arr(normals, np.float64, (self.P, self.N, 3))
            uu = _arr(u, np.float64, (self.P,))
            check(self.lib.glh_step(self.handle, int(frame), float(tau), _ptr(im), RNG_HOST, _ptr(n), _ptr(uu), 0))

    def track(self, frames, taus, images, seed=0):
        """len(frames) consecutive `step` updates (device RNG) in one call: frames (T,), taus (T,), images (T, O)
        with -1 / None for "no image" (tracker.py:326-357)."""
        fr = np.ascontiguousarray(frames, dtype=np.int32).reshape(-1)
        ta = np.ascontiguousarray(taus, dtype=np.float64).reshape(-1)
        im = np.array([[-1 if v is None else int(v) for v in row] for row in images], dtype=np.int32)
        if ta.shape != fr.shape or im.shape != (len(fr), self.O):
            raise ValueError("frames (T,), taus (T,) and images (T, O) do not agree")
        check(self.lib.glh_track(self.handle, len(fr), _ptr(fr), _ptr(ta), _ptr(np.ascontiguousarray(im)), seed))

    def track_covariances(self, on=True):
        """`track` also records the covariances of every frame it runs (glh_track_covariances)."""
        check(self.lib.glh_track_covariances(self.handle, int(bool(on))))

    def set_track_streams(self, n):
        """Streams of `track`'s frame loop: 0 automatic, 1 one, 2 two (glh_set_track_streams)."""
        check(self.lib.glh_set_track_streams(self.handle, int(n)))

    def last_track_streams(self):
        n = C.c_int(0)
        check(self.lib.glh_debug_last_track_streams(self.handle, C.byref(n)))
        return n.value

    def set_fused(self, mode=1):
        """0 staged kernels, 1 fused per-point kernel (default), 2 fused with tiles forced to HBM (test)."""
        check(self.lib.glh_set_fused(self.handle, int(mode)))

    def set_math(self, mode="exact"):
        """"exact" (NumPy rounding; default) or "fast" (FMA / reciprocal arithmetic for device-RNG runs)."""
        check(self.lib.glh_set_math(self.handle, {"exact": MATH_EXACT, "fast": MATH_FAST}[mode]))

    def set_highpass(self, size=(5, 5), mode="reflect"):
        """Window of the median high-pass filter, scipy order (rows, columns); odd sizes up to 7.  `mode`: scipy.ndimage's
        boundary mode -- "reflect" (its default), "nearest", "mirror" or "wrap"."""
        sy, sx = (int(size), int(size)) if np.isscalar(size) else (int(size[0]), int(size[1]))
        check(self.lib.glh_set_highpass(self.handle, sx, sy))
        check(self.lib.glh_set_highpass_mode(self.handle, HIGHPASS_MODES[mode]))

    def set_point_offset(self, offset):
        check(self.lib.glh_set_point_offset(self.handle, int(offset)))

    def phase_stamps(self):
        """Diagnostic: s_memtime stamps (P, 24) of the fused kernel's phase boundaries (first call arms)."""
        out = np.zeros((self.P, 24), dtype=np.uint64)
        check(self.lib.glh_debug_phase_stamps(self.handle, _ptr(out)))
        return out

    def debug_draws(self, kind, seed, step=0):
        """The device stream's numbers: kind "init" (P, N, 6), "evolve" (P, N, 3) or "u" (P,) of frame `step`."""
        k = {"init": 0, "evolve": 1, "u": 2}[kind]
        shape = {0: (self.P, self.N, 6), 1: (self.P, self.N, 3), 2: (self.P,)}[k]
        out = np.empty(shape, dtype=np.float64)
        check(self.lib.glh_debug_draws(self.handle, k, int(seed), int(step), _ptr(out)))
        return out

    def last_variant(self):
        """Diagnostic: (threads, particles in registers, observers, flags) of the fused kernel instantiation that took
        the last fused step; flags bit 0 = fast arithmetic, bit 1 = the general code, bit 2 = the compile-time contract."""
        out = np.zeros(4, dtype=np.int32)
        check(self.lib.glh_debug_last_variant(self.handle, _ptr(out)))
        return tuple(int(v) for v in out)

    def sync(self):
        check(self.lib.glh_sync(self.handle))

    def stream(self):
        s = C.c_void_p()
        check(self.lib.glh_get_stream(self.handle, C.byref(s)))
        return s.value

    # ---- results
    def get_moments(self, frame0, n_frames):
        out = np.empty((n_frames, self.P, 12))
        check(self.lib.glh_get_moments(self.handle, frame0, n_frames, _ptr(out)))
        return out

    def get_tracks(self, frame0, n_frames):
        """The posterior history as Tracks holds it: means (P, n_frames, 6), sigmas (P, n_frames, 6)."""
        means, sigmas = np.empty((self.P, n_frames, 6)), np.empty((self.P, n_frames, 6))
        check(self.lib.glh_get_tracks(self.handle, frame0, n_frames, _ptr(means), _ptr(sigmas)))
        return means, sigmas

    def moments_device(self):
        p, n = C.c_void_p(), C.c_uint64()
        check(self.lib.glh_get_moments_device(self.handle, C.byref(p), C.byref(n)))
        return p.value, n.value

    def get_template(self, obs, point):
        tw, th = self.tile
        box = np.empty(4, dtype=np.int32)
        duv = np.empty(2)
        tile = np.empty((th, tw))
        hv = np.empty(tw * th)
        hq = np.empty(tw * th)
        hn = C.c_int32()
        check(self.lib.glh_get_template(self.handle, obs, point, _ptr(box), _ptr(duv), _ptr(tile), _ptr(hv),
                                        _ptr(hq), C.byref(hn)))
        return {"box": box, "duv": duv, "tile": tile, "histogram": (hv[: hn.value].copy(), hq[: hn.value].copy())}

    def set_debug(self, keep=True):
        """True / 1: SSE surfaces, log likelihoods and resample indices are kept (staged kernels); 2: indices only."""
        check(self.lib.glh_set_debug(self.handle, int(keep)))

    def likelihood_debug(self, obs, point, want_sse=True):
        """uv (N,2), box (4,) or None, search float32 (Hs,Ws), sse float64 (Ho,Wo)."""
        tw, th = self.tile
        uv = np.empty((self.N, 2))
        box = np.empty(4, dtype=np.int32)
        check(self.lib.glh_get_likelihood_debug(self.handle, obs, point, _ptr(uv), _ptr(box), None, None))
        if box[0] < 0:
            return {"uv": uv, "box": None}
        ws, hs = int(box[2] - box[0]), int(box[3] - box[1])
        search = np.empty((hs, ws), dtype=np.float32)
        sse = np.empty((hs - th + 1, ws - tw + 1)) if want_sse else None
        check(self.lib.glh_get_likelihood_debug(self.handle, obs, point, None, None, _ptr(search), _ptr(sse)))
        return {"uv": uv, "box": box, "search": search, "sse": sse}

    def log_likelihoods(self, obs):
        out = np.empty((self.P, self.N))
        check(self.lib.glh_get_log_likelihoods(self.handle, obs, _ptr(out)))
        return out

    def resample_indices(self):
        out = np.empty((self.P, self.N), dtype=np.int32)
        check(self.lib.glh_get_resample_indices(self.handle, _ptr(out)))
        return out

    def copy_bandwidth(self, nbytes=1 << 30, iters=10):
        """Measured device-to-device copy rate (read + write bytes per second, GB/s)."""
        out = C.c_double(0.0)
        check(self.lib.glh_measure_copy_bandwidth(self.handle, int(nbytes), int(iters), C.byref(out)))
        return out.value

    def profile_enable(self, on=True):
        check(self.lib.glh_profile_enable(self.handle, int(bool(on))))

    def profile_reset(self):
        check(self.lib.glh_profile_reset(self.handle))

    def profile_get(self):
        n = self.lib.glh_stage_count()
        ms = np.zeros(n)
        launches = np.zeros(n, dtype=np.int64)
        check(self.lib.glh_profile_get(self.handle, _ptr(ms), _ptr(launches)))
        return {name: (float(ms[i]), int(launches[i])) for i, name in enumerate(stage_names())}

    def profile_launches(self, stage):
        """Duration (ms) of every timed launch of `stage` (a name of stage_names()) since the last reset."""
        k = stage_names().index(stage)
        n = C.c_int(0)
        check(self.lib.glh_profile_get_launches(self.handle, k, None, 0, C.byref(n)))
        out = np.zeros(n.value)
        if n.value:
            check(self.lib.glh_profile_get_launches(self.handle, k, _ptr(out), n.value, C.byref(n)))
        return out

    def profile_span(self, stage):
        """GPU time (ms) from the start of the first timed launch of `stage` to the end of its last one since the last
        reset (launches on two streams overlap: their durations do not add up to it)."""
        ms = C.c_double(0.0)
        check(self.lib.glh_profile_get_span(self.handle, stage_names().index(stage), C.byref(ms)))
        return ms.value

    # ---- multi-GPU (RCCL behind the C ABI; glimpse_amd/sharding.py drives it)
    def comm_init(self, comm_id, rank, world):
        """Join the communicator made by `comm_unique_id()` on one rank (collective)."""
        if len(comm_id) != COMM_ID_BYTES:
            raise ValueError(f"comm_id must be {COMM_ID_BYTES} bytes")
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        check(self.lib.glh_comm_init(self.handle, buf, int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        check(self.lib.glh_comm_destroy(self.handle))

    def comm_barrier(self):
        check(self.lib.glh_comm_barrier(self.handle))

    def comm_max(self, value):
        v = C.c_double(float(value))
        check(self.lib.glh_comm_max_f64(self.handle, C.byref(v)))
        return v.value

    def gather_moments(self, frame0, n_frames, points_per_rank, root=0, download=True):
        """One RCCL exchange: on `root` returns (moments (n_frames, sum P, 12) in rank order, status (sum P,));
        None elsewhere.  download=False leaves the blocks on the root's device (returns None everywhere); `gathered()`
        fetches them later."""
        ppr = np.ascontiguousarray(points_per_rank, dtype=np.int32)
        if ppr.shape != (self.world,):
            raise ValueError("points_per_rank must have one entry per rank")
        self._gather_shape = (int(n_frames), [int(v) for v in ppr])
        check(self.lib.glh_gather_moments(self.handle, root, frame0, n_frames, _ptr(ppr), None, None))
        if self.rank != root or not download:
            return None
        return self.gathered()

    def gathered(self):
        """(moments (n_frames, sum P, 12), status (sum P,)) of the last gather_moments on the root."""
        n_frames, ppr = self._gather_shape
        total = sum(ppr)
        flat = np.empty(total * n_frames * 12)
        status = np.empty(total, dtype=np.uint32)
        check(self.lib.glh_get_gathered(self.handle, _ptr(flat), _ptr(status)))
        blocks, at = [], 0
        for pr in ppr:
            blocks.append(flat[at: at + pr * n_frames * 12].reshape(n_frames, pr, 12))
            at += pr * n_frames * 12
        return np.concatenate(blocks, axis=1), status

# ---- stateless stage hooks (parity tests) -----------------------------------------------
def stage_project(cam, xyz, device_id=0, directions=False):
    cam = _arr(cam, np.float64, (CAM_LEN,))
    xyz = _arr(xyz, np.float64)
    uv = np.empty((len(xyz), 2))
    fn = load().glh_stage_project_directions if directions else load().glh_stage_project
    check(fn(device_id, _ptr(cam), _ptr(xyz), len(xyz), _ptr(uv)))
    return uv


def stage_project_depth(cam, xyz, directions=False, device_id=0):
    cam = _arr(cam, np.float64, (CAM_LEN,))
    xyz = _arr(xyz, np.float64)
    uv = np.empty((len(xyz), 2))
    depth = np.empty(len(xyz))
    check(load().glh_stage_project_depth(device_id, _ptr(cam), _ptr(xyz), len(xyz), int(bool(directions)), _ptr(uv),
                                         _ptr(depth)))
    return uv, depth


def stage_project_fast(cam, xyz, directions=False, simple=False, device_id=0):
    """The projection of GLH_MATH_FAST on explicit points: project_fast, or project_simple_fast with simple=True."""
    cam = _arr(cam, np.float64, (CAM_LEN,))
    xyz = _arr(xyz, np.float64)
    uv = np.empty((len(xyz), 2))
    check(load().glh_stage_project_fast(device_id, _ptr(cam), _ptr(xyz), len(xyz), int(bool(directions)), int(bool(simple)),
                                        _ptr(uv)))
    return uv


# glh_stage_fast_math: the ops (GLH_FM_* of include/glimpse_hip.h) and how many columns each reads
FM_ARGS = 8
FM_OPS = {"RCP": (0, 1), "SQRT": (1, 1), "EXP": (2, 1), "WEIGHT": (3, 1), "MIN_NN": (4, 2), "MAX_NN": (5, 2),
          "COUNT_FRACTION": (6, 2), "COUNT_LE": (7, 4), "BILINEAR": (8, 6)}


def stage_fast_math(op, *columns, device_id=0):
    """One primitive of GLH_MATH_FAST on the device, one thread per row: `columns` are the op's arguments as equally
    long 1-D arrays (FM_OPS says how many), the result is a float64 array of that length."""
    code, n_cols = FM_OPS[op]
    if len(columns) != n_cols:
        raise ValueError(f"{op} takes {n_cols} argument columns, got {len(columns)}")
    cols = [_arr(c, np.float64) for c in columns]
    if any(c.ndim != 1 or c.shape != cols[0].shape for c in cols):
        raise ValueError("argument columns must be 1-D and equally long")
    args = np.zeros((len(cols[0]), FM_ARGS))
    for j, c in enumerate(cols):
        args[:, j] = c
    out = np.empty(len(args))
    check(load().glh_stage_fast_math(device_id, code, _ptr(args), len(args), _ptr(out)))
    return out


def stage_unproject(cam, uv, depth=None, directions=True, device_id=0):
    cam = _arr(cam, np.float64, (CAM_LEN,))
    uv = _arr(uv, np.float64)
    d = None if depth is None else _arr(np.atleast_1d(depth), np.float64)
    xyz = np.empty((len(uv), 3))
    check(load().glh_stage_unproject(device_id, _ptr(cam), _ptr(uv), len(uv), _ptr(d), 0 if d is None else len(d),
                                     int(bool(directions)), _ptr(xyz)))
    return xyz


def stage_uv_to_xy(cam, uv, device_id=0):
    """Camera._uv_to_xy (camera.py:1510-1519): uv (n, 2) -> normalised camera coordinates (n, 2)."""
    cam = _arr(cam, np.float64, (CAM_LEN,))
    uv = _arr(uv, np.float64)
    xy = np.empty((len(uv), 2))
    if len(uv):
        check(load().glh_stage_uv_to_xy(device_id, _ptr(cam), _ptr(uv), len(uv), _ptr(xy)))
    return xy


REPROJECT_METHODS = {"linear": 0, "nearest": 1}
REPROJECT_DTYPES = {"uint8": (8, 0), "uint16": (16, 0), "float32": (32, 1), "float64": (64, 1)}


def stage_reproject(frames, src_cams, dst_cam, dst_size, method="linear", device_id=0, return_kernel_ms=False):
    """Image.project (image.py:301-361) over a batch: `frames` (n, h, w, channels) of uint8 / uint16 / float32 / float64,
    one or three channels, each frame with its own camera `src_cams` (n, CAM_LEN), resampled into `dst_cam` (same
    position), `dst_size` = (width, height) -> (n, height, width, channels) of the frames' dtype.  One library call: the
    frames' copies overlap their neighbours' kernels.  `return_kernel_ms`: also the summed kernel time (HIP events)."""
    if method not in REPROJECT_METHODS:
        raise ValueError(f"Method '{method}' is not defined")
    frames = np.ascontiguousarray(frames)
    if frames.ndim != 4:
        raise ValueError("frames must be (n, rows, cols, channels)")
    if frames.dtype.name not in REPROJECT_DTYPES:
        raise TypeError(f"frames of dtype {frames.dtype}: uint8, uint16, float32 or float64")
    bits, is_float = REPROJECT_DTYPES[frames.dtype.name]
    n, h, w, ch = frames.shape
    src_cams = _arr(src_cams, np.float64, (n, CAM_LEN))
    dst_cam = _arr(dst_cam, np.float64, (CAM_LEN,))
    dw, dh = (int(v) for v in dst_size)
    out = np.empty((n, dh, dw, ch), dtype=frames.dtype)
    ms = C.c_double(0.0)
    check(load().glh_stage_reproject(device_id, _ptr(frames), bits, is_float, w, h, ch, n, _ptr(src_cams), _ptr(dst_cam),
                                     dw, dh, REPROJECT_METHODS[method], _ptr(out),
                                     C.byref(ms) if return_kernel_ms else None))
    return (out, ms.value) if return_kernel_ms else out


def _frame_dims(frame):
    frame = _arr(frame, np.uint8)
    h, w = frame.shape[:2]
    ch = 1 if frame.ndim == 2 else frame.shape[2]
    return frame, w, h, ch


# scipy.ndimage boundary modes of the median high-pass the device implements (glh_set_highpass_mode); the grid-* names are
# scipy's aliases
HIGHPASS_MODES = {"reflect": 0, "grid-mirror": 0, "nearest": 1, "mirror": 2, "wrap": 3, "grid-wrap": 3}


def _highpass_xy(size):
    return (int(size), int(size)) if np.isscalar(size) else (int(size[1]), int(size[0]))  # scipy: (rows, columns)


def stage_template(frame, box, device_id=0, highpass=(5, 5), mode="reflect"):
    frame, w, h, ch = _frame_dims(frame)
    sx, sy = _highpass_xy(highpass)
    box = _arr(box, np.int32, (4,))
    tw, th = int(box[2] - box[0]), int(box[3] - box[1])
    tile = np.empty((th, tw))
    hv = np.empty(tw * th)
    hq = np.empty(tw * th)
    hn = C.c_int32()
    check(load().glh_stage_template_highpass(device_id, _ptr(frame), w, h, ch, _ptr(box), sx, sy, HIGHPASS_MODES[mode],
                                             _ptr(tile), _ptr(hv), _ptr(hq), C.byref(hn)))
    return tile, (hv[: hn.value].copy(), hq[: hn.value].copy())


def stage_search_tile(frame, box, histogram, device_id=0, highpass=(5, 5), mode="reflect"):
    frame, w, h, ch = _frame_dims(frame)
    sx, sy = _highpass_xy(highpass)
    box = _arr(box, np.int32, (4,))
    hv = _arr(histogram[0], np.float64)
    hq = _arr(histogram[1], np.float64)
    out = np.empty((int(box[3] - box[1]), int(box[2] - box[0])), dtype=np.float32)
    check(load().glh_stage_search_tile_highpass(device_id, _ptr(frame), w, h, ch, _ptr(box), _ptr(hv), _ptr(hq),
                                                len(hv), sx, sy, HIGHPASS_MODES[mode], _ptr(out)))
    return out


def stage_ssd(search, templ, device_id=0):
    search = _arr(search, np.float32)
    templ = _arr(templ, np.float32)
    hs, ws = search.shape
    th, tw = templ.shape
    out = np.empty((hs - th + 1, ws - tw + 1), dtype=np.float32)
    check(load().glh_stage_ssd(device_id, _ptr(search), hs, ws, _ptr(templ), th, tw, _ptr(out)))
    return out


def stage_sample(sse, box, uv, device_id=0, orders=None):
    """Observer.sample_tile (observer.py:178-214) on the device: (values, outside).  `orders` = (kx, ky) of
    RectBivariateSpline (rows axis, columns axis); None: the bicubic default."""
    sse = _arr(sse, np.float32)
    box = _arr(box, np.float64, (4,))
    uv = _arr(uv, np.float64)
    values = np.empty(len(uv))
    outside = np.empty(len(uv), dtype=np.uint8)
    if orders is None:
        check(load().glh_stage_sample(device_id, _ptr(sse), sse.shape[0], sse.shape[1], _ptr(box), _ptr(uv), len(uv),
                                      _ptr(values), _ptr(outside)))
    else:
        check(load().glh_stage_sample_orders(device_id, _ptr(sse), sse.shape[0], sse.shape[1], int(orders[0]),
                                             int(orders[1]), _ptr(box), _ptr(uv), len(uv), _ptr(values), _ptr(outside)))
    return values, outside.astype(bool)


def stage_resample(weights, u, device_id=0):
    w = _arr(weights, np.float64)
    idx = np.empty(len(w), dtype=np.int64)
    check(load().glh_stage_resample(device_id, _ptr(w), len(w), float(u), _ptr(idx)))
    return idx


def stage_raster_sample(raster, xy, order=1, device_id=0):
    z, nx, ny, gx, gy, sx, sy, x0, x1, y0, y1 = raster.device_args()
    xy = _arr(xy, np.float64)
    vals = np.empty(len(xy))
    oob = np.empty(len(xy), dtype=np.uint8)
    check(load().glh_stage_raster_sample(device_id, _ptr(z), nx, ny, _ptr(gx), _ptr(gy), sx, sy, x0, x1, y0, y1,
                                         _ptr(xy), len(xy), int(order), _ptr(vals), _ptr(oob)))
    return vals, oob.astype(bool)


# the dtype flag of a float array: GLH_VIEWSHED_*, GLH_PD_*, GLH_FILTER_* and GLH_TERRAIN_* of the header number them alike
F64, F32 = 0, 1
VIEWSHED_F64, VIEWSHED_F32 = F64, F32


def _timed(result, names, times, return_times, extend=False):
    """What a stage returns: `result`, and with `return_times` the dict of `names` -> the leading `times` after it
    (`extend`: as one more item of the tuple `result`)."""
    if not return_times:
        return result
    split = dict(zip(names, (float(t) for t in times)))
    return (*result, split) if extend else (result, split)


def _float_array(a):
    """(a, dtype flag, nx, ny) of `a` (ny, nx) float64 / float32 as a stage takes it; the callers in glimpse_amd check and
    widen what their caller gave."""
    if a.dtype not in (np.dtype(np.float64), np.dtype(np.float32)) or a.ndim != 2:
        raise TypeError(f"a two-dimensional float64 or float32 array (got {a.dtype}, {a.ndim} dimensions)")
    a = np.ascontiguousarray(a)
    return a, F32 if a.dtype == np.float32 else F64, a.shape[1], a.shape[0]


VIEWSHED_TIMES = ("upload_ms", "cells_ms", "sort_ms", "sweep_ms", "download_ms", "rings", "launches", "sort_scratch_bytes")


def viewshed_correction(correction):
    """`correction` of Raster.viewshed (raster.py:1322-1325) -> (on, radius, refraction): False / None skip it, True takes
    the defaults of helpers.elevation_corrections (helpers.py:1771-1773), a dict its keyword arguments (another key is the
    TypeError the reference's call would raise)."""
    def elevation_corrections(radius=6.3781e6, refraction=0.13):
        return True, float(radius), float(refraction)

    if correction is True:
        correction = {}
    if isinstance(correction, dict):
        return elevation_corrections(**correction)
    return False, 6.3781e6, 0.13


def viewshed_dem(array, origin_z):
    """The DEM as the kernel takes it, (z, dtype flag).  The reference forms `array.ravel() - origin[2]` in whatever dtype
    NumPy promotes to (raster.py:1320) -- for a float32 DEM that depends on what kind of scalar origin[2] is -- so the
    promotion is asked of NumPy itself, on one element: float32 stays float32 (the subtraction and the correction's sum
    are then rounded to float32 on the device too), everything else is computed in float64 (integers convert exactly)."""
    array = np.asarray(array)
    if array.dtype.kind not in "iuf" or array.dtype.itemsize > 8 or array.dtype == np.float16:
        raise TypeError(f"a DEM of dtype {array.dtype}: float64, float32 or integers")
    probe = (array.ravel()[:1] - origin_z).dtype
    if probe == np.float32:
        return np.ascontiguousarray(array, dtype=np.float32), VIEWSHED_F32
    if probe.kind not in "iuf" or probe.itemsize > 8 or probe == np.float16:
        raise TypeError(f"a DEM of dtype {array.dtype} less an origin of type {type(origin_z).__name__} is {probe}")
    return np.ascontiguousarray(array, dtype=np.float64), VIEWSHED_F64


def _dem_and_origins(raster, origins, float32):
    """(z, dtype flag, origins) of stage_viewshed and stage_horizon: the DEM of `raster` in the dtype `float32` decides
    (None: viewshed_dem asks NumPy with the first origin's z), and the (m, 3) positions as float64."""
    origins = np.asarray(origins)
    if origins.ndim != 2 or origins.shape[1] != 3 or len(origins) < 1:
        raise ValueError(f"origins must be (m, 3) with m >= 1, got {origins.shape}")
    if float32 is None:
        z, flag = viewshed_dem(raster.array, origins[0, 2])
    else:
        z = np.ascontiguousarray(raster.array, dtype=np.float32 if float32 else np.float64)
        flag = VIEWSHED_F32 if float32 else VIEWSHED_F64
    if z.ndim != 2:
        raise ValueError(f"a DEM is two-dimensional, got {z.shape}")
    return z, flag, _arr(origins, np.float64)


def stage_viewshed(raster, origins, correction=None, device_id=0, return_times=False, float32=None):
    """Raster.viewshed (raster.py:1293-1389) of `raster` from the m positions `origins` (m, 3): bool (m, ny, nx).  The DEM
    is uploaded once and the m viewsheds are computed one after another.  `float32`: whether the reference's dz would be
    float32 (None: NumPy's promotion of the DEM with `origins`' own scalar type is asked; Raster.viewshed asks with the
    caller's origin[2], which may be a Python float).  `return_times`: also a dict of the HIP-event split, summed over the
    origins (VIEWSHED_TIMES)."""
    on, radius, refraction = viewshed_correction(correction)
    z, flag, origins = _dem_and_origins(raster, origins, float32)
    ny, nx = z.shape
    x, y = _arr(raster.x, np.float64, (nx,)), _arr(raster.y, np.float64, (ny,))
    out = np.empty((len(origins), ny, nx), dtype=np.uint8)
    times = np.zeros(len(VIEWSHED_TIMES))
    check(load().glh_stage_viewshed(device_id, _ptr(z), flag, nx, ny, _ptr(x), _ptr(y), float(1 / abs(raster.d[0])),
                                    _ptr(origins), len(origins), int(on), radius, refraction, _ptr(out),
                                    _ptr(times) if return_times else None))
    return _timed(out.view(bool), VIEWSHED_TIMES, times, return_times)


HORIZON_TIMES = ("upload_ms", "kernel_ms", "download_ms")


def stage_horizon(raster, origins, starts, ends, correction=None, device_id=0, return_times=False, float32=None):
    """The device part of Raster.horizon (raster.py:1435-1458) for the m positions `origins` (m, 3) over one upload of the
    DEM: `starts` (m, 2) the (col, row) of each origin's cell, `ends` (m, n, 2) the (col, row) where each of its n rays
    leaves the grid.  Returns (cell (m, n, 2) int32 (row, col), -1 where a heading has no horizon point; dz (m, n) of the
    chosen cells, NaN there).  `float32`: whether dz stays float32, which depends on the type of the caller's origin
    (Raster.horizon passes viewshed_dem's answer for it); None decides from `origins` as an array, a float64 one unless
    the caller made it otherwise, so a float32 DEM is then widened.  `return_times`: also a dict of HORIZON_TIMES."""
    on, radius, refraction = viewshed_correction(correction)
    z, flag, origins = _dem_and_origins(raster, origins, float32)
    m = len(origins)
    starts = _arr(starts, np.int32, (m, 2))
    ends = _arr(ends, np.int32)
    if ends.ndim != 3 or ends.shape[0] != m or ends.shape[2] != 2 or ends.shape[1] < 1:
        raise ValueError(f"ends must be ({m}, n, 2) with n >= 1, got {ends.shape}")
    n = ends.shape[1]
    ny, nx = z.shape
    d = raster.d
    cell = np.empty((m, n, 2), dtype=np.int32)
    dz = np.empty((m, n), dtype=np.float64)
    times = np.zeros(len(HORIZON_TIMES))
    check(load().glh_stage_horizon(device_id, _ptr(z), flag, nx, ny, float(raster.xlim[0]), float(raster.ylim[0]),
                                   float(d[0]), float(d[1]), _ptr(origins), _ptr(starts), _ptr(ends), m, n, int(on), radius,
                                   refraction, _ptr(cell), _ptr(dz), _ptr(times) if return_times else None))
    return _timed((cell, dz), HORIZON_TIMES, times, return_times, extend=True)


REGRID_TIMES = ("upload_ms", "solve_ms", "evaluate_ms", "download_ms")
INTERPOLATE_TIMES = ("upload_ms", "regrid_ms", "blend_ms", "download_ms")


class RegridSrc(C.Structure):
    """glh_regrid_src (include/glimpse_hip.h)."""
    _fields_ = [("z", _P), ("nan_mask", _P), ("nx", C.c_int32), ("ny", C.c_int32), ("gx", _P), ("gy", _P),
                ("xmin", _D), ("xmax", _D), ("ymin", _D), ("ymax", _D), ("kx", C.c_int32), ("ky", C.c_int32),
                ("use_zmin", C.c_int32), ("flip_x", C.c_int32), ("flip_y", C.c_int32), ("reserved", C.c_int32), ("zmin", _D)]


def regrid_src(z, gx, gy, box, kx, ky, nan_mask=None, zmin=None, flip_x=False, flip_y=False):
    """(glh_regrid_src, the arrays it points into -- keep them alive for the call).  z (ny, nx) with ascending axes and no
    NaN (0 under `nan_mask`); gx, gy the ascending cell centres; box = (xmin, xmax, ymin, ymax)."""
    z = _arr(z, np.float64)
    if z.ndim != 2:
        raise ValueError(f"a raster is two-dimensional, got {z.shape}")
    ny, nx = z.shape
    gx, gy = _arr(gx, np.float64, (nx,)), _arr(gy, np.float64, (ny,))
    if nan_mask is not None:
        nan_mask = _arr(nan_mask, np.uint8, (ny, nx))
    use_zmin = zmin is not None and not np.isnan(zmin)
    src = RegridSrc(_ptr(z), _ptr(nan_mask), nx, ny, _ptr(gx), _ptr(gy), float(box[0]), float(box[1]), float(box[2]),
                    float(box[3]), int(kx), int(ky), int(use_zmin), int(bool(flip_x)), int(bool(flip_y)), 0,
                    float(zmin) if use_zmin else 0.0)
    return src, (z, gx, gy, nan_mask)


def stage_raster_regrid(src, xo, yo, device_id=0, return_times=False):
    """glh_stage_raster_regrid: the spline of `src` (regrid_src's pair) on the ascending vectors xo (mx,), yo (my,):
    float64 (my, mx).  `return_times`: also a dict of REGRID_TIMES."""
    struct, keep = src
    xo, yo = _arr(xo, np.float64), _arr(yo, np.float64)
    if xo.ndim != 1 or yo.ndim != 1:
        raise ValueError(f"xo and yo are vectors, got {xo.shape} and {yo.shape}")
    out = np.empty((len(yo), len(xo)), dtype=np.float64)
    times = np.zeros(len(REGRID_TIMES))
    check(load().glh_stage_raster_regrid(device_id, C.byref(struct), _ptr(xo), len(xo), _ptr(yo), len(yo), _ptr(out),
                                         _ptr(times) if return_times else None))
    del keep
    return _timed(out, REGRID_TIMES, times, return_times)


def stage_zoom_linear(a, shape, device_id=0, return_times=False):
    """glh_stage_zoom_linear: scipy.ndimage.zoom(a, zoom, order=1) of float64 `a` into `shape` = (my, mx)."""
    a = _arr(a, np.float64)
    if a.ndim != 2:
        raise ValueError(f"a raster is two-dimensional, got {a.shape}")
    my, mx = (int(v) for v in shape)
    if my < 1 or mx < 1:
        raise ValueError(f"the zoomed shape {(my, mx)} has no cells")
    out = np.empty((my, mx), dtype=np.float64)
    times = np.zeros(len(REGRID_TIMES))
    check(load().glh_stage_zoom_linear(device_id, _ptr(a), a.shape[1], a.shape[0], mx, my, _ptr(out),
                                       _ptr(times) if return_times else None))
    return _timed(out, REGRID_TIMES, times, return_times)


def stage_raster_interpolate(m0, m1, scale, scale2, ratio, s0=None, s1=None, xo=None, yo=None, device_id=0,
                             return_times=False):
    """glh_stage_raster_interpolate: (z, sigma or None) of RasterInterpolant._interpolate.  m0, s0: (ny, nx) arrays; m1, s1:
    arrays of that shape, or regrid_src pairs to be regridded at order 1 onto the ascending centres xo (nx,), yo (ny,).
    `scale2` = scale ** 2 and `ratio` = nearest_dx / dx as the caller's Python made them."""
    m0 = _arr(m0, np.float64)
    if m0.ndim != 2:
        raise ValueError(f"a raster is two-dimensional, got {m0.shape}")
    ny, nx = m0.shape

    def second(v):
        if isinstance(v, tuple):
            return None, v
        return _arr(v, np.float64, (ny, nx)), None

    m1, m1_src = second(m1)
    with_sigma = s0 is not None
    s1, s1_src = second(s1) if with_sigma else (None, None)
    s0 = _arr(s0, np.float64, (ny, nx)) if with_sigma else None
    if m1_src is not None or s1_src is not None:
        xo, yo = _arr(xo, np.float64, (nx,)), _arr(yo, np.float64, (ny,))
    else:
        xo = yo = None
    z = np.empty((ny, nx), dtype=np.float64)
    sigma = np.empty((ny, nx), dtype=np.float64) if with_sigma else None
    times = np.zeros(len(INTERPOLATE_TIMES))
    check(load().glh_stage_raster_interpolate(
        device_id, nx, ny, _ptr(m0), _ptr(m1), C.byref(m1_src[0]) if m1_src else None, _ptr(s0), _ptr(s1),
        C.byref(s1_src[0]) if s1_src else None, _ptr(xo), _ptr(yo), float(scale), float(scale2), 1 / 3, float(ratio), _ptr(z),
        _ptr(sigma), _ptr(times) if return_times else None))
    return _timed((z, sigma), INTERPOLATE_TIMES, times, return_times, extend=True)


PD_F64, PD_F32, PD_U8, PD_U16 = F64, F32, 2, 3
PD_DTYPES = {"float64": PD_F64, "float32": PD_F32, "uint8": PD_U8, "uint16": PD_U16}
PD_TIMES = ("upload_ms", "project_ms", "order_ms", "reduce_ms", "download_ms", "memberships", "kept", "sort_scratch_bytes")


def stage_project_dem(cam, z, values, mask, cols, x_coords, rows, y_coords, return_depth=False, device_id=0,
                      return_times=False):
    """Camera.project_dem (camera.py:967-1129) for the camera vector `cam` (CAM_LEN): float64 (height, width, layers +
    return_depth).  `z` (ny, nx): the DEM, float32 as it is, anything else as float64.  `values` (ny, nx, layers) or None:
    float64, float32, uint8, uint16 travel as they are, bool as uint8, anything else as the float64 np.bincount would
    make of it.  `mask` (ny, nx) or None.  `cols` / `rows`: the (start, stop) of the tiling's column / row slices
    (Raster.tile_indices), `x_coords` / `y_coords`: each slice's own coordinates, one slice after another.
    `return_times`: also a dict of the HIP-event split (PD_TIMES)."""
    cam = _arr(cam, np.float64, (CAM_LEN,))
    z = np.asarray(z)
    z = np.ascontiguousarray(z, dtype=np.float32 if z.dtype == np.float32 else np.float64)
    ny, nx = z.shape
    layers, code = 0, PD_F64
    if values is not None:
        values = np.asarray(values)
        if values.dtype == bool:
            values = values.view(np.uint8)
        if values.dtype.name not in PD_DTYPES:
            values = values.astype(np.float64)
        values = _arr(values, values.dtype, (ny, nx, values.shape[2]))
        layers, code = values.shape[2], PD_DTYPES[values.dtype.name]
    if mask is not None:
        mask = _arr(np.asarray(mask, dtype=bool), bool, (ny, nx)).view(np.uint8)
    xs, xe = (_arr([c[k] for c in cols], np.int32) for k in (0, 1))
    ys, ye = (_arr([r[k] for r in rows], np.int32) for k in (0, 1))
    x_coords = _arr(x_coords, np.float64, (int((xe - xs).sum()),))
    y_coords = _arr(y_coords, np.float64, (int((ye - ys).sum()),))
    width, height = int(cam[6]), int(cam[7])
    out = np.empty((height, width, layers + int(bool(return_depth))))
    times = np.zeros(len(PD_TIMES))
    check(load().glh_stage_project_dem(device_id, _ptr(cam), _ptr(z), PD_F32 if z.dtype == np.float32 else PD_F64, nx, ny,
                                       _ptr(mask), _ptr(values), code, layers, len(xs), _ptr(xs), _ptr(xe), _ptr(x_coords),
                                       len(ys), _ptr(ys), _ptr(ye), _ptr(y_coords), int(bool(return_depth)), _ptr(out),
                                       _ptr(times) if return_times else None))
    return _timed(out, PD_TIMES, times, return_times)


def stage_rasterize(keys, values, n_pixels, device_id=0, return_times=False):
    """helpers.rasterize_points (helpers.py:1617-1698) on the device: `keys` (n,) the pixel of every point, each in
    [0, n_pixels), `values` (n, d) -> float64 (n_pixels, d) of per-pixel means (the sum in the points' order, times
    1 / count), NaN where no point falls."""
    keys = _arr(keys, np.int32)
    values = _arr(values, np.float64, (len(keys), np.shape(values)[1]))
    out = np.empty((int(n_pixels), values.shape[1]))
    times = np.zeros(len(PD_TIMES))
    check(load().glh_stage_rasterize(device_id, _ptr(keys), len(keys), _ptr(values), values.shape[1], int(n_pixels),
                                     _ptr(out), _ptr(times) if return_times else None))
    return _timed(out, PD_TIMES, times, return_times)


def stage_orthorectify(frames, cams, z, x, y, seen=None, seen_of=None, method="linear", device_id=0,
                       return_kernel_ms=False):
    """Image.orthorectify over a batch: `frames` (n, h, w, channels) of uint8 / uint16 / float32 / float64, one or three
    channels, each frame with its own camera `cams` (n, CAM_LEN), resampled onto the DEM `z` (ny, nx) float64 / float32
    with the cell centres `x` (nx,), `y` (ny,) -> (n, ny, nx, channels), float32 for float32 frames and float64 for every
    other, NaN where a cell is not seen.  `seen`: None, or (m, ny, nx) masks (the caller's mask and viewshed of a cell)
    with `seen_of` (n,) naming each frame's (None: the first).  One library call: the DEM and the masks are uploaded once
    and the frames' copies overlap their neighbours' kernels.  `return_kernel_ms`: also the summed kernel time (HIP
    events)."""
    if method not in REPROJECT_METHODS:
        raise ValueError(f"Method '{method}' is not defined")
    frames = np.ascontiguousarray(frames)
    if frames.ndim != 4:
        raise ValueError("frames must be (n, rows, cols, channels)")
    if frames.dtype.name not in REPROJECT_DTYPES:
        raise TypeError(f"frames of dtype {frames.dtype}: uint8, uint16, float32 or float64")
    bits, is_float = REPROJECT_DTYPES[frames.dtype.name]
    n, h, w, ch = frames.shape
    cams = _arr(cams, np.float64, (n, CAM_LEN))
    z, flag, nx, ny = _float_array(np.asarray(z))
    x, y = _arr(x, np.float64, (nx,)), _arr(y, np.float64, (ny,))
    if seen is not None:
        seen = _arr(seen, np.uint8)
        if seen.ndim != 3 or seen.shape[1:] != (ny, nx) or len(seen) < 1:
            raise ValueError(f"seen must be (m, {ny}, {nx}) with m >= 1, got {seen.shape}")
        if seen_of is not None:
            seen_of = _arr(seen_of, np.int32, (n,))
    elif seen_of is not None:
        raise ValueError("seen_of without seen")
    out = np.empty((n, ny, nx, ch), dtype=np.float32 if frames.dtype == np.float32 else np.float64)
    ms = C.c_double(0.0)
    check(load().glh_stage_orthorectify(device_id, _ptr(frames), bits, is_float, w, h, ch, n, _ptr(cams), _ptr(z), flag, nx,
                                        ny, _ptr(x), _ptr(y), _ptr(seen), 0 if seen is None else len(seen), _ptr(seen_of),
                                        REPROJECT_METHODS[method], _ptr(out), C.byref(ms) if return_kernel_ms else None))
    return (out, ms.value) if return_kernel_ms else out


RAYCAST_TIMES = ("upload_ms", "pyramid_ms", "march_ms", "download_ms")
RAYCAST_DIRECTIONS, RAYCAST_UV, RAYCAST_GRID = 0, 1, 2
RAYCAST_STATUS = ("hit", "misses the domain", "enters below the surface", "leaves without a hit", "invalid")


def stage_raycast(z, x, y, d, origins=None, directions=None, cam=None, uv=None, step=None, correction=None, block=16,
                  device_id=0, return_times=False):
    """Rays cast onto the bilinear surface between the cell centres `x` (nx,), `y` (ny,) of the DEM `z` (ny, nx) float64 /
    float32, `d` its signed cell sizes (INPUTS.md, "Ray casting: the rule").  The rays are `directions` (n, 3) from
    `origins` (3,) or (n, 3); or the image coordinates `uv` (n, 2) of the camera `cam` (CAM_LEN,), unprojected on the
    device; or, with `step`, the camera's pixel centres step / 2 + k step, made on the device in row-major order.
    `correction`: None / False, True or the arguments of helpers.elevation_corrections.  `block`: 0 marches every patch,
    a power of two lets rays skip blocks of that many patches a side (the results do not depend on it).  Returns
    (t (n,), xyz (n, 3), patch (n,) int32, status (n,) uint8 indexing RAYCAST_STATUS); `return_times`: also a dict of
    RAYCAST_TIMES."""
    on, radius, refraction = viewshed_correction(correction)
    z, flag, nx, ny = _float_array(np.asarray(z))
    x, y = _arr(x, np.float64, (nx,)), _arr(y, np.float64, (ny,))
    block = int(block)
    if block < 0 or block & (block - 1):
        raise ValueError(f"block is 0 or a power of two, got {block}")
    if (directions is not None) + (uv is not None) + (step is not None) != 1:
        raise ValueError("one of directions, uv and step names the rays")
    rays = cam24 = None
    n_origins = 1
    if directions is not None:
        mode, rays = RAYCAST_DIRECTIONS, _arr(directions, np.float64)
        if rays.ndim != 2 or rays.shape[1] != 3 or len(rays) < 1:
            raise ValueError(f"directions must be (n, 3) with n >= 1, got {rays.shape}")
        origins = _arr(np.atleast_2d(np.asarray(origins, dtype=np.float64)), np.float64)
        if origins.shape not in ((1, 3), (len(rays), 3)):
            raise ValueError(f"origins must be (3,) or ({len(rays)}, 3), got {origins.shape}")
        n, n_origins = len(rays), len(origins)
    else:
        cam24, origins = _arr(cam, np.float64, (CAM_LEN,)), None
        if uv is not None:
            mode, rays = RAYCAST_UV, _arr(uv, np.float64)
            if rays.ndim != 2 or rays.shape[1] != 2 or len(rays) < 1:
                raise ValueError(f"uv must be (n, 2) with n >= 1, got {rays.shape}")
            n = len(rays)
        else:
            mode, step = RAYCAST_GRID, int(step)
            if step < 1:
                raise ValueError(f"step must be at least 1, got {step}")
            n = (int(cam24[6]) // step) * (int(cam24[7]) // step)
            if n < 1:
                raise ValueError(f"step {step} leaves no pixel of an image of {int(cam24[6])} x {int(cam24[7])}")
    t, xyz = np.empty(n), np.empty((n, 3))
    patch, status = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.uint8)
    times = np.zeros(len(RAYCAST_TIMES))
    check(load().glh_stage_raycast(device_id, _ptr(z), flag, nx, ny, _ptr(x), _ptr(y), float(d[0]), float(d[1]), mode,
                                   _ptr(cam24), _ptr(origins), n_origins, _ptr(rays), n, step or 0, int(on), radius,
                                   refraction, block, _ptr(t), _ptr(xyz), _ptr(patch), _ptr(status),
                                   _ptr(times) if return_times else None))
    return _timed((t, xyz, patch, status), RAYCAST_TIMES, times, return_times, extend=True)


DISPLACEMENTS_TIMES = ("upload_ms", "kernel_ms", "download_ms")
DISPLACEMENT_STATUS = ("matched", "peak on the edge", "no valid offset", "flat template", "template outside")
DISPLACEMENT_GUESS_LIMIT = 1 << 24  # whole pixels; beyond it no window of any frame the library takes is inside


def stage_displacements(frames, pairs, corners, valid, guess, size, reach, subpixel=True, return_surface=False,
                        device_id=0, return_times=False):
    """Dense template matching (INPUTS.md, "Displacements: the rule"): `frames` (F, h, w) uint8 (the integer path) or
    float32; `pairs` (P, 2) int32, the frame a pair's templates are cut from and the frame they are looked for in;
    `corners` (n, 2) int32, the (l, t) of each template box, with `valid` (n,) 0 where the box leaves the frame; `guess`
    None, or whole pixels (n, 2) / (P, n, 2) int32; `size` = (w, h) of the template, `reach` = (rx, ry).  Returns
    (duv (P, n, 2), score (P, n), status (P, n) uint8 indexing DISPLACEMENT_STATUS), with `return_surface` also the
    scores of every offset (P, n, 2 ry + 1, 2 rx + 1), with `return_times` also a dict of DISPLACEMENTS_TIMES."""
    frames = np.ascontiguousarray(frames)
    if frames.ndim != 3 or frames.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
        raise TypeError(f"frames (F, rows, cols) of uint8 or float32 (got {frames.dtype}, {frames.ndim} dimensions)")
    pairs = _arr(pairs, np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or len(pairs) < 1:
        raise ValueError(f"pairs must be (P, 2) with P >= 1, got {pairs.shape}")
    corners = _arr(corners, np.int32)
    if corners.ndim != 2 or corners.shape[1] != 2 or len(corners) < 1:
        raise ValueError(f"corners must be (n, 2) with n >= 1, got {corners.shape}")
    n, p = len(corners), len(pairs)
    valid = _arr(valid, np.uint8, (n,))
    per_pair = 0
    if guess is not None:
        guess = _arr(guess, np.int32)
        if guess.shape not in ((n, 2), (p, n, 2)):
            raise ValueError(f"guess must be ({n}, 2) or ({p}, {n}, 2), got {guess.shape}")
        per_pair = int(guess.ndim == 3)
    (w, h), (rx, ry) = (int(v) for v in size), (int(v) for v in reach)
    duv, score = np.empty((p, n, 2)), np.empty((p, n))
    status = np.empty((p, n), dtype=np.uint8)
    surface = np.empty((p, n, 2 * ry + 1, 2 * rx + 1)) if return_surface else None
    times = np.zeros(len(DISPLACEMENTS_TIMES))
    check(load().glh_stage_displacements(device_id, _ptr(frames), int(frames.dtype == np.float32), frames.shape[2],
                                         frames.shape[1], frames.shape[0], _ptr(pairs), p, _ptr(corners), _ptr(valid), n,
                                         _ptr(guess), per_pair, w, h, rx, ry, int(bool(subpixel)), _ptr(duv), _ptr(score),
                                         _ptr(status), _ptr(surface), _ptr(times) if return_times else None))
    result = (duv, score, status, surface) if return_surface else (duv, score, status)
    return _timed(result, DISPLACEMENTS_TIMES, times, return_times, extend=True)


VELOCITY_FIELD_TIMES = ("upload_ms", "test_ms", "stack_ms", "download_ms")


def stage_velocity_field(duv, score, status, grid, dt, scale, min_score, accept_edge, radius, min_neighbors, threshold,
                         epsilon, min_count, device_id=0, return_times=False):
    """Displacements tested against their neighbours and stacked over the pairs (INPUTS.md, "Velocity field: the rule"):
    `duv` (P, n, 2) float64, `score` (P, n) float64 and `status` (P, n) uint8 as `stage_displacements` returns them, at the
    n = rows * cols nodes of `grid` = (rows, cols) in row-major order; `dt` (P,) float64, `scale` a pair.  Returns
    (v (n, 2), sigma (n, 2), count (n,) int32, kept (P, n) bool), with `return_times` also a dict of VELOCITY_FIELD_TIMES.
    glimpse_amd.velocity checks what the caller gave."""
    duv = _arr(duv, np.float64)
    if duv.ndim != 3 or duv.shape[2] != 2 or duv.shape[0] < 1 or duv.shape[1] < 1:
        raise ValueError(f"duv must be (P, n, 2) with P, n >= 1, got {duv.shape}")
    p, n = duv.shape[:2]
    score, status, dt = _arr(score, np.float64, (p, n)), _arr(status, np.uint8, (p, n)), _arr(dt, np.float64, (p,))
    rows, cols = (int(v) for v in grid)
    v, sigma = np.empty((n, 2)), np.empty((n, 2))
    count, kept = np.empty(n, dtype=np.int32), np.empty((p, n), dtype=np.uint8)
    times = np.zeros(len(VELOCITY_FIELD_TIMES))
    check(load().glh_stage_velocity_field(device_id, _ptr(duv), _ptr(score), _ptr(status), p, rows, cols, n, _ptr(dt),
                                          float(scale[0]), float(scale[1]), float(min_score), int(bool(accept_edge)),
                                          int(radius), int(min_neighbors), float(threshold), float(epsilon),
                                          int(min_count), _ptr(v), _ptr(sigma), _ptr(count), _ptr(kept),
                                          _ptr(times) if return_times else None))
    return _timed((v, sigma, count, kept.view(np.bool_)), VELOCITY_FIELD_TIMES, times, return_times, extend=True)


FILTER_F64, FILTER_F32 = F64, F32
FILTER_TIMES =("upload_ms", "max_ms", "gauss0_ms", "gauss1_ms", "download_ms")


def _filter_array(a, mask):
    """(a, dtype flag, nx, ny, mask, out) of the filter stages: `a` (ny, nx) float64 / float32, `mask` uint8 (ny, nx) or
    None; glimpse_amd.filters checks what the caller gave."""
    a, flag, nx, ny = _float_array(a)
    if mask is not None:
        mask = _arr(mask, np.uint8, (ny, nx))
    return a, flag, nx, ny, mask, np.empty_like(a)


def _filter_weights(w):
    """(table, radius) of one axis of the Gaussian; (None, 0) for a skipped axis."""
    if w is None:
        return None, 0
    w = _arr(w, np.float64)
    if w.ndim != 1 or len(w) % 2 != 1:
        raise ValueError("a weight table has 2 * radius + 1 entries")
    return w, len(w) // 2


def stage_max_filter(a, mask, fill, size_y, size_x, mode=0, device_id=0, return_times=False):
    """helpers.maximum_filter (helpers.py:390-430) with a window of size_y rows x size_x columns and the boundary `mode`
    (a HIGHPASS_MODES code): a new array.  `return_times`: also a dict of the HIP-event split (FILTER_TIMES)."""
    a, flag, nx, ny, mask, out = _filter_array(a, mask)
    times = np.zeros(len(FILTER_TIMES))
    check(load().glh_stage_max_filter(device_id, _ptr(a), flag, nx, ny, _ptr(mask), int(bool(fill)), int(size_y), int(size_x),
                                      int(mode), _ptr(out), _ptr(times) if return_times else None))
    return _timed(out, FILTER_TIMES, times, return_times)


def stage_gaussian_filter(a, mask, fill, w0, w1, mode=0, device_id=0, return_times=False):
    """helpers.gaussian_filter (helpers.py:347-387) with the weight tables `w0` (along rows) and `w1` (along columns) of
    glimpse_amd.filters.gaussian_weights; None skips the axis."""
    a, flag, nx, ny, mask, out = _filter_array(a, mask)
    (w0, r0), (w1, r1) = _filter_weights(w0), _filter_weights(w1)
    times = np.zeros(len(FILTER_TIMES))
    check(load().glh_stage_gaussian_filter(device_id, _ptr(a), flag, nx, ny, _ptr(mask), int(bool(fill)), _ptr(w0), r0,
                                           _ptr(w1), r1, int(mode), _ptr(out), _ptr(times) if return_times else None))
    return _timed(out, FILTER_TIMES, times, return_times)


def stage_fill_crevasses(a, mask, fill, size_y, size_x, max_mode, w0, w1, gauss_mode, device_id=0, return_times=False):
    """Raster.fill_crevasses (raster.py:1266-1291): the Gaussian of the maximum, the same mask and `fill` for both, over
    one upload and one download."""
    a, flag, nx, ny, mask, out = _filter_array(a, mask)
    (w0, r0), (w1, r1) = _filter_weights(w0), _filter_weights(w1)
    times = np.zeros(len(FILTER_TIMES))
    check(load().glh_stage_fill_crevasses(device_id, _ptr(a), flag, nx, ny, _ptr(mask), int(bool(fill)), int(size_y),
                                          int(size_x), int(max_mode), _ptr(w0), r0, _ptr(w1), r1, int(gauss_mode), _ptr(out),
                                          _ptr(times) if return_times else None))
    return _timed(out, FILTER_TIMES, times, return_times)


CLAHE_TIMES = ("upload_ms", "histogram_ms", "lut_ms", "apply_ms", "download_ms")


def stage_clahe(array, clip_limit=40.0, tile_grid_size=(8, 8), device_id=0, return_luts=False, return_times=False):
    """CLAHE by INPUTS.md's "CLAHE: the rule" (optimize.CLAHE) of `array` uint8 (h, w) or (h, w, c) with c in 1 .. 4, whose
    channels are averaged first ((sum) // c, which is mean(axis=2).astype(uint8)): a new uint8 (h, w).  `tile_grid_size` is
    (tilesX, tilesY) as cv2 takes it.  `return_luts`: also every tile's table, uint8 (tilesY, tilesX, 256);
    `return_times`: also a dict of the HIP-event split (CLAHE_TIMES)."""
    array = np.asarray(array)
    if array.dtype != np.uint8 or array.ndim not in (2, 3):
        raise TypeError(f"a uint8 array of two or three dimensions (got {array.dtype}, {array.ndim} dimensions)")
    array = np.ascontiguousarray(array)
    h, w = array.shape[:2]
    channels = array.shape[2] if array.ndim == 3 else 1
    tiles_x, tiles_y = (int(t) for t in tile_grid_size)
    out = np.empty((h, w), np.uint8)
    luts = np.empty((max(tiles_y, 0), max(tiles_x, 0), 256), np.uint8) if return_luts else None
    times = np.zeros(len(CLAHE_TIMES))
    check(load().glh_stage_clahe(device_id, _ptr(array), w, h, channels, float(clip_limit), tiles_x, tiles_y, _ptr(out),
                                 _ptr(luts), _ptr(times) if return_times else None))
    return _timed((out, luts) if return_luts else out, CLAHE_TIMES, times, return_times, extend=return_luts)


TERRAIN_F64, TERRAIN_F32 = F64, F32
TR_TIMES = 5  # entries of times_ms that every terrain stage writes (csrc/glh_terrain.h), whatever it names of them
GRADIENT_TIMES = ("upload_ms", "kernel_ms", "download_ms")
HILLSHADE_TIMES = ("upload_ms", "stencil_ms", "reduce_ms", "normalise_ms", "download_ms")
POLYGON_MASK_TIMES = ("upload_ms", "kernels_ms", "download_ms")


def stage_gradient(z, d0, d1, device_id=0, return_times=False):
    """Raster.gradient (raster.py:1465-1474): (dzdx, dzdy) of `z` (ny, nx) with the signed cell sizes d0 (x) and d1 (y),
    each of z's dtype.  `return_times`: also a dict of the HIP-event split (GRADIENT_TIMES)."""
    z, flag, nx, ny = _float_array(z)
    dzdx, dzdy = np.empty_like(z), np.empty_like(z)
    times = np.zeros(max(len(GRADIENT_TIMES), TR_TIMES))
    check(load().glh_stage_gradient(device_id, _ptr(z), flag, nx, ny, float(d0), float(d1), _ptr(dzdx), _ptr(dzdy),
                                    _ptr(times) if return_times else None))
    return _timed((dzdx, dzdy), GRADIENT_TIMES, times, return_times)


def stage_hillshade(z, d0, d1, vert_exag, direction, fraction, device_id=0, return_times=False):
    """matplotlib's LightSource.hillshade (Raster.hillshade, raster.py:1249-1264) of `z` (ny, nx): float64 (ny, nx).  d0,
    d1: the spacings of the gradient along x and y (dy already negated); `direction` (3,) towards the light."""
    z, flag, nx, ny = _float_array(z)
    direction = _arr(direction, np.float64, (3,))
    out = np.empty((ny, nx))
    times = np.zeros(max(len(HILLSHADE_TIMES), TR_TIMES))
    check(load().glh_stage_hillshade(device_id, _ptr(z), flag, nx, ny, float(d0), float(d1), float(vert_exag), _ptr(direction),
                                     float(fraction), _ptr(out), _ptr(times) if return_times else None))
    return _timed(out, HILLSHADE_TIMES, times, return_times)


def stage_polygon_mask(xy, ring_off, n_polygons, n_holes, nx, ny, device_id=0, return_times=False):
    """helpers.polygons_to_mask (helpers.py:1701-1768) by the stated even-odd rule: `xy` (n, 2) the vertices of all rings
    in continuous cell coordinates, `ring_off` (rings + 1,) their offsets, the polygon rings first -> bool (ny, nx)."""
    ring_off = _arr(ring_off, np.int32, (int(n_polygons) + int(n_holes) + 1,))
    xy = _arr(xy, np.float64, (int(ring_off[-1]), 2))
    out = np.empty((int(ny), int(nx)), dtype=np.uint8)
    times = np.zeros(max(len(POLYGON_MASK_TIMES), TR_TIMES))
    check(load().glh_stage_polygon_mask(device_id, _ptr(xy), len(xy), _ptr(ring_off), int(n_polygons), int(n_holes), int(nx),
                                        int(ny), _ptr(out), _ptr(times) if return_times else None))
    return _timed(out.view(bool), POLYGON_MASK_TIMES, times, return_times)


class _Handle:
    """A device object of the library (glh_X_create): `_h` is its handle, null once closed.  A subclass names the
    export that frees it (`_destroy`) and passes `self._handle()` to every other."""
    _destroy = None
    _h = None  # (closed until __init__ has run)

    def __init__(self):
        self._h = C.c_void_p()

    def _handle(self):
        if not self._h:
            raise GlhError(E_STATE, "the handle is closed")
        return self._h

    def close(self):
        if self._h:
            handle, self._h = self._h, C.c_void_p()  # (first: a second close, or __del__ after a failed one, has nothing to free)
            check(getattr(load(), self._destroy)(handle))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


ORIENT_TIMES = ("upload", "map", "reduce", "download")


class Orient(_Handle):
    """The matches of an image sequence on the device (glh_orient_create): uploaded once, evaluated at many view
    directions (optimize.ObserverCameras.fit).  `pair_i`, `pair_j` (n_pairs,): the images of every pair; `pair_offset`
    (n_pairs + 1,): pair p's matches are rows pair_offset[p] .. pair_offset[p + 1] of `xy_i`, `xy_j` (N, 2), the
    normalised camera coordinates of a match in image i and in image j."""

    _destroy = "glh_orient_destroy"

    def __init__(self, n_images, pair_i, pair_j, pair_offset, xy_i, xy_j, device_id=0):
        super().__init__()
        self.n_images = int(n_images)
        pair_i, pair_j = _arr(pair_i, np.int32), _arr(pair_j, np.int32)
        pair_offset = _arr(pair_offset, np.int64, (len(pair_i) + 1,))
        xy_i, xy_j = _arr(xy_i, np.float64).reshape(-1, 2), _arr(xy_j, np.float64).reshape(-1, 2)
        # (the library is not told N: the rows the offsets name must exist; what else is wrong with them it reports)
        if pair_i.ndim != 1 or pair_j.shape != pair_i.shape or len(xy_i) != len(xy_j) or len(xy_i) < pair_offset.max():
            raise ValueError("pair_i / pair_j (n_pairs,) and xy_i / xy_j (N, 2) with N >= pair_offset.max()")
        check(load().glh_orient_create(int(device_id), self.n_images, len(pair_i), _ptr(pair_i), _ptr(pair_j),
                                       _ptr(pair_offset), _ptr(xy_i), _ptr(xy_j), C.byref(self._h)))

    def eval(self, R, Rprime, return_times=False):
        """(objective, gradient (n_images, 3)) of the matches at the rotation matrices `R` (n_images, 3, 3) and their
        derivatives `Rprime` (n_images, 3, 3, 3) ([r][w][k], Camera.Rprime)."""
        handle = self._handle()
        R = _arr(R, np.float64, (self.n_images, 3, 3))
        Rprime = _arr(Rprime, np.float64, (self.n_images, 3, 3, 3))
        objective, gradient, times = C.c_double(0.0), np.empty((self.n_images, 3)), np.zeros(len(ORIENT_TIMES))
        check(load().glh_orient_eval(handle, _ptr(R), _ptr(Rprime), C.byref(objective), _ptr(gradient), _ptr(times)))
        return _timed((objective.value, gradient), ORIENT_TIMES, times, return_times, extend=True)


CALIB_TIMES = ("upload", "points", "line_points", "nearest", "download")
CALIB_KINDS = {"points": 0, "lines": 1, "matches": 2, "rotation": 3, "rotation_xy": 4}


class Calib(_Handle):
    """The controls of a camera calibration on the device (glh_calib_create): uploaded once, evaluated under many sets
    of camera vectors (optimize.Cameras).  Control c is of `kind[c]` (CALIB_KINDS), belongs to camera `cam_a[c]` (the match
    kinds: to `cam_a[c]` and `cam_b[c]`) of `n_cams` and owns rows row_offset[c] .. row_offset[c + 1] of `obs` (N, 2) and
    `src` (N, 3) (include/glimpse_hip.h says what each kind keeps there)."""

    _destroy = "glh_calib_destroy"

    def __init__(self, n_cams, kind, cam_a, cam_b, directions, row_offset, obs, src, device_id=0):
        super().__init__()
        self.n_cams = int(n_cams)
        kind, cam_a, cam_b = _arr(kind, np.int32), _arr(cam_a, np.int32), _arr(cam_b, np.int32)
        directions = _arr(directions, np.int32)
        self.rows = np.diff(_arr(row_offset, np.int64, (len(kind) + 1,)))
        self.kind = kind
        row_offset = _arr(row_offset, np.int64)
        obs, src = _arr(obs, np.float64).reshape(-1, 2), _arr(src, np.float64).reshape(-1, 3)
        if kind.ndim != 1 or not (cam_a.shape == cam_b.shape == directions.shape == kind.shape) or len(obs) != len(src) \
                or len(obs) < row_offset.max():
            raise ValueError("kind / cam_a / cam_b / directions (n_controls,) and obs (N, 2), src (N, 3) with N >= row_offset.max()")
        check(load().glh_calib_create(int(device_id), self.n_cams, len(kind), _ptr(kind), _ptr(cam_a), _ptr(cam_b),
                                      _ptr(directions), _ptr(row_offset), _ptr(obs), _ptr(src), C.byref(self._h)))

    def eval(self, cams, rot, job_control, job_set, job_side=None, tables=None, return_times=False):
        """`predicted` (rows, 2) of the jobs, concatenated in job order: job q is control `job_control[q]` under the
        camera vectors `cams[job_set[q]]` (n_sets, n_cams, 24), with `rot` (n_sets, n_cams, 3, 3) the rotation matrices the
        host methods use.  `job_side`: which camera of a match control predicts (default 0).  `tables`: for every job
        None, or the segment table of a Lines job: (seg_vertex (S + 1,), seg_count (S,), seg_par (S, 5), vertex (V, 3))."""
        handle = self._handle()
        cams = _arr(cams, np.float64)
        if cams.ndim != 3 or cams.shape[1:] != (self.n_cams, CAM_LEN):
            raise ValueError(f"expected camera vectors (n_sets, {self.n_cams}, {CAM_LEN}), got {cams.shape}")
        rot = _arr(rot, np.float64, (len(cams), self.n_cams, 3, 3))
        job_control = _arr(job_control, np.int32)
        job_set = _arr(job_set, np.int32, job_control.shape)
        job_side = np.zeros(len(job_control), np.int32) if job_side is None else _arr(job_side, np.int32, job_control.shape)
        if tables is None:
            tables = [None] * len(job_control)
        job_seg, seg_vertex, seg_count, seg_par, vertex, nv = [0], [np.zeros(1, np.int64)], [], [], [], 0
        for table in tables:
            if table is not None:
                sv, sc, sp, vx = table
                seg_vertex.append(np.asarray(sv[1:], dtype=np.int64) + nv)
                seg_count.append(np.asarray(sc, dtype=np.int64))
                seg_par.append(np.asarray(sp, dtype=np.float64).reshape(-1, 5))
                vertex.append(np.asarray(vx, dtype=np.float64).reshape(-1, 3))
                nv += len(vertex[-1])
            job_seg.append(sum(len(c) for c in seg_count))
        job_seg = _arr(job_seg, np.int64)
        seg_vertex = _arr(np.concatenate(seg_vertex), np.int64)
        seg_count = _arr(np.concatenate(seg_count) if seg_count else np.zeros(0), np.int64)
        seg_par = _arr(np.concatenate(seg_par) if seg_par else np.zeros((0, 5)), np.float64)
        vertex = _arr(np.concatenate(vertex) if vertex else np.zeros((0, 3)), np.float64)
        in_range = (job_control >= 0) & (job_control < len(self.rows))
        predicted = np.empty((int(self.rows[job_control[in_range]].sum()), 2))
        times = np.zeros(len(CALIB_TIMES))
        check(load().glh_calib_eval(handle, len(cams), _ptr(cams), _ptr(rot), len(job_control), _ptr(job_control),
                                    _ptr(job_set), _ptr(job_side), _ptr(job_seg), _ptr(seg_vertex), _ptr(seg_count),
                                    _ptr(seg_par), len(vertex), _ptr(vertex), _ptr(predicted), _ptr(times)))
        return _timed(predicted, CALIB_TIMES, times, return_times)

    def fit_sets(self, cams, fit_cam, slots, x0, lb, ub, x_scale, set_offset, set_rows, weights=None, observed=None,
                 max_nfev=None, ftol=1e-8, xtol=1e-8, gtol=1e-8, max_error=None, return_times=False):
        """Fits the entries `slots` of camera `fit_cam`'s vector to each of the row sets in ONE device call
        (glh_calib_fit_sets; include/glimpse_hip.h says how): set q is set_rows[set_offset[q]:set_offset[q + 1]], global
        row numbers.  `cams` (n_cams, 24); `x0`, `lb`, `ub`, `x_scale` (p,), lb < ub; `weights` None or (N, 2); `observed`
        None (the uploaded obs) or (N, 2), which a "rotation" control needs: its obs are camera coordinates; `max_nfev`
        default 100 p.  Returns (x (S, p), status (S,) int32, mean_error (S,)) -- a status > 0 converged
        (CALIB_FIT_STATUS) -- and, with `max_error`, inlier (S, N) uint8: 1 where the row's error is < max_error under
        the set's values, 2 for the set's own rows."""
        handle = self._handle()
        cams, slots, weights, observed, max_nfev, n_rows = self._fit_arguments(cams, slots, weights, observed, max_nfev)
        if slots.ndim != 1:
            raise ValueError("slots (p,)")
        x0, lb, ub, x_scale = (_arr(v, np.float64, slots.shape) for v in (x0, lb, ub, x_scale))
        set_offset, set_rows = _arr(set_offset, np.int64), _arr(set_rows, np.int64)
        n_sets = len(set_offset) - 1
        if set_offset.ndim != 1 or n_sets < 0 or set_rows.ndim != 1 or len(set_rows) < set_offset.max(initial=0):
            raise ValueError("set_offset (S + 1,) and set_rows (set_offset.max(),)")
        score = max_error is not None
        x, status, mean_error = np.empty((n_sets, len(slots))), np.empty(n_sets, np.int32), np.empty(n_sets)
        inlier = np.empty((n_sets, n_rows), np.uint8) if score else None
        times = np.zeros(len(CALIB_FIT_TIMES))
        check(load().glh_calib_fit_sets(
            handle, _ptr(cams), int(fit_cam), len(slots), _ptr(slots), _ptr(x0), _ptr(lb), _ptr(ub), _ptr(x_scale),
            _ptr(weights), _ptr(observed), n_sets, _ptr(set_offset), _ptr(set_rows), max_nfev, float(ftol), float(xtol), float(gtol), int(score),
            float(max_error) if score else 0.0, _ptr(x), _ptr(status), _ptr(mean_error), _ptr(inlier) if score else None,
            _ptr(times)))
        out = (x, status, mean_error, inlier) if score else (x, status, mean_error)
        return _timed(out, CALIB_FIT_TIMES, times, return_times)

    def _fit_arguments(self, cams, slots, weights, observed, max_nfev):
        """What `fit_sets` and `ransac_groups` take alike, as the library reads it (max_nfev: default 100 per parameter), and N."""
        cams = _arr(cams, np.float64)
        if cams.shape != (self.n_cams, CAM_LEN):
            raise ValueError(f"expected camera vectors ({self.n_cams}, {CAM_LEN}), got {cams.shape}")
        slots = _arr(slots, np.int32)
        n_rows = int(self.rows.sum())
        if weights is not None:
            weights = _arr(weights, np.float64, (n_rows, 2))
        if observed is not None:
            observed = _arr(observed, np.float64, (n_rows, 2))
        return cams, slots, weights, observed, int(100 * slots.size if max_nfev is None else max_nfev), n_rows

    def ransac_groups(self, cams, group_control, group_cam, slots, x0, lb, ub, x_scale, hyp_offset, samples, max_error,
                      min_inliers, weights=None, observed=None, max_nfev=None, ftol=1e-8, xtol=1e-8, gtol=1e-8,
                      return_times=False, group_id=None, drawn=None, seed=(0, 0), n=None):
        """Random Sample Consensus over G groups in ONE device pass (glh_calib_ransac_groups; include/glimpse_hip.h says
        how): group g is the match control `group_control[g]` with the camera `group_cam[g]` fitted in the entries `slots`
        (p,) of its vector, from `x0` inside `lb` .. `ub` with the scales `x_scale`, each (G, p); it owns the hypotheses
        hyp_offset[g] .. hyp_offset[g + 1], rows of `samples` (H, n) (global row numbers).  `weights`, `observed`: as
        `fit_sets`.  Returns a dict: per hypothesis `values` (H, p), `status`, `consensus`, `refit_values`,
        `refit_status`, `mean_errors`; per group `winner` (its hypothesis counted from the group's first, -1: none); per
        row of the handle `inlier` (uint8).

        `drawn` (G,) of 0 / 1 (glh_calib_ransac_groups_drawn): a group with 1 has its samples drawn on the device as those
        of pair `group_id[g]` under the two 32-bit words `seed`, and `samples` (or None when every group is drawn) is not
        read for it (`n`: the sample size then); the dict also has `samples` (H, n), the global rows of every hypothesis,
        and the times `draw`."""
        handle = self._handle()
        cams, slots, weights, observed, max_nfev, n_rows = self._fit_arguments(cams, slots, weights, observed, max_nfev)
        group_control = _arr(group_control, np.int32)
        group_cam = _arr(group_cam, np.int32, group_control.shape)
        if slots.ndim != 1 or group_control.ndim != 1:
            raise ValueError("slots (p,) and group_control (G,)")
        n_groups, p = len(group_control), len(slots)
        x0, lb, ub, x_scale = (_arr(v, np.float64, (n_groups, p)) for v in (x0, lb, ub, x_scale))
        hyp_offset = _arr(hyp_offset, np.int64, (n_groups + 1,))
        n_hyp = int(hyp_offset.max(initial=0))
        if samples is not None or drawn is None:
            samples = _arr(samples, np.int64)
            if samples.ndim != 2 or len(samples) < n_hyp:
                raise ValueError("samples (H, n) with H >= hyp_offset.max()")
            n = samples.shape[1]
        out = dict(values=np.empty((n_hyp, p)), status=np.empty(n_hyp, np.int32), consensus=np.empty(n_hyp, np.int32),
                   refit_values=np.empty((n_hyp, p)), refit_status=np.empty(n_hyp, np.int32), mean_errors=np.empty(n_hyp),
                   winner=np.empty(n_groups, np.int32), inlier=np.empty(n_rows, np.uint8))
        shared = (handle, _ptr(cams), n_groups, _ptr(group_control), _ptr(group_cam), p, _ptr(slots), _ptr(x0), _ptr(lb), _ptr(ub),
                  _ptr(x_scale), _ptr(weights), _ptr(observed), _ptr(hyp_offset), int(n), _ptr(samples),
                  max_nfev, float(ftol), float(xtol), float(gtol), float(max_error),
                  int(min(max(min_inliers, -1), 2 ** 62)), *[_ptr(out[key]) for key in ("values", "status", "consensus", "refit_values",
                                                                                       "refit_status", "mean_errors", "winner", "inlier")])
        if drawn is None:
            names = CALIB_RANSAC_TIMES
            times = np.zeros(len(names))
            check(load().glh_calib_ransac_groups(*shared, _ptr(times)))
        else:
            names = CALIB_RANSAC_TIMES + ("draw",)
            times = np.zeros(len(names))
            drawn, group_id = _arr(drawn, np.uint8, (n_groups,)), _arr(group_id, np.int32, (n_groups,))
            out["samples"] = np.empty((n_hyp, int(n)), np.int64)
            check(load().glh_calib_ransac_groups_drawn(*shared, _ptr(group_id), _ptr(drawn), int(seed[0]), int(seed[1]),
                                                       _ptr(out["samples"]), _ptr(times)))
        return _timed(out, names, times, return_times)


def ransac_hypotheses(rows, n, iterations):
    """(hyps, enumerated), each (G,): min(iterations, C(rows[g], n)) hypotheses for a pair of rows[g] rows (0 for n rows or
    fewer) and whether they are all its combinations, which `ransac_combinations` lists, or drawn on the device
    (glh_ransac_hypotheses: host arithmetic, no device)."""
    rows = _arr(rows, np.int64)
    hyps, enumerated = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.uint8)
    check(load().glh_ransac_hypotheses(len(rows), _ptr(rows), int(n), int(iterations), _ptr(hyps), _ptr(enumerated)))
    return hyps, enumerated.astype(bool)


def ransac_combinations(rows, n, count):
    """(count, n) int64: the first `count` combinations of `n` of `rows` rows in lexicographic order
    (glh_ransac_combinations: host arithmetic, no device)."""
    samples = np.empty((int(count), int(n)), np.int64)
    check(load().glh_ransac_combinations(int(rows), int(n), int(count), _ptr(samples)))
    return samples


RANSAC_SAMPLES_TIMES = ("upload", "draw", "download")


def stage_ransac_samples(device_id, rows, group_id, hyp_offset, n, seed, return_times=False):
    """(H, n) int64: the samples `ransac_pairs(samples="device")` draws for G pairs of `rows[g]` rows that are the pairs
    `group_id[g]` of its list, hypotheses hyp_offset[g] .. hyp_offset[g + 1], under the two 32-bit words `seed`: rows
    within the pair, ascending (glh_stage_ransac_samples: the draw kernel alone)."""
    rows = _arr(rows, np.int64)
    group_id = _arr(group_id, np.int32, rows.shape)
    hyp_offset = _arr(hyp_offset, np.int64, (len(rows) + 1,))
    samples = np.empty((int(hyp_offset.max(initial=0)), int(n)), np.int64)
    times = np.zeros(len(RANSAC_SAMPLES_TIMES))
    check(load().glh_stage_ransac_samples(int(device_id), len(rows), _ptr(rows), _ptr(group_id), _ptr(hyp_offset), int(n),
                                          int(seed[0]), int(seed[1]), _ptr(samples), _ptr(times)))
    return _timed(samples, RANSAC_SAMPLES_TIMES, times, return_times)


def ransac_chunks(rows, hyps, budget):
    """chunk_of (G,) int32: the call each group goes to when consecutive groups share a call while its consensus masks
    (rows[g] * hyps[g] bytes each) stay at or below `budget` bytes (glh_ransac_chunks: host arithmetic, no device)."""
    rows, hyps = _arr(rows, np.int64), _arr(hyps, np.int64, np.shape(rows))
    chunk_of, n_chunks = np.zeros(len(rows), np.int32), C.c_int32(0)
    check(load().glh_ransac_chunks(len(rows), _ptr(rows), _ptr(hyps), int(budget), _ptr(chunk_of), C.byref(n_chunks)))
    return chunk_of


CALIB_RANSAC_TIMES = ("upload", "fit", "score", "refit", "final_score", "download")
CALIB_NOT_REFITTED = -100  # refit_status of a hypothesis that was not accepted (csrc/glh_ransac_plan.h)
CALIB_FIT_TIMES = ("upload", "fit", "score", "download")
CALIB_FIT_STATUS = {1: "gtol", 2: "ftol", 3: "xtol", 0: "the evaluation cap was reached", -1: "fewer residuals than parameters",
                    -2: "the cost is not finite", -3: "the system is singular"}
MATCH_TIMES = ("upload", "prepare", "search", "merge", "download")
MATCH_U8, MATCH_F32 = 0, 1
MATCH_U8_MAX_DIM = 256  # csrc/glh_match.h


class Matcher(_Handle):
    """Descriptor sets on the device (glh_match_create): each is uploaded once under a slot number and searched many
    times (optimize.match_keypoints, optimize.KeypointMatcher.build_matches).  `knn2(q, t)` is, for every row of slot q's
    set, the two rows of slot t's with the smallest keys (squared distance, row index): equal distances go to the lower
    index."""

    _destroy = "glh_match_destroy"

    def __init__(self, device_id=0):
        super().__init__()
        self._sets = {}  # slot -> (kind, n, dim)
        check(load().glh_match_create(int(device_id), C.byref(self._h)))

    def put(self, slot, descriptors, path=None):
        """Uploads `descriptors` (n, dim) under `slot`, in the place of what it held; returns the path taken.  uint8
        rows, and float rows whose values are all integers in 0 .. 255, take the integer path when dim <= 256 (exact
        int32 distances on the matrix cores); everything else the float path (float32, summed in element order).
        `path="float"` forces the float path."""
        handle = self._handle()
        if path not in (None, "float"):
            raise ValueError(f'path is None or "float", not {path!r}')
        d = np.asarray(descriptors)
        if d.ndim != 2:
            raise ValueError(f"expected descriptors (n, dim), got shape {d.shape}")
        integer = path is None and d.shape[1] <= MATCH_U8_MAX_DIM and d.dtype != np.bool_ and (
            d.dtype == np.uint8 or bool(np.all((d >= 0) & (d <= 255) & (d == np.floor(d)))))
        kind = MATCH_U8 if integer else MATCH_F32
        d = _arr(d, np.uint8 if integer else np.float32)
        check(load().glh_match_put(handle, int(slot), kind, d.shape[0], d.shape[1], _ptr(d)))
        self._sets[int(slot)] = (kind, d.shape[0], d.shape[1])
        return "integer" if integer else "float"

    def drop(self, slot):
        check(load().glh_match_drop(self._handle(), int(slot)))
        self._sets.pop(int(slot), None)

    def slots(self):
        return sorted(self._sets)

    def path(self, slot):
        """"integer" or "float": the path the set of `slot` was prepared for; None when the slot is empty."""
        held = self._sets.get(int(slot))
        return None if held is None else ("integer" if held[0] == MATCH_U8 else "float")

    def knn2(self, slot_q, slot_t, return_times=False):
        """(idx int32 (n_q, 2), d2 float32 (n_q, 2)): the nearest and second nearest row of slot_t's set for every row
        of slot_q's.  A set of one row has no second: (-1, inf)."""
        handle = self._handle()
        n_q = self._sets.get(int(slot_q), (0, 0, 0))[1]  # (an unknown slot is the library's to report)
        idx, d2 = np.empty((n_q, 2), np.int32), np.empty((n_q, 2), np.float32)
        times = np.zeros(len(MATCH_TIMES))
        check(load().glh_match_knn2(handle, int(slot_q), int(slot_t), _ptr(idx), _ptr(d2), _ptr(times)))
        return _timed((idx, d2), MATCH_TIMES, times, return_times, extend=True)

    def close(self):
        if self._h:
            self._sets = {}
        super().close()


SIFT_TIMES = ("upload", "base", "pyramid", "extrema", "refine", "describe", "download")
SIFT_GAUSS, SIFT_DOG, SIFT_CANDIDATES, SIFT_REFINED, SIFT_CELLS = range(5)
SIFT_MAX_LAYERS = 8  # csrc/glh_sift.h


def sift_tables(n_layers, sigma):
    """[(radius, weights float64)] of the S + 3 blurs of the SIFT pyramid (INPUTS.md, "SIFT: the rule"): [0] the doubled
    image's, sqrt(max(sigma^2 - 1, 0.01)); [i] from Gaussian layer i - 1 to layer i.  Radius (round(8 sig + 1) | 1) // 2,
    exp(-x^2 / 2 sig^2) normalised, in float64."""
    k = 2.0 ** (1.0 / n_layers)
    sigs = [math.sqrt(max(sigma * sigma - 1.0, 0.01))]
    for i in range(1, n_layers + 3):
        prev = math.pow(k, i - 1) * sigma
        total = prev * k
        sigs.append(math.sqrt(total * total - prev * prev))
    tables = []
    for sig in sigs:
        r = (int(np.rint(8.0 * sig + 1.0)) | 1) // 2
        x = np.arange(-r, r + 1, dtype=np.float64)
        w = np.exp(-(x * x) / (2.0 * sig * sig))
        tables.append((r, w / w.sum()))
    return tables


class Sift(_Handle):
    """SIFT detection and description on the device (glh_sift_create): the pyramid's buffers stay allocated between
    images of one size.  `detect` gives the keypoints in the rule's order, before the host-side steps of optimize.SIFT."""

    _destroy = "glh_sift_destroy"

    def __init__(self, device_id=0):
        super().__init__()
        check(load().glh_sift_create(int(device_id), C.byref(self._h)))

    def detect(self, image, n_layers=3, contrast=0.04, edge=10.0, sigma=1.6, return_times=False):
        """(keypoints float64 (n, 6): pt x, pt y, size, angle, response, octave; descriptors uint8 (n, 128)) of `image`
        uint8 (h, w)."""
        handle = self._handle()
        image = np.asarray(image)
        if image.ndim != 2 or image.dtype != np.uint8:
            raise TypeError(f"a two-dimensional uint8 image (got {image.dtype}, {image.ndim} dimensions)")
        image = np.ascontiguousarray(image)
        n_layers = int(n_layers)
        if not 1 <= n_layers <= SIFT_MAX_LAYERS:
            raise ValueError(f"nOctaveLayers {n_layers}: 1 .. {SIFT_MAX_LAYERS} are served")
        tables = sift_tables(n_layers, float(sigma))
        params = np.concatenate([[n_layers, contrast, edge, sigma], [r for r, _ in tables], *[w for _, w in tables]])
        params = np.ascontiguousarray(params, np.float64)
        n = C.c_int(0)
        times = np.zeros(len(SIFT_TIMES))
        check(load().glh_sift_detect(handle, _ptr(image), image.shape[1], image.shape[0], _ptr(params), C.byref(n),
                                     _ptr(times)))
        keypoints, descriptors = np.zeros((n.value, 6)), np.zeros((n.value, 128), np.uint8)
        check(load().glh_sift_read(handle, _ptr(keypoints), _ptr(descriptors)))
        return _timed((keypoints, descriptors), SIFT_TIMES, times, return_times, extend=True)

    def counts(self):
        """{octaves, candidates, keypoints, layers, width, height} of the last detection (width, height: doubled)."""
        out = np.zeros(6, np.int32)
        check(load().glh_sift_counts(self._handle(), _ptr(out)))
        return dict(zip(("octaves", "candidates", "keypoints", "layers", "width", "height"), out.tolist()))

    def layer(self, kind, octave=0, index=0):
        """One stage of the last detection (include/glimpse_hip.h: glh_sift_layer)."""
        c = self.counts()
        if kind in (SIFT_GAUSS, SIFT_DOG):
            if not 0 <= octave < c["octaves"]:
                raise ValueError(f"octave {octave}: the pyramid has {c['octaves']}")
            scale = (1 << octave) - 1
            out = np.zeros(((c["height"] + scale) >> octave, (c["width"] + scale) >> octave), np.float32)
        elif kind == SIFT_CANDIDATES:
            out = np.zeros((c["candidates"], 4), np.int32)
        elif kind == SIFT_REFINED:
            out = np.zeros((c["candidates"], 12), np.float64)
        elif kind == SIFT_CELLS:
            out = np.zeros((c["keypoints"], 5), np.int32)
        else:
            raise ValueError(f"unknown kind {kind}")
        if out.size:
            check(load().glh_sift_layer(self._handle(), int(kind), int(octave), int(index), _ptr(out)))
        return out
