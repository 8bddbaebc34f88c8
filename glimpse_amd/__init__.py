"""glimpse_amd: the `glimpse.Tracker` particle-filter hot path on AMD MI355X (gfx950).

Drop-in names for that path only (see DESIGN.md for scope):

    from glimpse_amd import Camera, Image, Observer, CartesianMotion, Tracker, Tracks
    (+ CylindricalMotion, TangentCartesianMotion, TangentCylindricalMotion)
    from glimpse_amd.optimize import ObserverCameras, RotationMatchesXYZ   # orienting an image sequence
    from glimpse_amd.optimize import Cameras, Points, Lines, Matches       # calibrating cameras
    from glimpse_amd.optimize import KeypointMatcher, match_keypoints      # matching keypoints between images

The compute runs in hand-written HIP kernels behind a C ABI (include/glimpse_hip.h,
glimpse_amd/lib/libglimpse_hip.so, bound with ctypes in glimpse_amd._lib).  There is no CPU
fallback: build the library with `python -m glimpse_amd.build`.
"""
from .camera import Camera
from .displacements import displacements
from .filters import gaussian_filter, maximum_filter
from .image import Image
from .motion import (CartesianMotion, CylindricalMotion, Motion, TangentCartesianMotion,
                     TangentCylindricalMotion)
from . import optimize
from .observer import Observer
from .optimize import (Cameras, KeypointMatcher, Lines, Matches, ObserverCameras, Points, Polynomial, RotationMatches,
                       RotationMatchesXY, RotationMatchesXYZ, match_keypoints, ransac)
from .raster import Raster, RasterInterpolant
from .tracker import Tracker
from .tracks import Tracks
from .velocity import velocity_field

__all__ = ["Camera", "Image", "Observer", "Motion", "CartesianMotion", "CylindricalMotion",
           "TangentCartesianMotion", "TangentCylindricalMotion", "Raster", "RasterInterpolant", "Tracker", "Tracks", "maximum_filter",
           "gaussian_filter", "optimize", "Matches", "RotationMatches", "RotationMatchesXY", "RotationMatchesXYZ",
           "ObserverCameras", "Cameras", "Points", "Lines", "Polynomial", "ransac", "KeypointMatcher", "match_keypoints",
           "displacements", "velocity_field"]
__version__ = "0.1.0"
