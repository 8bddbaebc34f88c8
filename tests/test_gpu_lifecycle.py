"""Contexts come and go without leaving device memory behind: every workspace a sequence grows on first use (float / 16-bit
workspaces, the second stream's events, phase stamps, debug buffers) is released by glh_destroy."""
import os
import subprocess
import sys

import numpy as np
import pytest

from glimpse_amd import _lib, workloads

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sequence(bits, streams, T=4):
    wl = workloads.Workload("C3", n_frames=T, n_points=24, n_particles=900, imgsz=(384, 384))
    frames = [wl.frames(o) for o in range(wl.O)]
    if bits == 32:
        frames = [[np.asarray(f, dtype=np.float32) * np.float32(1.0 / 255.0) for f in fo] for fo in frames]
    elif bits == 16:
        frames = [[np.asarray(f, dtype=np.uint16) * np.uint16(257) for f in fo] for fo in frames]
    wl.bits = bits
    with _lib.Context(wl.P, wl.N, wl.O, device_id=0, max_tile=max(wl.tile), max_search_dim=160, max_frames=T) as ctx:
        workloads.setup_context(ctx, wl, frames)
        ctx.set_math("fast")
        ctx.set_track_streams(streams)
        ctx.phase_stamps()  # (arms the diagnostic stamps: one more buffer to release)
        ctx.set_frame(0)
        ctx.init_particles(seed=5)
        ctx.init_templates(0, 0)
        ctx.record_moments(0)
        fr = list(range(1, T))
        ctx.track(fr, [1.0] * len(fr), [[j] for j in fr], seed=5)
        assert ctx.last_track_streams() == streams
        assert (ctx.point_status() == 0).all()
        return ctx.get_moments(0, T)


def test_contexts_release_their_device_memory():
    _sequence(8, 2)  # (the library's one-time allocations -- module, streams' pools -- happen here)
    _sequence(16, 1)
    _sequence(32, 2)
    free0, total = _lib.device_memory(0)
    first = None
    for rep in range(6):
        for bits, streams in ((8, 2), (16, 1), (32, 2)):
            m = _sequence(bits, streams)
            if rep == 0 and bits == 8:
                first = m
            elif bits == 8:
                np.testing.assert_array_equal(m, first)  # (and a fresh context repeats the run bit for bit)
    free1, _ = _lib.device_memory(0)
    assert free0 - free1 < 32 << 20, f"{(free0 - free1) >> 20} MiB of {total >> 20} gone after 18 contexts"


# The members that _sequence leaves alone, and a frame that a torch tensor lends.  A fresh interpreter runs it: torch
# bundles its own HIP runtime and has to be imported before the library is loaded (tests/test_gpu_interop.py).
SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import torch                      # first: see tests/test_gpu_interop.py
import numpy as np
import glimpse_amd
from glimpse_amd import _lib, workloads

T, P, N = 4, 12, 600
wl = workloads.Workload("C3", n_frames=T, n_points=P, n_particles=N, imgsz=(384, 384))
frames = [np.ascontiguousarray(f) for f in wl.frames(0)]
lim = (-40.0, 40.0)
rng = np.random.default_rng(9)
rasters = (glimpse_amd.Raster(0.05 * rng.standard_normal((33, 41)), x=lim, y=(40.0, -40.0)),
           glimpse_amd.Raster(0.3 + 0.1 * rng.random((17, 19)), x=lim, y=lim),
           glimpse_amd.Raster(np.ones((16, 16)), x=lim, y=lim))
params = np.zeros((P, _lib.MOTION_FULL_LEN))
params[:, :18] = wl.params
params[:, 7:10] = (0.2, 0.2, 0.05)
params[:, 13:16] = (0.05, 0.05, 0.01)
params[:, 20:22] = 1.0  # (dem and dem_sigma from the rasters)
lent = torch.from_numpy(frames[3]).cuda()
torch.cuda.synchronize()
host = np.empty_like(frames[2])
_lib.host_register(host.ctypes.data, host.nbytes)


def every_other_member():
    # One context with the copy stream, its pinned ring and events (six async uploads through four slots, one pinned
    # upload), a borrowed frame, the three rasters, the spline factors of general orders, host-fed normals and uniforms,
    # the extra log likelihoods, the debug buffers of both levels, the residual draw counts, the covariances and the
    # track layout.
    rng = np.random.default_rng(3)
    with _lib.Context(P, N, 1, device_id=0, max_tile=max(wl.tile), max_search_dim=160, max_frames=T) as ctx:
        ctx.observer_init(0, T, wl.imgsz[0], wl.imgsz[1], 1, wl.sigmas[0])
        ctx.observer_set_cameras(0, np.tile(wl.cams[0], (T, 1)))
        for t in (0, 1, 2, 3, 0, 1):  # (the fifth upload waits for the first one's slot)
            ctx.observer_upload_frame_async(0, t, frames[t])
        host[...] = frames[2]
        assert ctx.upload_done(ctx.observer_upload_frame_pinned(0, 2, host), wait=True)
        ctx.observer_set_frame_device(0, 3, lent.data_ptr())  # (in place of the frame uploaded above, which is freed)
        ctx.begin_sequence(P, N, wl.tile)
        for slot, raster in zip((_lib.RASTER_DEM, _lib.RASTER_DEM_SIGMA, _lib.RASTER_VIEWSHED), rasters):
            ctx.set_raster(slot, raster)
        ctx.set_motion(params)
        ctx.set_interpolation(2, 4)
        ctx.track_covariances(True)
        ctx.set_fused(0)
        ctx.set_debug(1)
        ctx.set_frame(0)
        ctx.init_particles(normals=rng.standard_normal((P, N, 6)))
        ctx.init_templates(0, 0)
        ctx.record_moments(0)
        ctx.set_extra_log_likelihoods(np.zeros((P, N)))
        for i, method in ((1, "stratified"), (2, "residual")):
            ctx.set_frame(i)
            ctx.evolve(1.0, seed=5, step=i)
            ctx.update_weights([i])
            ctx.resample(u=rng.random((P, N)), method=method)
            ctx.record_moments(i)
        ctx.set_extra_log_likelihoods(None)
        ctx.set_debug(2)
        ctx.track([3], [1.0], [[3]], seed=5)  # (on the borrowed frame, with the covariances of the frame)
        assert np.isfinite(ctx.get_covariances(3, 1)).all()
        means, sigmas = ctx.get_tracks(0, T)
        moments = ctx.get_moments(0, T)
        np.testing.assert_array_equal(means, moments[:, :, :6].transpose(1, 0, 2))
        np.testing.assert_array_equal(sigmas, moments[:, :, 6:].transpose(1, 0, 2))
        assert (ctx.point_status() == 0).all()
        return moments


# The warm-up pass is two contexts, because the one-time allocations of a process are not over after one.  Free memory
# read after every context on an MI355X (ROCm 7), with this library and with the one before the context's members owned
# their memory, each feature above on its own and all together: 204 800 KiB go once, with the second context of the
# process, whatever it does, and 0 KiB with each of the 35 contexts after it.  (The test above warms up with three.)
first = every_other_member()
np.testing.assert_array_equal(every_other_member(), first)
free0, total = _lib.device_memory(0)
gone = []
for rep in range(6):
    np.testing.assert_array_equal(every_other_member(), first)
    gone.append((free0 - _lib.device_memory(0)[0]) >> 10)
free1, _ = _lib.device_memory(0)
_lib.host_unregister(host.ctypes.data)
print(f"KiB gone after each context: {{gone}}")
print(f"{{(free0 - free1) >> 20}} MiB of {{total >> 20}} gone after 6 contexts")
assert free0 - free1 < 32 << 20
np.testing.assert_array_equal(lent.cpu().numpy(), frames[3])
print("LIFECYCLE_OK")
"""


def test_contexts_release_what_they_grow_on_demand_and_leave_a_borrowed_frame_alone(tmp_path):
    """The members that test_contexts_release_their_device_memory does not reach (SCRIPT: every_other_member) are
    released with their context too, and a frame lent with observer_set_frame_device is not: the torch tensor holds its
    values after the contexts that read it are closed.  The comparison of free device memory only sees buffers of
    megabytes (the SSE copy, the staging of the normals); that the small ones -- events, streams, tables of a few
    kilobytes -- are released is what their types are for: every member of the context owns what it holds
    (csrc/glh_stage.h)."""
    script = tmp_path / "lifecycle.py"
    script.write_text(SCRIPT.format(root=ROOT))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "LIFECYCLE_OK" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
