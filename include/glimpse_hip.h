/*
 * glimpse_hip.h -- C ABI of libglimpse_hip.so, the MI355X (gfx950) implementation of
 * the glimpse.Tracker particle-filter hot path.
 *
 * The reference (ezwelty/glimpse 0.1.1) is pure Python and has NO FFI layer; its
 * replaceable seams are Python duck types.  This header is
 * therefore the interface a maintainer would bind with ctypes;
 * every entry point cites the reference function whose work it takes over.
 * Citations are relative to /root/reference/src/glimpse/.
 *
 * Conventions
 *  - plain C: opaque context, raw pointers and sizes, no C++/torch types;
 *  - every function returns an int status: GLH_OK (0) or a negative GLH_E_* code;
 *    `glh_last_error()` returns a human-readable message for the calling thread;
 *  - host buffers are caller-owned, device buffers are library-owned;
 *  - one host thread per context; every call enqueues on the context's HIP stream,
 *    only `glh_get_*`, `glh_sync` and the `glh_stage_*` test hooks block;
 *  - array layouts are C-contiguous, doubles unless stated:
 *      particles [P][N][6]  (x, y, z, vx, vy, vz)   -- Tracker.particles, track/tracker.py:35
 *      weights   [P][N]                              -- Tracker.weights,   track/tracker.py:37
 *      cameras   [n][GLH_CAM_LEN]                    -- Camera._vector[20] (camera.py:101) + correction
 *      moments   [P][12] = mean(6) | sigma(6)        -- track/tracker.py:350-354
 */
#ifndef GLIMPSE_HIP_H
#define GLIMPSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLH_VERSION 100

/* ---- status codes ------------------------------------------------------------------ */
#define GLH_OK 0
#define GLH_E_INVALID (-1)   /* bad argument / size mismatch                              */
#define GLH_E_HIP (-2)       /* a HIP runtime call failed                                 */
#define GLH_E_NOMEM (-3)     /* host or device allocation failed                          */
#define GLH_E_STATE (-4)     /* call sequence error (e.g. step before templates)          */
#define GLH_E_UNSUPPORTED (-5)
#define GLH_E_COMM (-6)      /* librccl missing, or an RCCL call failed                   */

/* ---- camera vector ------------------------------------------------------------------ */
/* [0:3] xyz  [3:6] viewdir(deg)  [6:8] imgsz  [8:10] f  [10:12] c  [12:18] k1..k6
 * [18:20] p1,p2   -- exactly Camera._vector (camera.py:101, :128-198) --
 * [20] correction flag  [21] radius  [22] refraction (camera.py:118-121)
 * [23] 0 = camera.  1 = georeferenced raster image (an orthophoto observer, Raster as image,
 *      track/observer.py:26): world -> image is Grid.xyz_to_uv (raster.py:423-445),
 *      uv = (xy - (xlim[0], ylim[0])) / d, with [0:2] = (xlim[0], ylim[0]), [6:8] = size,
 *      [8:10] = d (signed cell size); every other entry is ignored.                            */
#define GLH_CAM_LEN 24

/* ---- motion parameters (CartesianMotion, track/motion.py:121-147) ------------------- */
/* [0:2] xy [2:4] xy_sigma [4:7] vxyz [7:10] vxyz_sigma [10:13] axyz [13:16] axyz_sigma
 * [16] dem (constant surface) [17] dem_sigma (constant)                                   */
#define GLH_MOTION_LEN 18

/* ---- motion parameters, general form (glh_set_motion) -------------------------------- */
/* [0:18] as above, read per model kind:
 *   CARTESIAN            (motion.py:92-204)   vxyz, vxyz_sigma, axyz, axyz_sigma
 *   CYLINDRICAL          (motion.py:207-311)  [4:7] vrthz [7:10] vrthz_sigma [10:13] arthz [13:16] arthz_sigma
 *   TANGENT_CARTESIAN    (motion.py:314-412)  [4:6] vxy [7:9] vxy_sigma [10:12] axy [13:15] axy_sigma
 *   TANGENT_CYLINDRICAL  (motion.py:415-522)  [4:6] vrth [7:9] vrth_sigma [10:12] arth [13:15] arth_sigma
 * [18] kind (GLH_MOTION_*)  [19] slope_sigma (tangent models)
 * [20] 1 = this point's dem is the context's GLH_RASTER_DEM raster (then [16] is ignored)
 * [21] 1 = this point's dem_sigma is the GLH_RASTER_DEM_SIGMA raster  [22:24] reserved.       */
#define GLH_MOTION_FULL_LEN 24
#define GLH_MOTION_CARTESIAN 0
#define GLH_MOTION_CYLINDRICAL 1
#define GLH_MOTION_TANGENT_CARTESIAN 2
#define GLH_MOTION_TANGENT_CYLINDRICAL 3
#define GLH_MOTION_EXTERNAL 4 /* a user-defined Motion (the duck type of motion.py:13-89): the caller initialises and
                               * evolves the particles (glh_set_particles) and supplies its log-likelihood term
                               * (glh_set_extra_log_likelihoods); the device does the observer likelihoods,
                               * resampling and moments                                                          */

/* ---- per-point status bits (sticky; the Python Tracker turns them into Tracks.errors).  A word holds the bits of the frame
 * at which its point first failed (glh_get_point_error_frame); what later frames would raise on the state the failure left
 * behind is not recorded: the reference has ended the track there. */
#define GLH_PT_NAN 1u            /* ValueError "missing (NaN) values"      tracker.py:118  */
#define GLH_PT_TEMPLATE_OOB 2u   /* IndexError "Box extends beyond grid"   raster.py:417   */
#define GLH_PT_SAMPLE_OUTSIDE 4u /* ValueError "sampling points outside"   observer.py:201 */
#define GLH_PT_RESAMPLE_CLAMP 8u /* searchsorted returned n (IndexError in the reference)  */
#define GLH_PT_CONST_TILE 16u    /* zero-variance template tile (reference yields NaNs)    */
#define GLH_PT_RASTER_OOB 32u    /* ValueError "sampling coordinates are out of bounds" raster.py:961-973 */
#define GLH_PT_NOT_VISIBLE 64u   /* ValueError "non-visible viewshed cells"  tracker.py:114-117 */

/* ---- per-(observer, point) status of the last likelihood evaluation ------------------ */
#define GLH_OBS_OK 0
#define GLH_OBS_SKIPPED 1      /* img is None or observer masked         tracker.py:577    */
#define GLH_OBS_OUT_OF_BOUNDS 2 /* warning + skip                        tracker.py:597-601 */
#define GLH_OBS_TILE_TOO_LARGE 3 /* search tile exceeds the workspace (build limit)        */
#define GLH_OBS_NO_TEMPLATE 4

/* ---- resampling methods (track/tracker.py:151-223) ------------------------------------- */
#define GLH_RESAMPLE_SYSTEMATIC 0 /* one uniform per point          tracker.py:168-176        */
#define GLH_RESAMPLE_STRATIFIED 1 /* one uniform per particle       tracker.py:178-186        */
#define GLH_RESAMPLE_CHOICE 2     /* np.random.choice(n, n, p=w)    tracker.py:205-209        */
#define GLH_RESAMPLE_RESIDUAL 3   /* as written in the reference     tracker.py:188-203        */

/* ---- random-number modes ------------------------------------------------------------- */
#define GLH_RNG_HOST 0   /* caller supplies the normals / uniforms (parity with np.random)  */
#define GLH_RNG_PHILOX 1 /* counter-based Philox4x32 (7 rounds) on the device               */

/* ---- arithmetic modes (glh_set_math) --------------------------------------------------- */
#define GLH_MATH_EXACT 0 /* every float64 expression rounds like NumPy's (default): with host-fed draws the resample
                          * indices are the reference's bit for bit                                           */
#define GLH_MATH_FAST 1  /* same formulas with fused multiply-adds, Newton reciprocals instead of IEEE divisions, a
                          * table exp and no normalisation pass in the systematic resampling: ~1e-13 relative on the
                          * posteriors, 10-15 % faster; meant for device-RNG runs, where no reference stream exists to be
                          * bit-exact with.  Small fitted surfaces are sampled in a per-cell power form.  Every motion
                          * model and surface kind has it (their own evolve steps and lookups have one form only).
                          * One limit: a non-zero dem_sigma of a point with a gridded surface (a constant beside a dem
                          * raster, or a node of the dem_sigma raster) must have 1.06e-154 <= |dem_sigma| <= 9.4e153 --
                          * the Newton reciprocal of 2 dem_sigma^2 is NaN outside the normal doubles, where the IEEE
                          * division gives inf or 0; glh_update_weights, glh_step and glh_track return
                          * GLH_E_UNSUPPORTED for such a value rather than NaN weights.                                  */

typedef struct glh_ctx glh_ctx;

typedef struct glh_config {
  int32_t device_id;      /* HIP device ordinal                                             */
  int32_t max_points;     /* P capacity                                                     */
  int32_t max_particles;  /* N capacity (uniform across points)                             */
  int32_t n_observers;    /* O                                                              */
  int32_t max_tile;       /* largest template side, tile_size <= max_tile (default 31)      */
  int32_t max_search_dim; /* search tiles up to max_search_dim^2 pixels per point           */
  int32_t max_frames;     /* moments history capacity (frames per sequence)                 */
  int32_t reserved;
} glh_config;

/* ---- library / context ---------------------------------------------------------------- */
int glh_version(void);
const char* glh_last_error(void);
int glh_device_count(int* count);
/* Free and total bytes of device `device_id` (hipMemGetInfo): the Python Tracker bounds the growth of its search-tile
   workspaces by them (it re-runs a sequence with larger workspaces when a tile outgrows them, tracker.py has no such
   limit: its tiles live in host memory).                                                                              */
int glh_device_memory(int device_id, uint64_t* free_bytes, uint64_t* total_bytes);
/* Compute units of device `device_id`: what glh_track's automatic choice of streams compares a batch with.           */
int glh_device_compute_units(int device_id, int* count);
int glh_create(const glh_config* cfg, glh_ctx** out);
int glh_destroy(glh_ctx* ctx);
int glh_sync(glh_ctx* ctx);
/* The HIP stream (hipStream_t) the context enqueues on, for event timing by the caller.   */
int glh_get_stream(glh_ctx* ctx, void** stream);

/* ---- observers: images + cameras ------------------------------------------------------ */
/* Observer(images, sigma) (track/observer.py:50-69).  Declares the image list size, the
 * frame geometry and `sigma`; frames are resident in HBM for the whole sequence.          */
int glh_observer_init(glh_ctx* ctx, int obs, int n_images, int width, int height, int channels,
                      double sigma);
/* Sample type of the observer's frames: 8 (default, uint8), 16 (uint16), 32 (float32) or 64 (float64), one or three
 * channels -- Tracker.extract_tile works on any dtype (tracker.py:494-534) and normalises a float tile in the frame's
 * own dtype (a float32 mean / std in NumPy's summation order).  After glh_observer_init, before the first upload; the
 * upload calls then copy width * height * channels * bits / 8 bytes.  16-bit observers run on the fused step while
 * max_search_dim <= 255 (a tile's pixel count is then a 16-bit key), on the staged kernels beyond; float observers on the
 * staged kernels (the pixels at or below every pixel of a tile by a two-level ranking over the tile's value range).     */
int glh_observer_set_depth(glh_ctx* ctx, int obs, int bits);
/* One Camera per image (Image.cam, image.py:110; Camera.R camera.py:239-280 is evaluated
 * on the host in float64 at upload).  cams: [n_images][GLH_CAM_LEN].                      */
int glh_observer_set_cameras(glh_ctx* ctx, int obs, int first_image, int n_images,
                             const double* cams);
/* Image.read() cached array (image.py:180-186): uint8 [height][width][channels].          */
int glh_observer_upload_frame(glh_ctx* ctx, int obs, int image, const uint8_t* pixels);
/* The same without waiting for the device (frame ingest from files: a decoder pool feeds this call).
 * `pixels` is copied to a pinned staging buffer before the call returns; the host-to-device copy runs
 * on a copy stream and every later call that reads frames is ordered after it on the device.      */
int glh_observer_upload_frame_async(glh_ctx* ctx, int obs, int image, const uint8_t* pixels);
/* Frame ingest without the staging copy (round 5): a host buffer the caller registers ONCE -- e.g. the shared-memory ring
 * its decoder processes fill (glimpse_amd/ingest.py) -- is page-locked for the device, and glh_observer_upload_frame_pinned
 * enqueues the host-to-device copy on the copy stream straight from `pixels`, which must lie inside a registered buffer and
 * stay untouched until glh_upload_done reports the copy `*ticket` identifies as finished (`wait` != 0: blocks until it is).
 * Ordering against the kernels is that of glh_observer_upload_frame_async.                                              */
int glh_host_register(void* ptr, uint64_t bytes);
int glh_host_unregister(void* ptr);
int glh_observer_upload_frame_pinned(glh_ctx* ctx, int obs, int image, const uint8_t* pixels, int64_t* ticket);
int glh_upload_done(glh_ctx* ctx, int64_t ticket, int wait, int* done);
/* Same, from a buffer that is already on the device (no PCIe in the timed region).        */
int glh_observer_set_frame_device(glh_ctx* ctx, int obs, int image, const void* dev_pixels);

/* ---- points (tracks) ------------------------------------------------------------------- */
/* Number of tracked points P and particles per point N for this sequence; clears state
 * (Tracker.reset, track/tracker.py:419-423).                                               */
int glh_begin_sequence(glh_ctx* ctx, int n_points, int n_particles, int tile_w, int tile_h);
/* CartesianMotion parameters per point: [P][GLH_MOTION_LEN] (track/motion.py:121-147).     */
int glh_set_motion_cartesian(glh_ctx* ctx, const double* params);
/* Any mix of motion models, one per point: [P][GLH_MOTION_FULL_LEN].  The tangent models return
 * no log likelihood (base Motion.compute_log_likelihoods, motion.py:76-89): a frame on which every
 * observer is skipped leaves their weights unchanged (tracker.py:146-149).  Points that are not
 * CartesianMotion run through the staged kernels.                                             */
int glh_set_motion(glh_ctx* ctx, const double* params);
/* Gridded surfaces (Raster, raster.py:613-): `which` = GLH_RASTER_DEM / _DEM_SIGMA (sampled
 * bilinearly at every particle, Raster.sample order 1, raster.py:913-1027) or _VIEWSHED (nearest
 * cell, order 0, Tracker.test_particles tracker.py:114-117).  z [ny][nx] is Raster.array; gx / gy are
 * the ASCENDING cell-centre coordinates (Grid.x / Grid.y reversed where dx / dy < 0); sx, sy the signs
 * of dx, dy; the limits are Grid.min / Grid.max.  z = NULL removes the raster.  nx, ny >= 2.  The coordinates must be
 * those of a uniform grid over the limits (np.linspace, as Grid makes them) to within a quarter cell:
 * GLH_E_UNSUPPORTED otherwise (the kernels find a sample's cell from the cell size).                  */
#define GLH_RASTER_DEM 0
#define GLH_RASTER_DEM_SIGMA 1
#define GLH_RASTER_VIEWSHED 2
int glh_set_raster(glh_ctx* ctx, int which, const double* z, int nx, int ny, const double* gx,
                   const double* gy, int sx, int sy, double xmin, double xmax, double ymin, double ymax);
/* Global index of this context's point 0 when the tracked points are sharded over several
 * contexts / GPUs (default 0).  The device RNG (GLH_RNG_PHILOX) is keyed on the GLOBAL point
 * index, so a sharded run draws exactly what the unsharded run draws.                        */
int glh_set_point_offset(glh_ctx* ctx, int offset);
/* observer_mask [P][O] (track/tracker.py:250-252, :289-290); NULL = all ones.              */
int glh_set_observer_mask(glh_ctx* ctx, const uint8_t* mask);
/* active [P]: 1 = the point takes part in the following stage calls (frames inside its
 * [first, last] window, track/tracker.py:321-326); NULL = all active.                      */
int glh_set_active(glh_ctx* ctx, const uint8_t* active);

int glh_set_particles(glh_ctx* ctx, const double* particles); /* [P][N][6] */
int glh_get_particles(glh_ctx* ctx, double* particles);
int glh_set_weights(glh_ctx* ctx, const double* weights);
/* A log-likelihood term computed by the caller for the NEXT glh_update_weights calls, ll [P][N] (NULL removes it):
 * Motion.compute_log_likelihoods of a user-defined motion model (motion.py:74-89), appended to the observers' terms
 * like the built-in one (tracker.py:139-149).                                                                    */
int glh_set_extra_log_likelihoods(glh_ctx* ctx, const double* ll); /* [P][N] */
int glh_get_weights(glh_ctx* ctx, double* weights);
int glh_get_point_status(glh_ctx* ctx, uint32_t* status);    /* [P]    GLH_PT_* bits        */
/* Frame index (glh_set_frame) at which each point first raised a status bit, or a large
 * value if none: the reference aborts the track there, so rows >= this frame are NaN
 * (track/tracker.py:360-368).                                                               */
int glh_get_point_error_frame(glh_ctx* ctx, int32_t* frames); /* [P] */
int glh_get_observer_status(glh_ctx* ctx, int32_t* status);
/* The same for frames [frame0, frame0 + n_frames): status [n_frames][O][P] (every frame of a sequence keeps its own
 * status words, so a run of glh_track frames can be inspected afterwards: one warning per skipped image and track,
 * tracker.py:597-601).                                                                                      */
int glh_get_observer_status_frames(glh_ctx* ctx, int frame0, int n_frames, int32_t* status);
/* Particles [N][6] and weights [N] of ONE point (either may be NULL): what the reference's Tracker.particles /
 * .weights hold after the last track (tracker.py:35-37).                                                       */
int glh_get_point_state(glh_ctx* ctx, int point, double* particles, double* weights);  /* [O][P] GLH_OBS_*            */
/* Search boxes (l,t,r,b) of the last glh_update_weights (tracker.py:595): [O][P][4];
 * entries whose observer status is not GLH_OBS_OK are stale.                                */
int glh_get_search_boxes(glh_ctx* ctx, int32_t* boxes);

/* ---- stages of one frame (track/tracker.py:326-357), in the reference's order ---------- */
/* Index i of the datetime being processed (track/tracker.py:326); recorded with errors.     */
int glh_set_frame(glh_ctx* ctx, int frame);
/* CartesianMotion.initialize_particles (track/motion.py:149-163) + initialize_weights
 * (track/tracker.py:121-124).  GLH_RNG_HOST: normals [P][N][6] = randn(n,2)|randn(n)|randn(n,3). */
int glh_init_particles(glh_ctx* ctx, int rng_mode, const double* normals, uint64_t seed);
/* CartesianMotion.evolve_particles (track/motion.py:165-179) + test_particles NaN check
 * (track/tracker.py:118-119).  tau = dt / time_unit.  GLH_RNG_HOST: normals [P][N][3].     */
int glh_evolve(glh_ctx* ctx, double tau, int rng_mode, const double* normals, uint64_t seed,
               uint64_t step);
/* Tracker.initialize_template (track/tracker.py:536-561) for observer `obs` at image
 * `image`, for every active point with the observer enabled: weighted mean -> project ->
 * Grid.snap_box (raster.py:390-421) -> extract_tile (tracker.py:494-534).                 */
int glh_init_templates(glh_ctx* ctx, int obs, int image);
/* Tracker.update_weights (track/tracker.py:126-149): for each observer o with
 * images[o] >= 0, compute_observer_log_likelihoods (tracker.py:563-625); plus
 * CartesianMotion.compute_log_likelihoods (motion.py:181-204); w = exp(-sum) + 1e-300.     */
int glh_update_weights(glh_ctx* ctx, const int32_t* images /* [O], -1 = None */);

/* Tracker.resample_particles("systematic") (track/tracker.py:168-176, :222-223).
 * GLH_RNG_HOST: u [P] = the np.random.random() draw of each point.                         */
int glh_resample(glh_ctx* ctx, int rng_mode, const double* u, uint64_t seed, uint64_t step);
/* Same with an explicit method (GLH_RESAMPLE_*).  GLH_RNG_HOST: u is [P] for systematic (the
 * np.random.random() of each point) and [P][N] for stratified (np.random.random(n)), choice (the n
 * uniforms RandomState.choice draws) and residual (np.random.random(n - sum(repetitions)): the first
 * n - R entries of each row are used; glh_get_residual_draws returns the counts).  Residual follows the
 * reference's arithmetic literally (repetition counts subtracted from normalised weights, then
 * np.searchsorted's stateful bisection over a cumulative sum that is not monotone).            */
int glh_resample_method(glh_ctx* ctx, int method, int rng_mode, const double* u, uint64_t seed,
                        uint64_t step);
/* Tracker.particle_covariance (track/tracker.py:78-82; np.cov(aweights=w, ddof=0)) of every
 * active point into history slot `frame`; glh_get_covariances: out [n_frames][P][36].       */
/* Number of uniforms the last GLH_RESAMPLE_RESIDUAL step consumed per point, n - sum(repetitions)
 * (tracker.py:199-201): draws [P].  Lets a host that feeds np.random keep its stream aligned.   */
int glh_get_residual_draws(glh_ctx* ctx, int32_t* draws);
int glh_record_covariances(glh_ctx* ctx, int frame);
int glh_get_covariances(glh_ctx* ctx, int frame0, int n_frames, double* out);
/* particle_mean + compute_particle_sigma (track/tracker.py:72-76, :89-104) of every active
 * point into history slot `frame` (rows of inactive points keep NaN).                      */
int glh_record_moments(glh_ctx* ctx, int frame);
/* evolve -> update_weights -> resample -> record_moments: the per-frame step i > first of
 * track/tracker.py:331-357 for all active points, enqueued back to back.                   */
int glh_step(glh_ctx* ctx, int frame, double tau, const int32_t* images, int rng_mode,
             const double* normals, const double* u, uint64_t seed);
/* The whole frame loop of every track (track/tracker.py:326-357: `for i, img in enumerate(...)` of
 * process()) in one call: n_frames consecutive glh_step updates with GLH_RNG_PHILOX, enqueued back
 * to back on the context's stream without host synchronisation.  frames [n_frames] = history
 * slots / Philox steps, taus [n_frames] = dt / time_unit of each update, images [n_frames][O]
 * (-1 = None).  Same results as the same glh_step calls.                                       */
int glh_track(glh_ctx* ctx, int n_frames, const int32_t* frames, const double* taus, const int32_t* images,
              uint64_t seed);
/* on = 1: glh_track also records the covariance of the particles after every frame it runs (glh_record_covariances:
 * Tracker.track(return_covariances=True), track/tracker.py:307-308, :352), so that such a run is still one call.   */
int glh_track_covariances(glh_ctx* ctx, int on);
/* Streams of glh_track's frame loop.  The tracks of the reference are independent (track/tracker.py:381-387 hands them
 * to a process pool); here the two halves of a large batch run their frame loops on two HIP streams, so that one
 * half's launch fills the compute units the other half's launch leaves idle while it drains and refills (bit for bit
 * the results of one stream).  0 (default) = automatic: two streams when the batch has more points than the device has
 * compute units (a launch ends with its slowest point: the halves fill each other's tails); 1 = one stream; 2 = two
 * streams whenever the fused step runs.                                                                                */
int glh_set_track_streams(glh_ctx* ctx, int n);

/* glh_step implementation: 1 (default) = the fused per-point kernel (weights + resample +
 * re-evolving gather + moments in one launch, evolved state never round-trips through HBM)
 * whenever no active mask / debug capture is in force; 0 = always the staged kernels
 * (glh_evolve -> glh_update_weights -> glh_resample); 2 = fused, but with every search tile
 * forced into the HBM workspaces (test hook for the large-tile path).  All give the same
 * particles bit for bit.                                                                      */
int glh_set_fused(glh_ctx* ctx, int on);
/* GLH_MATH_EXACT (default) or GLH_MATH_FAST for every kernel of this context (the staged and the fused kernels use
 * the same arithmetic in either mode, so they stay bit-identical to each other).                                */
int glh_set_math(glh_ctx* ctx, int mode);
/* Window of the median high-pass filter of every tile (Tracker(highpass={"size": (size_y, size_x)}), tracker.py:59,
 * :530: scipy.ndimage.median_filter): odd sizes up to 7; 5 x 5 (the reference default) unless set.                                                                                           */
int glh_set_highpass(glh_ctx* ctx, int size_x, int size_y);
/* Boundary mode of that filter (Tracker(highpass={"size": ..., "mode": ...}): tracker.py:530 hands the dictionary to
 * scipy.ndimage.median_filter): 0 'reflect' (scipy's default, and the reference's), 1 'nearest', 2 'mirror', 3 'wrap'.
 * ('constant' needs a fill value in the matched tile's units: not served.)                                             */
int glh_set_highpass_mode(glh_ctx* ctx, int mode);
/* Orders of the spline that samples the SSD surface at the particles (Tracker(interpolation={"kx": .., "ky": ..}),
 * tracker.py:60, :585-590, :623: scipy RectBivariateSpline(kx, ky), s = 0): (3, 3), the reference default, or (1, 1)
 * -- bilinear; any other orders 1 .. 5 (kx: rows axis, ky: columns axis): the interpolating spline of those degrees with
 * FITPACK's knots, banded solves of bandwidth k, on the staged kernels.  The orders also set the least size of the
 * surface (the search box is widened to ky + 1 columns and kx + 1 rows, tracker.py:585-590).                        */
int glh_set_interpolation(glh_ctx* ctx, int kx, int ky);

/* Diagnostic: the numbers of the GLH_RNG_PHILOX streams of this context's points (global indices point_offset ..),
 * so that a parity test can hand the CPU oracle the draws a device-RNG run consumed -- the role np.random plays in
 * the reference (motion.py:156-162, :176; tracker.py:173).  kind 0: initialisation normals out [P][N][6] in the order
 * randn(n,2) | randn(n) | randn(n,3); kind 1: the evolve normals of frame `step`, out [P][N][3]; kind 2: the
 * systematic resampling offset of frame `step`, out [P].  `step` is the frame index passed to glh_step.          */
int glh_debug_draws(glh_ctx* ctx, int kind, uint64_t seed, uint64_t step, double* out);
/* Diagnostic: s_memtime stamps [P][24] at the phase boundaries of the fused kernel during the
 * last fused glh_step (the first call only arms them and returns zeros).                      */
int glh_debug_phase_stamps(glh_ctx* ctx, uint64_t* stamps);
/* Diagnostic: which instantiation of the fused kernel took the last fused glh_step / glh_track frame:
 * variant[0..3] = threads per workgroup, particles kept in registers per thread, observers, flags (bit 0: fast
 * arithmetic, bit 1: the general code (gridded surfaces, every motion model), bit 2: the compile-time contract of long
 * device-RNG runs; flags == 5 is the common instantiation bench.py times).  Zeros before any.                    */
int glh_debug_last_variant(glh_ctx* ctx, int32_t* variant);
/* Streams the last glh_track call ran on (1 or 2). */
int glh_debug_last_track_streams(glh_ctx* ctx, int* n);

/* ---- results --------------------------------------------------------------------------- */
/* means/sigmas for frames [frame0, frame0 + n_frames): out [n_frames][P][12].              */
int glh_get_moments(glh_ctx* ctx, int frame0, int n_frames, double* out);
/* The same history in the layout of the reference's Tracks (tracks.py:52-88): means [P][n_frames][6] and sigmas
 * [P][n_frames][6], rearranged on the device (no host-side transposes of tens of megabytes).                    */
int glh_get_tracks(glh_ctx* ctx, int frame0, int n_frames, double* means, double* sigmas);
/* Device pointer + byte size of the moments history [max_frames][P][12] (for an RCCL
 * gather issued by the caller; no copy).                                                    */
int glh_get_moments_device(glh_ctx* ctx, void** dev_ptr, uint64_t* bytes);
/* Template of (obs, point): box[4], duv[2], tile [th][tw], histogram (values, quantiles)
 * (track/tracker.py:552-561).  hist_n receives the number of CDF entries (<= th*tw).       */
int glh_get_template(glh_ctx* ctx, int obs, int point, int32_t* box, double* duv, double* tile,
                     double* hist_values, double* hist_quantiles, int32_t* hist_n);
/* Intermediates of the last glh_update_weights for (obs, point), for parity tests:
 * uv [N][2], box[4] (l,t,r,b), search tile float32 [Hs][Ws], sse float64 [Ho][Wo] (the
 * float32 SSE surface widened, before the spline fit).  Any pointer may be NULL.           */
int glh_get_likelihood_debug(glh_ctx* ctx, int obs, int point, double* uv, int32_t* box,
                             float* search, double* sse);
/* keep = 1: keep a copy of the SSE surface before the in-place spline fit, the per-observer log
 * likelihoods and the resample indices (costs extra passes and takes glh_step through the staged
 * kernels; off by default, on for parity tests).  keep = 2: the resample indices only (glh_step
 * stays on the fused kernel).                                                                  */
int glh_set_debug(glh_ctx* ctx, int keep);
/* Per-observer log likelihoods of the last glh_update_weights, i.e. the return value of
 * compute_observer_log_likelihoods (track/tracker.py:563-625): ll [P][N], NaN where the
 * reference returns None (needs glh_set_debug).                                              */
int glh_get_log_likelihoods(glh_ctx* ctx, int obs, double* ll);
/* np.searchsorted result of the last glh_resample (needs glh_set_debug): idx [P][N].        */
int glh_get_resample_indices(glh_ctx* ctx, int32_t* idx);
/* Per-stage device time (ms, HIP events on the context's stream) accumulated since the
 * last reset: names in glh_stage_name(i), i < glh_stage_count().                            */
int glh_profile_enable(glh_ctx* ctx, int on);
int glh_profile_reset(glh_ctx* ctx);
int glh_stage_count(void);
const char* glh_stage_name(int stage);
/* `launches` counts kernel launches: when glh_track runs a batch on two streams (glh_set_track_streams) a frame update
 * is TWO launches of the fused step, one per half of the points.                                                  */
int glh_profile_get(glh_ctx* ctx, double* ms /* [stages] */, int64_t* launches /* [stages] */);
/* Duration (ms) of every timed launch of `stage` since the last reset, in launch order: up to `cap` values
 * into ms, *n = how many there are (the first frames after the wide prior run longer than the steady state). */
/* GPU time (ms) a stage spans since the last reset: start of its first timed launch to the end of its last, on whichever
 * stream (the launches of glh_track's two streams overlap, so their durations do not add up to the time they take).  */
int glh_profile_get_span(glh_ctx* ctx, int stage, double* ms);
int glh_profile_get_launches(glh_ctx* ctx, int stage, double* ms, int cap, int* n);
/* Measured device-copy ceiling of this GPU: `iters` device-to-device copies of `bytes`
 * bytes on the context's stream between two HIP events; *gbps = bytes read + bytes written per second / 1e9. */
int glh_measure_copy_bandwidth(glh_ctx* ctx, uint64_t bytes, int iters, double* gbps);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ------------------------------------------
 * The reference's one parallel seam is a map over tracks (track/tracker.py:381-387,
 * `config.backend(np=parallel)`, helpers.py:2008-2017): tracks are independent, so here every process owns
 * one GPU, one context and a contiguous block of the tracked points (glh_set_point_offset), nothing is
 * exchanged while a sequence runs, and at its end the per-point posterior moments are collected on one rank.
 * librccl is loaded on the first of these calls (dlopen), never by a single-GPU user.                  */
#define GLH_COMM_ID_BYTES 128
/* One rank (the root) makes the communicator id (ncclGetUniqueId) and hands its 128 bytes to the others by
 * whatever the launcher offers (glimpse_amd/sharding.py: a file store under MASTER_PORT).               */
int glh_comm_unique_id(char* id /* [GLH_COMM_ID_BYTES] */);
/* Join the communicator as `rank` of `world` on the context's device and stream (ncclCommInitRank:
 * collective, every rank calls it).                                                                    */
int glh_comm_init(glh_ctx* ctx, const char* id, int rank, int world);
int glh_comm_destroy(glh_ctx* ctx);
/* Every rank's stream has reached this point (an all-reduce of one word, then a stream sync).            */
int glh_comm_barrier(glh_ctx* ctx);
/* *value = max over the ranks of *value (host double; wall-clock maxima of a timed region).              */
int glh_comm_max_f64(glh_ctx* ctx, double* value);
/* The one collective of a sequence: frames [frame0, frame0 + n_frames) of every rank's moments history
 * ([n_frames][P_rank][12], what `process` returns per track, tracker.py:370-373) and its per-point status
 * words to rank `root`, as ONE group of ncclSend / ncclRecv on the context's stream.  points_per_rank
 * [world]; on the root `out` receives | rank 0: [n_frames][P_0][12] | rank 1: ... | and `status` (or NULL)
 * | P_0 | P_1 | ... |; other ranks pass NULL.  Blocks until the exchange is over.                        */
int glh_gather_moments(glh_ctx* ctx, int root, int frame0, int n_frames, const int32_t* points_per_rank,
                       double* out, uint32_t* status);
/* On the root, `out` may be NULL: the blocks then stay in the root's device memory (the exchange is all the call does)
 * and glh_get_gathered copies them to the host later, in the layout above.                                        */
int glh_get_gathered(glh_ctx* ctx, double* out, uint32_t* status);

/* ---- stage-level test hooks (stateless; each runs one kernel on explicit inputs) -------- */
/* Camera.xyz_to_uv (camera.py:591-628): xyz [n][3] -> uv [n][2].                            */
int glh_stage_project(int device_id, const double* cam, const double* xyz, int n, double* uv);
/* Same with xyz read as ray directions relative to the camera (directions=True, camera.py:1448).  */
int glh_stage_project_directions(int device_id, const double* cam, const double* xyz, int n, double* uv);
/* Camera.xyz_to_uv(return_depth=True) (camera.py:591-628, :1468-1469): uv [n][2] and the distance of every
 * point along the optical axis, depth [n] (also for points behind the camera, whose uv are NaN).   */
int glh_stage_project_depth(int device_id, const double* cam, const double* xyz, int n, int directions,
                            double* uv, double* depth);
/* The projection of GLH_MATH_FAST (csrc/glh_math.h: project_fast with the camera's flags) on explicit points, as
 * glh_stage_project runs the exact one; directions != 0 reads xyz as ray directions (GLH_E_INVALID for a raster grid).
 * simple != 0 runs project_simple_fast, the form the fused kernel's common instantiation compiles: GLH_E_INVALID for a
 * camera it does not cover (a raster grid, k4..k6, tangential terms, the elevation correction) and with directions.  */
int glh_stage_project_fast(int device_id, const double* cam, const double* xyz, int n, int directions, int simple,
                           double* uv);
/* One primitive of GLH_MATH_FAST (csrc/glh_math.h, csrc/glh_kernels.h) on n rows of GLH_FM_ARGS doubles, one thread per
 * row: out [n].  Which columns an op reads:
 *   RCP, SQRT, EXP     x                      rcp_nr, sqrt_nr; exp_fast on the table the device makes (as the weights kernel)
 *   WEIGHT             ll                     weight_of: exp(-ll) + 1e-300
 *   MIN_NN, MAX_NN     a, b
 *   COUNT_FRACTION     k, n                   count_fraction(k, n, 1.0 / n), k an integer in an int's range
 *   COUNT_LE           ck, scale, u, n        count_le_fast, the count as a double
 *   BILINEAR           z00, z10, z01, z11, tx, ty   raster_bilinear_fast
 * GLH_E_INVALID: a null pointer, n <= 0, another op.                                                                 */
#define GLH_FM_ARGS 8
#define GLH_FM_RCP 0
#define GLH_FM_SQRT 1
#define GLH_FM_EXP 2
#define GLH_FM_WEIGHT 3
#define GLH_FM_MIN_NN 4
#define GLH_FM_MAX_NN 5
#define GLH_FM_COUNT_FRACTION 6
#define GLH_FM_COUNT_LE 7
#define GLH_FM_BILINEAR 8
int glh_stage_fast_math(int device_id, int op, const double* args, int n, double* out);
/* Camera.uv_to_xyz (camera.py:630-663): uv [n][2] -> xyz [n][3]; depth NULL (= 1), [1] or [n];
 * undistortion by the closed form for k1 alone, else 20 Oulu iterations (camera.py:1198-1337).   */
int glh_stage_unproject(int device_id, const double* cam, const double* uv, int n, const double* depth,
                        int n_depth, int directions, double* xyz);
/* Image.project (image.py:301-361): n_frames >= 1 frames of one shape [n_frames][height][width][channels], each with its
 * own camera src_cams [n_frames][GLH_CAM_LEN], resampled into the camera dst_cam at the same position: out
 * [n_frames][dst_height][dst_width][channels] in the frames' own type.  depth_bits / is_float: 8 / 0, 16 / 0 (unsigned),
 * 32 / 1, 64 / 1; channels 1 or 3; method 0 = linear, 1 = nearest, on the grid of the source pixel centres as
 * scipy.interpolate.RegularGridInterpolator(bounds_error=False) evaluates them.  Pixels that see nothing of the frame are
 * NaN in float frames and 0 in integer frames.  Frames travel through pinned staging buffers on streams of their own, so
 * that a frame's copies overlap its neighbours' kernels.  kernel_ms (or NULL): the sum of the kernels' durations, from
 * events.  GLH_E_UNSUPPORTED: a raster grid as camera, another type, channel count or method; GLH_E_INVALID: cameras at
 * different positions ('xyz'), camera imgsz that differ from the frame sizes.                                            */
int glh_stage_reproject(int device_id, const void* frames, int depth_bits, int is_float, int width, int height,
                        int channels, int n_frames, const double* src_cams, const double* dst_cam, int dst_width,
                        int dst_height, int method, void* out, double* kernel_ms);
/* Tracker.extract_tile(return_histogram=True) (tracker.py:494-534) on a uint8 frame crop
 * `box` (l,t,r,b): tile float64 [h][w], CDF values/quantiles, n entries.                    */
int glh_stage_template(int device_id, const uint8_t* frame, int width, int height, int channels,
                       const int32_t* box, double* tile, double* hist_values,
                       double* hist_quantiles, int32_t* hist_n);
/* Tracker.extract_tile(histogram=...) (tracker.py:494-534): search tile float32 [h][w].     */
int glh_stage_search_tile(int device_id, const uint8_t* frame, int width, int height,
                          int channels, const int32_t* box, const double* hist_values,
                          const double* hist_quantiles, int hist_n, float* tile);
/* The two tile hooks with another high-pass window (odd sizes up to 7) and boundary mode (glh_set_highpass_mode).   */
int glh_stage_template_highpass(int device_id, const uint8_t* frame, int width, int height, int channels,
                                const int32_t* box, int size_x, int size_y, int mode, double* tile,
                                double* hist_values, double* hist_quantiles, int32_t* hist_n);
int glh_stage_search_tile_highpass(int device_id, const uint8_t* frame, int width, int height, int channels,
                                   const int32_t* box, const double* hist_values, const double* hist_quantiles,
                                   int hist_n, int size_x, int size_y, int mode, float* tile);
/* cv2.matchTemplate(TM_SQDIFF) * 1/(tw*th) (tracker.py:609-614): float32 in, float32 out.   */
int glh_stage_ssd(int device_id, const float* search, int hs, int ws, const float* templ, int th,
                  int tw, float* sse);
/* Observer.sample_tile (observer.py:178-214): sse float32 [ho][wo], box (4 doubles),
 * uv [n][2] -> values [n]; outside [n] flags points outside the box.                         */
int glh_stage_sample(int device_id, const float* sse, int ho, int wo, const double* box,
                     const double* uv, int n, double* values, uint8_t* outside);
/* The same for any orders of RectBivariateSpline (kx: rows axis, ky: columns axis, each 1 .. 5; Tracker(interpolation=
 * {"kx": ..., "ky": ...}), tracker.py:60, :623): ho >= kx + 1, wo >= ky + 1.                                          */
int glh_stage_sample_orders(int dev, const float* sse, int ho, int wo, int kx, int ky, const double* box,
                            const double* uv, int n, double* values, uint8_t* outside);
/* Raster.sample(xy, order) (raster.py:913-1027) at n points: values [n], oob [n] = 1 where the
 * reference would raise (outside the outer limits).                                            */
int glh_stage_raster_sample(int device_id, const double* z, int nx, int ny, const double* gx,
                            const double* gy, int sx, int sy, double xmin, double xmax, double ymin,
                            double ymax, const double* xy, int n, int order, double* values,
                            uint8_t* oob);
/* Raster.viewshed(origin, correction) (raster.py:1293-1389) for m >= 1 origins [m][3] over ONE upload of the DEM:
 * visible [m][ny][nx], 1 = seen from the origin.  z [ny][nx] is Raster.array as float64 (z_dtype GLH_VIEWSHED_F64) or as
 * float32 (GLH_VIEWSHED_F32: the reference's `array.ravel() - origin[2]` stays float32 -- a float32 DEM and an origin
 * NumPy does not promote it with -- so the subtraction and the correction's sum are rounded to float32).  x [nx], y [ny]
 * are Grid.x / Grid.y as NumPy made them (first to last column / row, either direction); inv_cell = 1 / abs(d[0]).
 * correction != 0 adds helpers.elevation_corrections (helpers.py:1771-1790) with `radius` and `refraction`.  The
 * reference's algorithm and its quirks: cells ordered by ring (distance in cells, rounded) and heading, rings swept in
 * ascending order with the previous ring's running maximum interpolated as np.interp(period=2 pi) does; a ring 0 beside
 * other rings is never processed (the cell under the origin is 0); cells that all lie in ring 0 are all 1.
 * times_ms (or NULL) [8]: HIP-event milliseconds summed over the origins -- [0] upload, [1] per-cell kernel, [2] sort,
 * [3] sweep, [4] download -- then [5] rings processed, [6] sweep launches, [7] bytes of the sort's scratch.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, nx, ny or m < 1, nx * ny >= 2^31, coordinates,
 * origins or inv_cell that are not finite, radius 0), GLH_E_UNSUPPORTED (an unknown z_dtype; an origin more than 2^24
 * cells from the DEM).  A failed device allocation is GLH_E_NOMEM, with the bytes it asked for in glh_last_error().    */
#define GLH_VIEWSHED_F64 0
#define GLH_VIEWSHED_F32 1
int glh_stage_viewshed(int device_id, const void* z, int z_dtype, int nx, int ny, const double* x, const double* y,
                       double inv_cell, const double* origins, int m, int correction, double radius,
                       double refraction, uint8_t* visible, double* times_ms);
/* Raster.horizon(origin, headings, correction) (raster.py:1391-1463) for m >= 1 origins [m][3] with n headings each, over
 * ONE upload of the DEM.  z, z_dtype (GLH_VIEWSHED_F64 / _F32), correction, radius and refraction as in glh_stage_viewshed;
 * xlim0, ylim0 = the outer corner of cell (row 0, col 0) and d0, d1 = Grid.d as NumPy made it, with its signs: the centre
 * of a cell is ((col + 0.5) d0 + xlim0, (row + 0.5) d1 + ylim0) (rowcol_to_xy, raster.py:461-476).  The rays are the
 * caller's: starts [m][2] = the (col, row) of each origin's cell, ends [m][n][2] = the (col, row) where each ray leaves
 * the grid (the host keeps NumPy's cos / sin).  Per (origin, heading) the cells of helpers.bresenham_line(start, end)
 * after the start cell are taken, each with dz = z - origin z (float32 under _F32, widened afterwards) and the ratio
 * dz / sqrt(dxy) -- (dz + (refraction - 1) dxy / (2 radius)) / sqrt(dxy) with correction -- in float64, operation by
 * operation as NumPy rounds them.  A NaN dz makes a cell missing.  The horizon cell is the one of greatest ratio, the
 * first among equals (np.nanargmax), and only if a cell that is not missing lies beyond it.
 * cell [m][n][2] int32 = its (row, col), -1 -1 where the heading has no horizon point; dz [m][n] = its dz (NaN there).
 * One workgroup per line, the cell index in closed form, a fixed-order reduction: two calls give the same bytes.
 * times_ms (or NULL) [3]: HIP-event milliseconds -- [0] upload, [1] kernel, [2] download.
 * Elevations are finite or NaN: with +-inf in z the choice among cells of ratio -inf or NaN is not np.nanargmax's.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, nx, ny, m or n < 1, nx * ny >= 2^31, m * n >= 2^24
 * (a launch of one workgroup per line holds fewer than 2^32 lanes), a start or end cell outside the grid, origins, corner
 * or cell sizes that are not finite, a cell size of 0, radius 0 with correction), GLH_E_UNSUPPORTED (an unknown z_dtype).
 * A failed device allocation is GLH_E_NOMEM.                                                                            */
int glh_stage_horizon(int device_id, const void* z, int z_dtype, int nx, int ny, double xlim0, double ylim0, double d0,
                      double d1, const double* origins, const int32_t* starts, const int32_t* ends, int m, int n,
                      int correction, double radius, double refraction, int32_t* cell, double* dz, double* times_ms);
/* Camera.project_dem (camera.py:967-1129) with scale_limits = (1, 1): the image a camera records of a DEM's per-cell
 * values, and the depth of the DEM along the optical axis.  out [height][width][layers + (return_depth != 0)] float64 with
 * (width, height) = the camera's imgsz; NaN where no cell lands.  cam [GLH_CAM_LEN] (a camera, not a raster grid).
 * z [ny][nx] is the DEM as float64 or float32 (z_dtype GLH_PD_F64 / GLH_PD_F32); mask [ny][nx] (0 = skip the cell) or NULL
 * (every cell; a NaN elevation never projects); values [ny][nx][layers] of v_dtype (GLH_PD_F64, _F32, _U8, _U16), NULL
 * with layers == 0.  The tiling is the caller's (Grid.tile_indices, raster.py:581-610; the device never re-derives it): the
 * tiles are the cross product of n_ty row slices [y_start[k], y_end[k]) and n_tx column slices [x_start[k], x_end[k]), in
 * row-major order; x_coords holds, slice after slice, the x of each column of the slice as the tile's own Grid.x has it
 * (sum of the widths entries), y_coords likewise per row slice.  A cell takes part in a tile when its mask is set, it lies
 * in front of the camera and its uv truncate to a pixel of the image (a uv exactly on the far edge, where the reference
 * raises, is out of frame).  Within a tile a pixel is sum * (1 / count) per layer, the sum in float64 in row-major cell
 * order as np.bincount forms it; across tiles the last tile that reaches a pixel overwrites the earlier ones (no depth
 * test).  The value layers are bit for bit the reference's, and two calls give identical bytes.
 * times_ms (or NULL) [8]: HIP-event milliseconds -- [0] upload, [1] project, [2] order (winners, sort, runs), [3] reduce,
 * [4] download -- then [5] memberships (cells summed over the tiles), [6] memberships kept, [7] bytes of the sort's scratch.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, sizes < 1, no layer at all, values without layers or
 * layers without values, slices that are empty, not ascending or outside the DEM, an imgsz that is not a positive
 * integer), GLH_E_UNSUPPORTED (an unknown dtype code, a raster grid as camera, 2^31 or more memberships, cells or
 * pixels).  A failed device allocation is GLH_E_NOMEM.                                                                 */
#define GLH_PD_F64 0
#define GLH_PD_F32 1
#define GLH_PD_U8 2
#define GLH_PD_U16 3
int glh_stage_project_dem(int device_id, const double* cam, const void* z, int z_dtype, int nx, int ny,
                          const uint8_t* mask, const void* values, int v_dtype, int layers, int n_tx,
                          const int32_t* x_start, const int32_t* x_end, const double* x_coords, int n_ty,
                          const int32_t* y_start, const int32_t* y_end, const double* y_coords, int return_depth,
                          double* out, double* times_ms);
/* Camera.rasterize (camera.py:858-883; helpers.rasterize_points, helpers.py:1617-1698): n points, each with its pixel
 * keys [n] in [0, n_pixels) and values [n][layers] float64, to out [n_pixels][layers]: per pixel sum * (1 / count) with
 * the sum in the points' order, NaN without a point.  The sort and the reduction are glh_stage_project_dem's.  times_ms as
 * there ([1] is the index fill; [5] = [6] = n).  GLH_E_INVALID before a device is touched: null pointers, n, layers or
 * n_pixels < 1, a key outside [0, n_pixels).                                                                          */
int glh_stage_rasterize(int device_id, const int32_t* keys, int n, const double* values, int layers, int n_pixels,
                        double* out, double* times_ms);
/* Image.orthorectify (the inverse of Camera.project_dem; the reference has no single function for it -- the rule is
 * INPUTS.md, "Orthorectification: the rule"): n_frames >= 1 frames of one shape [n_frames][height][width][channels]
 * (depth_bits / is_float and channels as for glh_stage_reproject), each with its own camera cams [n_frames][GLH_CAM_LEN],
 * resampled onto the grid of the DEM z [ny][nx] (z_dtype GLH_PD_F64 / GLH_PD_F32) whose cell centres are x [nx] by
 * y [ny], in whichever direction they run: out [n_frames][ny][nx][channels], float32 for float32 frames and float64 for
 * every other.  A cell's value is the frame at Camera.xyz_to_uv((x, y, z)), method 0 = linear, 1 = nearest, on the grid
 * of the pixel centres as scipy.interpolate.RegularGridInterpolator(bounds_error=False) evaluates them; NaN where the
 * elevation is NaN, the cell is behind the camera or lands off the pixel centres, or its mask is 0.  seen (or NULL:
 * every cell) [n_seen][ny][nx]: the caller's mask and viewshed of a cell; seen_of [n_frames] (or NULL: the first) names
 * each frame's.  The DEM and the masks are uploaded once; frames travel as in glh_stage_reproject, one kernel each.
 * kernel_ms (or NULL): the sum of the kernels' durations, from events.  Before a device is touched, GLH_E_UNSUPPORTED: a
 * raster grid as camera, another type, channel count or method; GLH_E_INVALID: null pointers, a camera imgsz that
 * differs from the frame size, a frame below 2 x 2 or a grid of 2^31 cells, seen_of outside [0, n_seen).               */
int glh_stage_orthorectify(int device_id, const void* frames, int depth_bits, int is_float, int width, int height,
                           int channels, int n_frames, const double* cams, const void* z, int z_dtype, int nx, int ny,
                           const double* x, const double* y, const uint8_t* seen, int n_seen, const int32_t* seen_of,
                           int method, void* out, double* kernel_ms);
/* Raster.intersect_rays, Camera.uv_to_dem and Camera.xyz_map: n rays P(t) = o + t d cast onto the bilinear surface between
 * the cell centres of the DEM z [ny][nx] (z_dtype GLH_PD_F64 / GLH_PD_F32; float32 is widened, all arithmetic is float64).
 * The reference has no such function; the rule is INPUTS.md, "Ray casting: the rule", restated in tests/raycast_rule.py,
 * which the device equals bit for bit.  x [nx], y [ny] are the cell centres from the first column / row to the last, in
 * either direction, and d0, d1 the raster's signed cell sizes: a ray is marched in grid coordinates (x - x[0]) / d0,
 * (y - y[0]) / d1 over the domain of the outer cell centres (the half-cell rim beyond them is not part of the surface).
 * The rays come from one of three sources (`mode`):
 *   GLH_RAYCAST_DIRECTIONS  rays [n][3] are directions, origins [n_origins][3] their origins, one each or one for all
 *                           (n_origins == 1); cam is NULL.
 *   GLH_RAYCAST_UV          rays [n][2] are image coordinates of the camera cam [GLH_CAM_LEN], unprojected on the device:
 *                           o = the camera's position, d = Camera.uv_to_xyz(uv, directions=True), so t is the depth along
 *                           the optical axis; origins is NULL.
 *   GLH_RAYCAST_GRID        the pixel centres (step / 2 + c step, step / 2 + r step) of the camera, c < imgsz[0] / step,
 *                           r < imgsz[1] / step, made on the device, ray r * cols + c; n must be cols * rows; rays and
 *                           origins are NULL.
 * correction != 0 lowers the apparent surface by helpers.elevation_corrections(t^2 (dx^2 + dy^2), radius, refraction), as
 * Camera.xyz_to_uv applies it.  block = 0 marches every patch; block = B, a power of two, first reduces the DEM to the
 * maxima of its B x B blocks of patches and lets a ray skip the blocks it clears: the results do not depend on it.
 * Per ray: t [n] (NaN without a hit), xyz [n][3] = o + t d, patch [n] = row * (nx - 1) + column of the patch hit (-1
 * without one) and status [n], one of GLH_RAYCAST_HIT, _MISS (the ray misses the domain), _BELOW (it enters the domain
 * below the surface), _LEAVES (it leaves the domain without a hit), _INVALID (a uv, direction or origin that is not
 * finite, or a direction of zero).
 * times_ms (or NULL) [4]: HIP-event milliseconds -- [0] upload, [1] pyramid (the block maxima), [2] march, [3] download.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, nx, ny or n < 1, step < 1, n_origins neither 1 nor
 * n, n that is not the grid's size, coordinates or cell sizes that are not finite, a cell size of 0, radius 0 with
 * correction), GLH_E_UNSUPPORTED (an unknown z_dtype or mode, a raster grid as camera, a DEM with a singleton dimension,
 * coordinates that are not those of a uniform grid to a quarter cell, 2^31 or more cells or rays, a block that is neither
 * 0 nor a power of two up to 32768).  A failed device allocation is GLH_E_NOMEM.                                     */
#define GLH_RAYCAST_DIRECTIONS 0
#define GLH_RAYCAST_UV 1
#define GLH_RAYCAST_GRID 2
#define GLH_RAYCAST_HIT 0
#define GLH_RAYCAST_MISS 1
#define GLH_RAYCAST_BELOW 2
#define GLH_RAYCAST_LEAVES 3
#define GLH_RAYCAST_INVALID 4
int glh_stage_raycast(int device_id, const void* z, int z_dtype, int nx, int ny, const double* x, const double* y,
                      double d0, double d1, int mode, const double* cam, const double* origins, int n_origins,
                      const double* rays, int n, int step, int correction, double radius, double refraction, int block,
                      double* t, double* xyz, int32_t* patch, uint8_t* status, double* times_ms);
/* glimpse_amd.displacements, Image.displacements and Observer.displacements: dense template matching between frames by
 * zero-normalised cross-correlation.  The reference has no such function; the rule is INPUTS.md, "Displacements: the
 * rule", restated in tests/displacement_rule.py, which the device equals bit for bit.  frames [n_frames][height][width],
 * uint8 (is_float == 0, the integer path) or float32 (is_float != 0); pairs [n_pairs][2] name, for each pair, the frame
 * the templates are cut from and the frame they are looked for in.  corners [n][2] are the (l, t) of each point's
 * template box [l, l + w) x [t, t + h), valid [n] is 0 where the caller found the box outside the frame (the device
 * checks the corners of the others again); guess (or NULL: none) holds whole-pixel guesses [n][2], or
 * [n_pairs][n][2] with guess_per_pair != 0, each within +-2^24.  The offsets searched are (i, j), |i| <= rx, |j| <= ry,
 * around the guess.  Per pair and point: duv [n_pairs][n][2], score [n_pairs][n], status [n_pairs][n], one of
 * GLH_DISPLACE_MATCHED, _EDGE (matched, but the peak lies on the border of the range or beside an invalid offset: no
 * sub-pixel term on that axis), _NO_OFFSET, _FLAT, _OUTSIDE (the last three: duv and score NaN); surface (or NULL)
 * [n_pairs][n][2 ry + 1][2 rx + 1], the score of every offset, NaN where it is invalid.  subpixel == 0: whole pixels,
 * never _EDGE.
 * times_ms (or NULL) [3]: HIP-event milliseconds -- [0] upload, [1] kernel, [2] download.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, sizes < 1, a pair outside [0, n_frames), a guess
 * beyond +-2^24), GLH_E_UNSUPPORTED (w or h outside 3 .. 63, rx or ry outside 1 .. 32, a frame side above 32768, more
 * than 65535 pairs).  A failed device allocation is GLH_E_NOMEM.                                                       */
#define GLH_DISPLACE_MATCHED 0
#define GLH_DISPLACE_EDGE 1
#define GLH_DISPLACE_NO_OFFSET 2
#define GLH_DISPLACE_FLAT 3
#define GLH_DISPLACE_OUTSIDE 4
int glh_stage_displacements(int device_id, const void* frames, int is_float, int width, int height, int n_frames,
                            const int32_t* pairs, int n_pairs, const int32_t* corners, const uint8_t* valid, int n,
                            const int32_t* guess, int guess_per_pair, int w, int h, int rx, int ry, int subpixel,
                            double* duv, double* score, uint8_t* status, double* surface, double* times_ms);
/* glimpse_amd.velocity_field and Observer.velocity_field: the displacements of n_pairs image pairs at the n = rows * cols
 * nodes of a regular grid (row-major), tested against their neighbours and stacked over the pairs.  The reference has no
 * such function; the rule is INPUTS.md, "Velocity field: the rule", restated in tests/velocity_field_rule.py, which the
 * device equals bit for bit.  duv [n_pairs][n][2], score [n_pairs][n] and status [n_pairs][n] are what
 * glh_stage_displacements wrote.  A vector is a candidate when its status is GLH_DISPLACE_MATCHED (or _EDGE, with
 * accept_edge != 0), its score >= min_score and both components are finite.  A candidate is kept (kept [n_pairs][n], 1 or 0)
 * when at least min_neighbors of the nodes within `radius` rows and columns of it are candidates of the same pair and, on
 * both components, |x - med| / (res + epsilon) <= threshold, med the median of the neighbours' values and res the median
 * of their absolute deviations from it (Westerweel & Scarano, 2005); radius 0: every candidate is kept, and
 * min_neighbors, threshold and epsilon are not read.  Per node and component, over the kept pairs: x = duv * scale / dt[p]
 * (scale_u, scale_v; dt [n_pairs]), v [n][2] the median of x, sigma [n][2] 1.4826 times the median of |x - v|,
 * count [n] their number; a count below min_count gives NaN in v and sigma.
 * times_ms (or NULL) [4]: HIP-event milliseconds -- [0] upload, [1] the neighbour test, [2] the stack, [3] download.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, sizes < 1, rows * cols != n, min_neighbors outside
 * 1 .. (2 radius + 1)^2 - 1, a threshold or epsilon that is not finite and positive, min_count < 1, a scale that is not
 * finite, a dt that is zero or not finite), GLH_E_UNSUPPORTED (more than 1024 pairs, a radius outside 0 .. 2, more than
 * 2^24 nodes).  A failed device allocation is GLH_E_NOMEM.                                                             */
int glh_stage_velocity_field(int device_id, const double* duv, const double* score, const uint8_t* status, int n_pairs,
                             int rows, int cols, int n, const double* dt, double scale_u, double scale_v,
                             double min_score, int accept_edge, int radius, int min_neighbors, double threshold,
                             double epsilon, int min_count, double* v, double* sigma, int32_t* count, uint8_t* kept,
                             double* times_ms);
/* helpers.maximum_filter(a, mask, fill, size, mode) (helpers.py:390-430; scipy.ndimage.maximum_filter) of a [ny][nx],
 * float64 (dtype GLH_FILTER_F64) or float32 (GLH_FILTER_F32), into out [ny][nx] of the same dtype.  The window is size_y
 * rows x size_x columns, each 1 .. 31 (a tile and its halo live in LDS), reaching size / 2 cells back and size - 1 - size / 2
 * forward as SciPy centres it; `mode` is the boundary: 0 reflect, 1 nearest, 2 mirror, 3 wrap.  mask [ny][nx] (0 = excluded)
 * or NULL: an excluded cell counts as the dtype's lowest finite value, and afterwards a's own values are put back at the
 * excluded cells (fill == 0) or at the cells whose maximum is that lowest value (fill != 0).  A NaN at an included cell is
 * the caller's to refuse (the comparison `v > m` drops it).
 * times_ms (or NULL) [5]: HIP-event milliseconds -- [0] upload, [1] maximum, [2] Gaussian along axis 0, [3] along axis 1,
 * [4] download (the same layout for the three filter stages; a stage that does not run is 0).
 * Checked before a device is touched: GLH_E_INVALID (null a / out, nx or ny < 1, nx * ny >= 2^31, a window side < 1),
 * GLH_E_UNSUPPORTED (another dtype or mode, a window side above 31).  A failed device allocation is GLH_E_NOMEM.        */
#define GLH_FILTER_F64 0
#define GLH_FILTER_F32 1
int glh_stage_max_filter(int device_id, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                         int size_y, int size_x, int mode, void* out, double* times_ms);
/* helpers.gaussian_filter(a, mask, fill, ...) (helpers.py:347-387; scipy.ndimage.gaussian_filter, order 0).  w0
 * [2 * r0 + 1]: the normalised weights along axis 0 (rows) as the host's NumPy makes them, NULL when SciPy skips the axis;
 * w1 [2 * r1 + 1] likewise along axis 1 (columns).  Radii 0 .. 4096 (the half table is kept in LDS); the tables must be
 * symmetric, as a Gaussian's are: each pass is SciPy's symmetric form  tmp = in[0] w[0]; for j = -r .. -1: tmp += (in[j] +
 * in[-j]) w[j], in float64 in that order, rounded to a's dtype after each axis, so the result equals SciPy's in every bit.
 * With a mask: G(a, 0 at excluded cells) / G(1 at included cells) in a's dtype, a's own values put back at excluded cells
 * when fill == 0; fill != 0 leaves 0 / 0 = NaN where no included cell is in reach.  `mode` and times_ms as above.
 * GLH_E_INVALID: as above, a negative radius, a weight that is not finite; GLH_E_UNSUPPORTED: another dtype or mode, a
 * radius above 4096, weights that are not symmetric.                                                                     */
int glh_stage_gaussian_filter(int device_id, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                              const double* w0, int r0, const double* w1, int r1, int mode, void* out, double* times_ms);
/* Raster.fill_crevasses (raster.py:1266-1291): the Gaussian of the maximum, both with the ORIGINAL mask and `fill`, over
 * one upload and one download; the maximum never leaves the device.  Arguments, limits and times_ms as the two above.   */
int glh_stage_fill_crevasses(int device_id, const void* a, int dtype, int nx, int ny, const uint8_t* mask, int fill,
                             int size_y, int size_x, int max_mode, const double* w0, int r0, const double* w1, int r1,
                             int gauss_mode, void* out, double* times_ms);
/* ---- terrain: Raster.gradient, Raster.hillshade, helpers.polygons_to_mask -------------------------------------------------
 * Raster.gradient (raster.py:1465-1474; np.gradient(array, d[1], d[0])) of z [ny][nx], float64 (dtype GLH_TERRAIN_F64) or
 * float32 (GLH_TERRAIN_F32), with the signed cell sizes d0 (along x, the columns) and d1 (along y, the rows), into dzdx and
 * dzdy [ny][nx] of the same dtype: along a line with spacing h, (f[i+1] - f[i-1]) / (2 h) inside and (f[1] - f[0]) / h,
 * (f[n-1] - f[n-2]) / h at the two ends.  The difference is formed in z's dtype, the quotient in float64 and rounded to z's
 * dtype, as NumPy does with a float64 spacing: float64 results equal NumPy's in every bit.  One stencil kernel.
 * times_ms (or NULL) [5]: HIP-event milliseconds -- [0] upload, [1] the kernel, [2] download, the rest 0.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, nx or ny < 2, nx * ny >= 2^31, a cell size that is zero
 * or not finite), GLH_E_UNSUPPORTED (another dtype).  A failed device allocation is GLH_E_NOMEM.                          */
#define GLH_TERRAIN_F64 0
#define GLH_TERRAIN_F32 1
int glh_stage_gradient(int device_id, const void* z, int dtype, int nx, int ny, double d0, double d1, void* dzdx, void* dzdy,
                       double* times_ms);
/* Raster.hillshade (raster.py:1249-1264; matplotlib.colors.LightSource.hillshade) into out [ny][nx] float64.  d0, d1: the
 * spacings the gradient takes along x and y (the caller hands matplotlib's: dx = d[0], dy = -d[1]); `direction` [3] the unit
 * vector towards the light as the host's NumPy makes it.  Per cell: e_dx, e_dy the gradients (as above) of vert_exag * z,
 * the product in z's dtype; the normal (-e_dx, -e_dy, 1) over sqrt((n0^2 + n1^2) + n2^2); I = n0 l0 + n1 l1 + n2 l2 summed
 * left to right.  imin, imax over all cells (NaN when any cell is NaN: then nothing is normalised); I *= fraction; if
 * imax - imin > 1e-6, I = (I - imin) / (imax - imin); I clipped to [0, 1], NaN kept.  A stencil kernel stores I and one
 * (min, max, saw-NaN) partial per workgroup, one workgroup folds the partials in a fixed order, a third kernel scales,
 * normalises and clips in place; no floating-point atomics, so two calls give the same bytes.
 * times_ms [5]: [0] upload, [1] stencil, [2] reduction, [3] normalisation, [4] download.
 * Checks as glh_stage_gradient; also GLH_E_INVALID for a vert_exag, fraction or direction that is not finite.          */
int glh_stage_hillshade(int device_id, const void* z, int dtype, int nx, int ny, double d0, double d1, double vert_exag,
                        const double* direction, double fraction, double* out, double* times_ms);
/* helpers.polygons_to_mask (helpers.py:1701-1768) by a stated rule (the reference calls GDAL, which is not pinned): out
 * [ny][nx] uint8, 1 inside.  xy [n_vertices][2]: the rings' vertices (x, y) in continuous cell coordinates, the top-left
 * corner of cell (row 0, column 0) at (0, 0); ring k is vertices ring_off[k] .. ring_off[k + 1] - 1, closed implicitly; the
 * first n_polygons rings are polygons, the n_holes after them holes.  Per ring, even-odd on the cell centres
 * (c + 0.5, r + 0.5): an edge with y1 != y2 crosses row r when min(y1, y2) <= r + 0.5 < max(y1, y2), at
 * x = x1 + (cy - y1) * (x2 - x1) / (y2 - y1) in float64 in that order, and toggles every cell of the row with c + 0.5 > x.
 * The polygons' cells of odd parity are set, one ring after another; then the holes' are cleared.  Per ring, within its
 * bounding rows and columns: a thread per (row, edge) toggles the bit of the first toggled column (atomicXor on 32-bit
 * words), a wave per row turns the bits into parities by a prefix XOR and writes the cells.
 * times_ms [5]: [0] upload and clearing, [1] the kernels of all rings, [2] download, the rest 0.
 * GLH_E_INVALID before a device is touched: null pointers, nx or ny < 1, nx * ny >= 2^31, n_vertices or n_polygons < 1,
 * n_holes < 0, offsets that do not run from 0 to n_vertices, a ring of fewer than three vertices, a vertex that is not
 * finite.  GLH_E_UNSUPPORTED: a ring whose rows x edges exceed one launch (2^39 pairs).                                   */
int glh_stage_polygon_mask(int device_id, const double* xy, int n_vertices, const int32_t* ring_off, int n_polygons,
                           int n_holes, int nx, int ny, uint8_t* out, double* times_ms);
/* ---- optimize.CLAHE: contrast-limited adaptive histogram equalisation of an 8-bit image -------------------------------
 * The rule is INPUTS.md's "CLAHE: the rule" (OpenCV's clahe.cpp for 8-bit input, written out); tests/clahe_restated.py
 * restates it in NumPy and the results equal it in every bit.  src uint8 [h][w][channels], channels 1 .. 4: the image is
 * gray = (sum of the channels) / channels in integers, which is array.mean(axis=2).astype(uint8).  The grid has
 * tiles_x x tiles_y tiles of 256 bins; clip_limit <= 0 means no clipping.  dst uint8 [h][w].  luts (or NULL) uint8
 * [tiles_y][tiles_x][256]: every tile's table, so that a test can tell a wrong table from a wrong blend.  Integer
 * histograms and one float32 expression per pixel with no contraction: the result is a function of the input alone.
 * times_ms (or NULL) [5]: HIP-event milliseconds -- [0] upload, [1] histograms (and the gray plane), [2] tables, [3] the
 * blend, [4] download.
 * GLH_E_INVALID before a device is touched: src or dst null, w or h < 1, w * h >= 2^31, channels outside 1 .. 4, tiles_x < 1
 * or > w, tiles_y < 1 or > h (the reflection that extends the image to the grid stays inside it), clip_limit not finite.
 * GLH_E_UNSUPPORTED: an extended side or a tile of 2^31 cells or more.                                                  */
int glh_stage_clahe(int device_id, const uint8_t* src, int w, int h, int channels, double clip_limit, int tiles_x,
                    int tiles_y, uint8_t* dst, uint8_t* luts, double* times_ms);
/* ---- regridding: Raster.sample(grid=True) / resample, Raster.resize, RasterInterpolant ("regrid", since
 * glh_stage_resample is particle resampling) ------------------------------------------------------------------------------
 * A raster as the source of a spline evaluation.  z [ny][nx] float64 with rows and columns in ASCENDING coordinate order
 * (the caller flips a descending axis); gx [nx], gy [ny] its strictly ascending cell centres; xmin .. ymax the box = the
 * raster's outer limits, half a cell beyond the outermost centres: the end knots sit there, not on the outermost centres
 * as in the tracker's spline kernels, so the spline extrapolates in that half cell and arguments beyond the box are
 * clamped to it (FITPACK's fpbisp).  kx, ky in 1 .. 5.  Per axis the knots are FITPACK regrid's for s = 0: k + 1 at
 * either limit, between them the centres x[(k+1)/2 .. n-(k+1)/2-1] (k odd) or the midpoints (x[i] + x[i+1]) / 2,
 * i = k/2 .. n-k/2-2 (k even).  nan_mask [ny][nx] (or NULL; kx == ky == 1 only): 1 where the cell is NaN, z holding any
 * finite value there; a sample is NaN when a coefficient of nonzero weight has a masked cell in its support (its own
 * cell, and for the first / last coefficient of a line the neighbour it is extrapolated from).  use_zmin: samples below
 * zmin become NaN (raster.py:1068).  flip_x / flip_y: output column j holds coordinate xo[mx - 1 - j] (row i: yo).      */
typedef struct glh_regrid_src {
  const double* z;
  const uint8_t* nan_mask;
  int32_t nx, ny;
  const double* gx;
  const double* gy;
  double xmin, xmax, ymin, ymax;
  int32_t kx, ky;
  int32_t use_zmin;
  int32_t flip_x, flip_y;
  int32_t reserved;
  double zmin;
} glh_regrid_src;
/* scipy.interpolate.RectBivariateSpline(gy, gx, z, bbox, kx, ky, s=0)(yo, xo, grid=True) (raster.py:1056-1067): out
 * [my][mx] float64, the interpolating tensor-product spline of `src` on the non-decreasing coordinate vectors xo [mx],
 * yo [my].  The per-axis banded collocation matrices (k diagonals on either side) are factored by LU without pivoting on
 * the host; one kernel substitutes down the columns (a thread per column), one along the rows (tiles transposed through
 * LDS), one evaluates (a thread per output cell, (ky+1)(kx+1) terms, rows outer).  Order 1 on an axis of three or more
 * cells launches no solve: the first and last coefficient of a line have a closed form.  float64 throughout, no
 * contraction, fixed summation orders: two calls give the same bytes.
 * times_ms (or NULL) [4]: HIP-event milliseconds -- [0] upload, [1] solve, [2] evaluate, [3] download.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, n <= k on an axis, k outside 1 .. 5, mx or my < 1,
 * nx * ny or mx * my >= 2^31, centres not strictly ascending or outside the box, outputs decreasing, values not finite),
 * GLH_E_UNSUPPORTED (a nan_mask with an order above 1).  A failed device allocation is GLH_E_NOMEM.                     */
int glh_stage_raster_regrid(int device_id, const glh_regrid_src* src, const double* xo, int mx, const double* yo, int my,
                            double* out, double* times_ms);
/* scipy.ndimage.zoom(a, zoom, order=1) of float64 a [ny][nx] into out [my][mx] (the caller rounds n * zoom): output index
 * i samples input coordinate c = i (n_in - 1) / (n_out - 1) (0 when n_out == 1); i0 = floor(c), t = c - i0, and
 * out = a00 (1-ty)(1-tx) + a01 (1-ty) tx + a10 ty (1-tx) + a11 ty tx summed in that order.  times_ms as above ([1] is 0).
 * GLH_E_INVALID: null pointers, a dimension < 1, nx * ny or mx * my >= 2^31.                                           */
int glh_stage_zoom_linear(int device_id, const double* a, int nx, int ny, int mx, int my, double* out, double* times_ms);
/* RasterInterpolant._interpolate (raster.py:1681-1698) over one upload and one download: z = m0 + (m1 - m0) scale and,
 * when sigma is not NULL, sigma = sqrt(s0^2 + scale2 (s0^2 + s1^2) + ((third (m1 - m0)) ratio)^2), operation by operation
 * in that order (the caller passes scale2 = scale ** 2, third = 1 / 3 and ratio = nearest_dx / dx as its own Python made
 * them).  m0, s0, z, sigma [ny][nx].  The second mean is m1 [ny][nx], or, when m1_src is not NULL, m1_src regridded at
 * order 1 onto the ascending centres xo [nx], yo [ny] of the first's grid (Raster.resample; its flip_x / flip_y say how
 * the first's array runs); likewise s1 / s1_src.  times_ms [4]: upload, regrid, blend, download.
 * Checks as glh_stage_raster_regrid; a source must have kx == ky == 1.                                                   */
int glh_stage_raster_interpolate(int device_id, int nx, int ny, const double* m0, const double* m1,
                                 const glh_regrid_src* m1_src, const double* s0, const double* s1,
                                 const glh_regrid_src* s1_src, const double* xo, const double* yo, double scale,
                                 double scale2, double third, double ratio, double* z, double* sigma, double* times_ms);
/* Camera._uv_to_xy (camera.py:1510-1519): uv [n][2] -> normalised camera coordinates xy [n][2]; the undistortion of
 * glh_stage_unproject (closed form for k1 alone, else 20 Oulu iterations), stopped before the rotation.               */
int glh_stage_uv_to_xy(int device_id, const double* cam, const double* uv, int n, double* xy);

/* ---- optimize.ObserverCameras.fit: the objective and its gradient (optimize.py:2047-2072) ----------------------------
 * A handle holds the point matches of a sequence on the device; they are uploaded once and evaluated at many view
 * directions.  n_pairs >= 0 image pairs (pair_i[p], pair_j[p]), each an index into the n_images >= 1 images; the matches
 * of pair p are rows pair_offset[p] .. pair_offset[p + 1] (int64 [n_pairs + 1], from 0, not decreasing) of xy_i and xy_j
 * [N][2]: the normalised camera coordinates of a match in image i and in image j.
 * Checked before a device is touched: GLH_E_INVALID (null pointers, n_images < 1, 2^24 images or 2^30 pairs or more,
 * offsets that do not start at 0 or decrease, an image index outside 0 .. n_images - 1, 2^31 chunks or more).           */
typedef struct glh_orient glh_orient;
int glh_orient_create(int device_id, int n_images, int n_pairs, const int32_t* pair_i, const int32_t* pair_j,
                      const int64_t* pair_offset, const double* xy_i, const double* xy_j, glh_orient** handle);
/* One evaluation at the rotation matrices R [n_images][9] (Camera.R, row-major) and their derivatives Rprime
 * [n_images][27] (Camera.Rprime, [r][w][k]), both made by the caller.  Per match of pair (i, j), with x^ = [x, y, 1]:
 * d_i = R_i^T x^_i times 1 / sqrt((a^2 + b^2) + c^2), d_j likewise, e = d_i - d_j; *objective = sum |e|;
 * g[w] = sum_r sign(e[r]) (Rprime_i[r][w] . x^_i) is added to gradient[i] and subtracted from gradient[j]
 * (gradient [n_images][3]; the reference's own formula: Rprime of image i only, no derivative of the normalisation).
 * float64, no contraction, no atomics: the order of every sum depends on the pair sizes alone, so two
 * evaluations give the same bytes.  times_ms (or NULL) [4]: HIP-event milliseconds -- [0] upload of R and Rprime, [1]
 * the map kernel, [2] the reduce kernel, [3] download.                                                               */
int glh_orient_eval(glh_orient* handle, const double* R, const double* Rprime, double* objective, double* gradient,
                    double* times_ms);
/* Frees the handle and its device memory (NULL: nothing).                                                              */
int glh_orient_destroy(glh_orient* handle);

/* ---- optimize.Cameras: the predictions of the controls under many sets of camera vectors (optimize.py:1721-1764) ------
 * A handle holds the controls of a calibration on the device; they are uploaded once and evaluated many times.  Control c
 * is of kind[c] (GLH_CALIB_*), belongs to camera cam_a[c] of the n_cams cameras (the match kinds: to cam_a[c] and
 * cam_b[c], the first and the second camera of the matches) and owns rows row_offset[c] .. row_offset[c + 1] (int64
 * [n_controls + 1], from 0, not decreasing) of obs [N][2] and src [N][3]:
 *   POINTS       obs = the observed image coordinates, src = the world coordinates (ray directions if directions[c])
 *   LINES        obs = the observed image coordinates, src unused
 *   MATCHES      obs = the first camera's image coordinates, src[.][0:2] = the second camera's
 *   ROTATION, ROTATION_XY   likewise, with normalised camera coordinates instead of image coordinates
 * Checked before a device is touched: GLH_E_INVALID (null pointers, n_cams < 1, n_controls < 0, an unknown kind, a camera
 * index outside 0 .. n_cams - 1, offsets that do not start at 0 or decrease, 2^31 rows or more).                        */
#define GLH_CALIB_POINTS 0
#define GLH_CALIB_LINES 1
#define GLH_CALIB_MATCHES 2
#define GLH_CALIB_ROTATION 3
#define GLH_CALIB_ROTATION_XY 4
typedef struct glh_calib glh_calib;
int glh_calib_create(int device_id, int n_cams, int n_controls, const int32_t* kind, const int32_t* cam_a,
                     const int32_t* cam_b, const int32_t* directions, const int64_t* row_offset, const double* obs,
                     const double* src, glh_calib** handle);
/* One evaluation of n_jobs jobs.  Job q is control job_control[q] under the camera vectors of set job_set[q] of cams
 * [n_sets][n_cams][GLH_CAM_LEN]; rot [n_sets][n_cams][9] are the cameras' rotation matrices as the caller's own host code
 * makes them (Camera.R, row-major: what Camera._xy_to_xyz and _xyz_to_xy of the ROTATION kinds multiply by).  For the
 * match kinds job_side[q] says which camera predicts: 0 the first (from the second's points), 1 the second; 0 otherwise.
 * predicted: the jobs' rows [sum of rows][2] in job order --
 *   POINTS       Camera.xyz_to_uv of the world coordinates
 *   MATCHES      Camera.uv_to_xyz of the other camera, then Camera.xyz_to_uv(directions=True)
 *   ROTATION     Camera._xy_to_xyz of the other camera ((R[0][k] x + R[1][k] y) + R[2][k], with rot), then xyz_to_uv
 *   ROTATION_XY  the same rays, then Camera._xyz_to_xy with rot: camera coordinates
 *   LINES        for every observed point the nearest (dx dx + dy dy; the first of equal ones; index 0 if none is below
 *                +inf) of the job's projected points.  Those are made from the job's segment table, segments job_seg[q] ..
 *                job_seg[q + 1] (int64 [n_jobs + 1]; other kinds have none, a LINES job at least one): segment s has the
 *                vertices seg_vertex[s] .. seg_vertex[s + 1] (int64 [n_segments + 1]) of vertex [n_vertices][3] -- camera
 *                coordinates x, y and the distance along the segment, not decreasing -- and seg_count[s] >= 1 points at
 *                the distances of np.linspace, from seg_par[s] = (start, stop, step, delta, div): i step + start (i / div
 *                times delta where step is 0; i delta for a single point), the last one stop.  A point's camera
 *                coordinates are np.interp's; Camera._distort and _xy_to_uv of the job's camera make its image
 *                coordinates.
 * float64, no contraction, no atomics: two evaluations give the same bytes.  times_ms (or NULL) [5]: HIP-event
 * milliseconds -- [0] upload, [1] the point and match rows, [2] the line points, [3] the nearest search, [4] download.
 * GLH_E_INVALID: null pointers, an index out of range, a table that does not add up, 2^31 rows, points or vertices or
 * more; GLH_E_UNSUPPORTED: a raster grid among the cameras.                                                             */
int glh_calib_eval(glh_calib* handle, int n_sets, const double* cams, const double* rot, int n_jobs,
                   const int32_t* job_control, const int32_t* job_set, const int32_t* job_side, const int64_t* job_seg,
                   const int64_t* seg_vertex, const int64_t* seg_count, const double* seg_par, int64_t n_vertices,
                   const double* vertex, double* predicted, double* times_ms);
/* optimize.ransac(batched=True): fits the parameters of ONE camera, fit_cam, to each of n_sets sets of rows in one call,
 * and can score every row of the handle under each fitted set.  cams [n_cams][GLH_CAM_LEN]: the cameras' vectors (the
 * others keep theirs).  The p parameters (1 .. 18) are the entries slots[i] of the camera vector (distinct, of 0 .. 5 and
 * 8 .. 19: not imgsz); each set starts from x0 [p] inside lb <= x0 <= ub (lb < ub), with the steps relative to x_scale [p] > 0 (as
 * scipy.optimize.least_squares' x_scale).  weights: NULL or [N][2], multiplied into the residuals predicted - observed
 * (a match control predicts in its first camera from its second camera's points, as glh_calib_eval's side 0).  observed:
 * NULL -- the handle's obs, which is what every kind but ROTATION is compared with -- or [N][2]: a ROTATION control
 * predicts image coordinates while its obs are camera coordinates, so a handle that holds one needs this.  Set q
 * holds the rows set_rows[set_offset[q] .. set_offset[q + 1]] (int64; global row numbers over all controls; no row of a
 * LINES control).
 *   The fit: one workgroup per set runs a damped Gauss-Newton (Levenberg-Marquardt) on 0.5 sum r r: the Jacobian by
 * scipy's 2-point forward differences, the rotation matrix rebuilt on the device from the stepped view direction (not
 * NumPy's bits), J^T J and J^T r summed within each wave, then across the waves, in a fixed order (no atomics: a call
 * repeated gives the same bytes), the p x p solve, the damping and the clamp into the bounds in csrc/glh_lm.h.  A row whose
 * prediction is NaN adds nothing.  At most max_nfev trial steps, 16 rejected ones in a row; it stops on scipy's tests
 * with ftol, xtol, gtol.  status [n_sets]: 1 gtol, 2 ftol, 3 xtol (scipy's numbers): converged; 0 the cap was reached,
 * -1 fewer residuals than parameters, -2 a cost that is not finite, -3 a singular system: failed.  x [n_sets][p]: the
 * values; mean_error [n_sets]: the mean of |r| over the set's own rows (NaN if the fit failed or a row has no prediction).
 *   score != 0: inlier [n_sets][N] uint8, 1 where |r| < max_error (strict; NaN is none) under the set's values, 2 for the
 * set's own rows, 0 throughout for a failed set.  The handle must hold no LINES rows then.
 * times_ms (or NULL) [4]: HIP-event milliseconds -- [0] upload, [1] fit, [2] score, [3] download.
 * GLH_E_INVALID (checked before a device is touched; the handle stays usable): null pointers, fit_cam or a row out of
 * range, p outside 1 .. 18, slots that repeat or are no parameter, x0 outside its bounds, lb >= ub, a scale that is not positive,
 * offsets that do not start at 0 or decrease, 2^31 set rows or scored (set, row) pairs or more, a LINES row, max_nfev < 1,
 * tolerances outside [0, 1); GLH_E_UNSUPPORTED: a raster grid among the cameras.                                       */
int glh_calib_fit_sets(glh_calib* handle, const double* cams, int fit_cam, int p, const int32_t* slots, const double* x0,
                       const double* lb, const double* ub, const double* x_scale, const double* weights,
                       const double* observed, int n_sets, const int64_t* set_offset, const int64_t* set_rows, int max_nfev, double ftol, double xtol,
                       double gtol, int score, double max_error, double* x, int32_t* status, double* mean_error,
                       uint8_t* inlier, double* times_ms);
/* optimize.ransac_pairs: Random Sample Consensus over n_groups GROUPS in one pass on the device.  Group g is the match
 * control group_control[g] of the handle (MATCHES, ROTATION or ROTATION_XY; the groups name distinct controls in ascending
 * order, and every row of the handle belongs to one of them) with the camera group_cam[g], one of the control's two, fitted
 * in the entries slots [p] of its vector (as glh_calib_fit_sets) from x0 inside lb .. ub with the scales x_scale, each
 * [n_groups][p]; the control's other camera, and this camera where another group holds it, stay at cams
 * [n_cams][GLH_CAM_LEN].  weights, observed: as glh_calib_fit_sets.  The group owns hypotheses hyp_offset[g] ..
 * hyp_offset[g + 1] (int64 [n_groups + 1], from 0, not decreasing): hypothesis h samples the n rows samples[h][0 .. n)
 * (int64, global row numbers, inside the group's control).
 *   1. every hypothesis is fitted to its sample by glh_calib_fit_sets' damped Gauss-Newton (a sample of up to 64 rows by
 *      one wave, several to a workgroup; the LDS sized for p <= 3 or p <= 18): x [H][p], status [H] (its codes);
 *   2. every row of the hypothesis's own group is scored under x: consensus [H] int32 counts the rows outside the sample
 *      with |r| < max_error (0 for a failed fit); the masks stay on the device, hypotheses times rows bytes per group;
 *   3. a hypothesis with status > 0 and consensus > min_inliers is refitted on sample and consensus, the group's rows in
 *      ascending order: refit_x [H][p], refit_status [H], mean_error [H] (the mean of |r| over that set; NaN if the refit
 *      failed or a row has no prediction).  The others get NaN and refit_status -100;
 *   4. winner [n_groups]: the group's hypothesis (counted from the group's first) with refit_status > 0 and the smallest
 *      mean_error that is a number, the earlier of equal ones; -1 if there is none;
 *   5. inlier [N] uint8: 1 where |r| <= max_error under the winner's refit_x, 0 elsewhere and in a group without a winner.
 * float64, no contraction, no floating-point atomics: a call repeated gives the same bytes, and a group's results do not
 * depend on the other groups of the call.  times_ms (or NULL) [6]: HIP-event milliseconds -- [0] upload, [1] fit,
 * [2] score, [3] refit, [4] winner and final score, [5] download.
 * GLH_E_INVALID (checked before a device is touched, by csrc/glh_ransac_plan.h; the handle stays usable): null pointers, a
 * group's control or camera out of range, a camera that is neither of its control's, a POINTS or LINES control, controls
 * that repeat or descend, rows of the handle outside every group, a sample row outside its group's control, p, slots,
 * bounds, scales and tolerances as glh_calib_fit_sets, n < 1, offsets that do not start at 0 or decrease, 2^31 mask bytes
 * or sample rows or more, a ROTATION control without observed; GLH_E_UNSUPPORTED: a raster grid among the cameras.    */
int glh_calib_ransac_groups(glh_calib* handle, const double* cams, int n_groups, const int32_t* group_control,
                            const int32_t* group_cam, int p, const int32_t* slots, const double* x0, const double* lb,
                            const double* ub, const double* x_scale, const double* weights, const double* observed,
                            const int64_t* hyp_offset, int n, const int64_t* samples, int max_nfev, double ftol, double xtol,
                            double gtol, double max_error, int64_t min_inliers, double* x, int32_t* status, int32_t* consensus,
                            double* refit_x, int32_t* refit_status, double* mean_error, int32_t* winner, uint8_t* inlier,
                            double* times_ms);
/* optimize.ransac_pairs(samples="device"): glh_calib_ransac_groups with the samples of some groups drawn on the device
 * (INPUTS.md, "Device samples: the rule"; csrc/glh_ransac_draw.h).  group_id [n_groups] int32 >= 0: the pair the group is
 * in the caller's whole list, which with the hypothesis's number within the group, the group's row count, n and the seed
 * words seed0, seed1 decides a drawn sample -- not the group's place in this call.  drawn [n_groups] uint8: 1, the
 * group's hypotheses are drawn by Floyd's algorithm from Philox4x32 streams (the round count of the tracker's) and its
 * entries of samples are not read -- it must have more than n rows; 0, they are read from samples as
 * glh_calib_ransac_groups reads them (samples may be NULL if no group with a hypothesis has 0).  samples_out (or NULL)
 * int64 [H][n]: the rows every hypothesis sampled, global row numbers, ascending within a drawn one.  Everything else, and
 * every result, as glh_calib_ransac_groups for those samples.  times_ms (or NULL) [7]: its six -- [1] from the end of the
 * draw -- and [6] the draw.
 * GLH_E_INVALID, before a device is touched: as glh_calib_ransac_groups, and null group_id or drawn, a negative id, a flag
 * above 1, a drawn group with hypotheses and n rows or fewer.                                                           */
int glh_calib_ransac_groups_drawn(glh_calib* handle, const double* cams, int n_groups, const int32_t* group_control,
                                  const int32_t* group_cam, int p, const int32_t* slots, const double* x0, const double* lb,
                                  const double* ub, const double* x_scale, const double* weights, const double* observed,
                                  const int64_t* hyp_offset, int n, const int64_t* samples, int max_nfev, double ftol,
                                  double xtol, double gtol, double max_error, int64_t min_inliers, double* x, int32_t* status,
                                  int32_t* consensus, double* refit_x, int32_t* refit_status, double* mean_error,
                                  int32_t* winner, uint8_t* inlier, const int32_t* group_id, const uint8_t* drawn,
                                  uint32_t seed0, uint32_t seed1, int64_t* samples_out, double* times_ms);
/* hyps [n_groups]: min(iterations, C(rows[g], n)) hypotheses for a group of rows[g] rows, the binomial coefficient exact;
 * 0 for a group of n rows or fewer.  enumerated [n_groups] uint8: 1 where C(rows[g], n) <= iterations, a group whose
 * hypotheses are all combinations (glh_ransac_combinations) and not drawn.  Host arithmetic; GLH_E_INVALID: null pointers,
 * n < 1, rows or iterations outside 0 .. 2^31 - 1.                                                                       */
int glh_ransac_hypotheses(int n_groups, const int64_t* rows, int n, int64_t iterations, int64_t* hyps, uint8_t* enumerated);
/* samples [count][n] int64: the first count combinations of n of the rows 0 .. rows - 1 in lexicographic order.  Host
 * arithmetic; GLH_E_INVALID: n < 1, rows < n or above 2^31 - 1, count negative or above C(rows, n), null output.       */
int glh_ransac_combinations(int64_t rows, int n, int64_t count, int64_t* samples);
/* The draw alone: samples int64 [H][n], for hypothesis h of group g (hyp_offset [n_groups + 1] from 0, not decreasing) the
 * rows 0 .. rows[g] - 1 that glh_calib_ransac_groups_drawn draws for a group of that id, row count and seed, counted
 * within the group.  times_ms (or NULL) [3]: upload, draw, download.  GLH_E_INVALID, before a device is touched: null
 * pointers, 2^24 groups or more, n < 1, a group of n rows or fewer or of more than 2^31 - 1, a negative id, offsets that
 * do not start at 0 or decrease, 2^31 sampled rows or more in all.                                                       */
int glh_stage_ransac_samples(int device_id, int n_groups, const int64_t* rows, const int32_t* group_id,
                             const int64_t* hyp_offset, int n, uint32_t seed0, uint32_t seed1, int64_t* samples,
                             double* times_ms);
/* chunk_of [n_groups]: the call of glh_calib_ransac_groups that each group of a longer list goes to, when consecutive
 * groups share a call while its masks (rows[g] times hyps[g] bytes each) stay at or below budget bytes and a group whose
 * own masks exceed it gets a call of its own; n_chunks: how many calls.  Host arithmetic; GLH_E_INVALID: null pointers, a
 * negative count.                                                                                                       */
int glh_ransac_chunks(int n_groups, const int64_t* rows, const int64_t* hyps, int64_t budget, int32_t* chunk_of,
                      int32_t* n_chunks);
/* Frees the handle and its device memory (NULL: nothing).                                                              */
int glh_calib_destroy(glh_calib* handle);

/* ---- optimize.match_keypoints: the exact two nearest neighbours among descriptor sets (optimize.py:2234-2309) ----------
 * A handle keeps descriptor sets on the device, each under a slot number >= 0 of the caller's choosing; a set is uploaded
 * once and searched many times.  For every row q of set Q, glh_match_knn2 gives the two rows of set T with the smallest
 * keys (d2, row index) in lexicographic order: equal distances go to the lower index.  The order is total, so the result
 * is a function of the two sets alone.
 *   GLH_MATCH_U8   data uint8 [n][dim], dim <= 256.  d2 = |q|^2 + |t|^2 - 2 q.t on x - 128 in int32 (the int8 matrix
 *                  instructions), exact; returned as the float32 of that integer (below 2^24).
 *   GLH_MATCH_F32  data float32 [n][dim].  d2 accumulated in float32 in element order k = 0 .. dim - 1 as
 *                  s = s + (q_k - t_k) * (q_k - t_k), every operation rounded, no FMA.  A NaN distance is never taken.  */
#define GLH_MATCH_U8 0
#define GLH_MATCH_F32 1
typedef struct glh_match glh_match;
int glh_match_create(int device_id, glh_match** handle);
/* Uploads and prepares n >= 1 rows of dim >= 1 elements under `slot`, in the place of what the slot held.
 * GLH_E_INVALID: a null pointer, slot < 0, an unknown kind, n == 0 or n > 2^30, dim < 1, dim > 256 (U8) or 2^16 (F32),
 * more than 2^35 elements (n times dim rounded up to a multiple of 32).                                                 */
int glh_match_put(glh_match* handle, int slot, int kind, int n, int dim, const void* data);
/* Frees the set of `slot`.  GLH_E_INVALID: nothing is in that slot.                                                     */
int glh_match_drop(glh_match* handle, int slot);
/* idx int32 [n_q][2], d2 float32 [n_q][2]: the nearest and the second nearest row of slot_t's set for every row of
 * slot_q's (the same slot may be both).  A set of one row has no second: (-1, +inf).  times_ms (or NULL) [5]: HIP-event
 * milliseconds -- [0] upload and [1] preparation of the two sets, as measured when they were put, [2] the search kernel,
 * [3] the merge of T's ranges (0 when T is one range), [4] download.
 * GLH_E_INVALID: a null pointer, an unknown slot, sets of different dim or of different kinds.                          */
int glh_match_knn2(glh_match* handle, int slot_q, int slot_t, int32_t* idx, float* d2, double* times_ms);
/* Frees the handle, its sets and its device memory (NULL: nothing).                                                    */
int glh_match_destroy(glh_match* handle);

/* ---- optimize.SIFT: keypoint detection and description (Lowe 2004 with OpenCV's structure and constants) ---------------
 * The rule is INPUTS.md's "SIFT: the rule"; tests/sift_restated.py restates it in NumPy and the results equal it in every
 * bit.  A handle keeps the pyramid's buffers between images: a sequence of frames of one size allocates once.
 * params (float64): [0] nOctaveLayers S (1 .. 8), [1] contrastThreshold (0 .. 10^6), [2] edgeThreshold (> 0, <= 10^6),
 * [3] sigma (0 < sigma <= 16), [4 .. 4 + S + 3) the radii r_i (0 .. 4096) of the S + 3 weight tables -- [0] the blur of the
 * doubled image, [i] the step from Gaussian layer i - 1 to layer i -- and after them the tables themselves, 2 r_i + 1
 * weights each (symmetric; made by the caller: NumPy's exp).
 * glh_sift_detect: image uint8 [h][w].  *n: the keypoints found, in the rule's order, before the caller's steps (equal
 * neighbours, mask, nfeatures).  times_ms (or NULL) [7]: HIP-event milliseconds -- [0] upload, [1] base, [2] pyramid,
 * [3] extrema, [4] refinement and orientation, [5] descriptors, [6] download.  An image too small for an octave gives
 * *n = 0.  GLH_E_INVALID: a null pointer, w or h < 1 or above 2^23, a doubled image of 2^31 cells or more, parameters
 * outside the ranges above; GLH_E_NOMEM: an allocation failed (the message has the bytes asked for).                     */
typedef struct glh_sift glh_sift;
int glh_sift_create(int device_id, glh_sift** handle);
int glh_sift_detect(glh_sift* handle, const uint8_t* image, int w, int h, const double* params, int* n, double* times_ms);
/* keypoints float64 [n][6] (pt x, pt y, size, angle, response, octave as OpenCV packs it), descriptors uint8 [n][128] of
 * the last detection.  GLH_E_INVALID: a null pointer, nothing detected yet.                                              */
int glh_sift_read(glh_sift* handle, double* keypoints, uint8_t* descriptors);
/* counts int32 [6] of the last detection: octaves, candidates, keypoints, S, doubled width, doubled height (octave o has
 * (side + 2^o - 1) >> o cells a side).                                                                                   */
int glh_sift_counts(glh_sift* handle, int32_t* counts);
/* One stage of the last detection, for tests that tell where a difference starts:
 *   GLH_SIFT_GAUSS       float32 [H][W]: Gaussian layer `index` (0 .. S + 2) of `octave`
 *   GLH_SIFT_DOG         float32 [H][W]: difference `index` (0 .. S + 1) of `octave`
 *   GLH_SIFT_CANDIDATES  int32 [candidates][4]: octave, layer, row, column, ascending
 *   GLH_SIFT_REFINED     float64 [candidates][12]: status (0 kept, 1 zero pivot, 2 left the border or the layers, 3 not
 *                        settled, 4 contrast, 5 edge, 6 a step above 10^6), then of a kept one: octave, layer, row, column
 *                        of the settled cell, xc, xr, xi, contrast, size, pt x, pt y (zeros otherwise)
 *   GLH_SIFT_CELLS       int32 [keypoints][5]: octave, layer, row, column, orientation bin of every keypoint
 * GLH_E_INVALID: a null pointer, nothing detected yet, an unknown kind, a layer the pyramid does not have.               */
#define GLH_SIFT_GAUSS 0
#define GLH_SIFT_DOG 1
#define GLH_SIFT_CANDIDATES 2
#define GLH_SIFT_REFINED 3
#define GLH_SIFT_CELLS 4
int glh_sift_layer(glh_sift* handle, int kind, int octave, int index, void* out);
/* Frees the handle and its device memory (NULL: nothing).                                                              */
int glh_sift_destroy(glh_sift* handle);

/* Tracker.resample_particles("systematic") on one population: idx int64 [n].                 */
int glh_stage_resample(int device_id, const double* weights, int n, double u, int64_t* idx);

#ifdef __cplusplus
}
#endif
#endif /* GLIMPSE_HIP_H */
