/*
 * dmf.h — C ABI of the MI355X-native voxel ray-tracing / depth-fusion engine.
 *
 * The reference (REXJJ/depth-map-fusion-utils) has no FFI layer: its boundary is the
 * header-only C++ class API of include/Camera.hpp, include/Volume.hpp and
 * include/RayTracingEngine.hpp.  Every entry point below names the
 * reference member it replaces (file:line in the reference tree).  The C++ drop-in
 * classes in depth-map-fusion-utils_amd/compat/ and the Python mirror in dmf_amd/
 * are thin layers over this ABI; see INTEGRATION.md for the bindings.
 *
 * Conventions
 *  - All calls return an int status (DMF_OK == 0); nothing throws across the ABI.
 *    dmf_last_error() returns a thread-local message for the last failure.
 *  - A dmf_volume is one device-resident VoxelVolume plus its HIP stream; use one
 *    handle per host thread (the reference hot path is single-threaded).
 *  - Poses are float[12], row-major 3x4 [R|t] (rows 0..2 of Eigen::Affine3f), camera
 *    -> world, exactly the `transformation` argument of the reference.
 *  - Voxel ids are the reference hash (x<<40) ^ (y<<20) ^ z (Volume.hpp:143-148).
 *    "slot" = position of a voxel in occupied_cells_ (first-touch order).
 *  - Functions without a _device suffix take HOST pointers and synchronise the
 *    stream before returning; *_device functions take DEVICE pointers, only enqueue
 *    work on the volume's stream and never synchronise.
 *  - The engine needs a gfx950 GPU.  There is no CPU fallback: with no usable
 *    device every compute call fails with DMF_ERR_NO_DEVICE.
 */
#ifndef DMF_H_
#define DMF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMF_ABI_VERSION 1

enum dmf_status {
  DMF_OK = 0,
  DMF_ERR_INVALID = 1,   /* bad argument (null pointer, bad size, bad pose count ...) */
  DMF_ERR_STATE = 2,     /* volume not constructed / wrong call order              */
  DMF_ERR_HIP = 3,       /* HIP runtime error (message in dmf_last_error)          */
  DMF_ERR_NOMEM = 4,     /* device or host allocation failed                       */
  DMF_ERR_CAPACITY = 5,  /* output buffer too small: required size returned        */
  DMF_ERR_RANGE = 6,     /* grid too large for a packed field (hash / fixed point) */
  DMF_ERR_NO_DEVICE = 7, /* no usable GPU                                          */
  DMF_ERR_DEVICE_CHECK = 8 /* a device-side consistency check failed: the results of the
                              calls it covers are invalid (dmf_fuse_status)               */
};

typedef struct dmf_volume dmf_volume;

/* Camera(vector<float>& K, int height=480, int width=640)  Camera.hpp:23
 * K row-major 3x3: fx=K[0], cx=K[2], fy=K[4], cy=K[5]  (Camera.hpp:26). */
typedef struct dmf_camera {
  float K[9];
  int32_t height;
  int32_t width;
} dmf_camera;

/* VoxelVolume public fields (Volume.hpp:54-60) + engine bookkeeping. */
typedef struct dmf_volume_info {
  double xmin, xmax, ymin, ymax, zmin, zmax;
  double xcenter, ycenter, zcenter;
  double xdelta, ydelta, zdelta;
  double voxel_size;
  int32_t xdim, ydim, zdim;
  int32_t constructed;
  uint64_t hsize;
  int64_t num_occupied;  /* occupied_cells_.size() */
  int64_t num_points;    /* points binned so far   */
  int64_t hazards;       /* unguarded out-of-range accesses the reference would make */
} dmf_volume_info;

/* 3D-DDA log-odds fusion parameters (not in the reference).
 * Depth gate: any int32 pair.  A pixel of depth d (uint16, 0..65535) is traced iff
 * dmin_mm <= d < dmax_mm, so an empty or inverted gate (dmin_mm >= dmax_mm) traces nothing,
 * dmin_mm <= 0 admits d = 0 (a ray that ends at the camera centre: one update in the camera's
 * cell when that lies in the grid) and dmax_mm > 65535 admits d = 65535.
 * Clamp: -32768 <= l_min <= l_max <= 32767 (the log-odds are int16).  The finalize entry
 * points (dmf_fuse_finalize, dmf_fuse_finalize_device, dmf_fuse_finalize_slab_device,
 * dmf_fuse_merge_finalize_device) return DMF_ERR_INVALID for any other clamp and touch
 * neither the output nor the counters.  l_hit and l_miss are any int32 (the sum is formed
 * in 64 bits). */
typedef struct dmf_fuse_params {
  int32_t dmin_mm;  /* depth accepted iff dmin_mm <= d < dmax_mm */
  int32_t dmax_mm;
  int32_t l_hit;    /* milli-logit per hit   (OctoMap default p=0.7  ->  847) */
  int32_t l_miss;   /* milli-logit per miss  (OctoMap default p=0.4  -> -405) */
  int32_t l_min;    /* clamp                 (p=0.1192 -> -2000)              */
  int32_t l_max;    /*                       (p=0.971  ->  3511)              */
} dmf_fuse_params;

/* ---- library ------------------------------------------------------------ */
int dmf_abi_version(void);
const char* dmf_status_string(int status);
const char* dmf_last_error(void);
int dmf_device_count(int32_t* count);
void dmf_fuse_params_default(dmf_fuse_params* p);
/* The normal test degree(acos(n.v)) in [0,90] (CommonUtilities.hpp:17,
 * RayTracingEngine.hpp:207-219) is evaluated on the GPU as dstar <= n.v <= 1, with
 * dstar the smallest float whose host-libm acosf passes (the function the reference
 * binary calls).  Host-only; no GPU needed. */
int dmf_angle_threshold(float* dstar);
/* The fusion implementation, its kernel name and the tuning / test knobs of a volume are
 * diagnostics, declared in include/dmf_diag.h (results never depend on them). */

/* ---- VoxelVolume  (Volume.hpp:50-255) ------------------------------------ */
/* VoxelVolume::VoxelVolume()  Volume.hpp:63 — device = HIP device ordinal. */
int dmf_volume_create(dmf_volume** out, int32_t device);
/* VoxelVolume::~VoxelVolume()  Volume.hpp:80-87 */
int dmf_volume_destroy(dmf_volume* v);
/* All work of this handle is enqueued on `stream` (hipStream_t; NULL = default).  The
 * switch does not block the host: the new stream waits for the work already enqueued on
 * the old one (skipped when either stream is capturing a graph). */
int dmf_volume_set_stream(dmf_volume* v, void* hip_stream);
int dmf_volume_synchronize(dmf_volume* v);
/* setDimensions  Volume.hpp:89-100 */
int dmf_volume_set_dimensions(dmf_volume* v, double xmin, double xmax, double ymin, double ymax,
                              double zmin, double zmax);
/* setResolution  Volume.hpp:102-107 */
int dmf_volume_set_resolution(dmf_volume* v, double xdelta, double ydelta, double zdelta);
/* setVolumeSize  Volume.hpp:109-117 */
int dmf_volume_set_volume_size(dmf_volume* v, int32_t xdim, int32_t ydim, int32_t zdim);
/* constructVolume  Volume.hpp:119-128 (dims recomputed by truncation, as the reference) */
int dmf_volume_construct(dmf_volume* v);
int dmf_volume_get_info(const dmf_volume* v, dmf_volume_info* out);

/* integratePointCloud(cloud [, normals])  Volume.hpp:172-197 / :199-228.
 * xyz: n*3 floats (PointXYZRGB x,y,z); normals: n*3 floats or NULL.  Points
 * outside the grid are skipped (the no-normals reference overload indexes out of
 * range there — counted in *n_hazard). */
int dmf_volume_integrate(dmf_volume* v, const float* xyz, const float* normals, int64_t n,
                         int64_t* n_binned, int64_t* n_hazard);
int dmf_volume_integrate_device(dmf_volume* v, const float* d_xyz, const float* d_normals, int64_t n);

/* occupied_cells_ (Volume.hpp:54) in insertion order. */
int dmf_volume_occupied(const dmf_volume* v, uint64_t* hashes, int64_t cap, int64_t* n);
/* Voxel::view / Voxel::good (Volume.hpp:29-48) per slot. */
int dmf_volume_voxel_flags(const dmf_volume* v, int32_t* view, uint8_t* good, int64_t cap);
int dmf_volume_reset_flags(dmf_volume* v);
/* Voxel::pts.size() / normals.size() per slot. */
int dmf_volume_voxel_counts(const dmf_volume* v, int64_t* npts, int64_t* nnormals, int64_t cap);
/* Voxel::pts / Voxel::normals of one voxel (insertion order); *n = #points, -1 if empty. */
int dmf_volume_voxel_points(const dmf_volume* v, uint64_t hash, float* pts, float* normals, int64_t cap,
                            int64_t* n);
/* Bulk export of every voxel's points/normals (host mirror of voxels_[x][y][z]->pts /
 * ->normals): offsets[V+1] (points of slot s are [offsets[s], offsets[s+1])), pts
 * 3 floats per point, normals4 4 floats per point (w = 1 if the point carried a
 * normal), in occupied_cells_ order and insertion order within a voxel.  cap_points
 * must be >= num_points (dmf_volume_get_info); any output may be NULL. */
int dmf_volume_export(const dmf_volume* v, int32_t* offsets, float* pts, float* normals4, int64_t cap_points);
/* voxels_[x][y][z] != nullptr as a dense x-major byte grid (xdim*ydim*zdim). */
int dmf_volume_occupancy(const dmf_volume* v, uint8_t* dense);

/* ---- Camera back-projection  (Camera.hpp:24-31 projectPoint + :39-45 transformPoints) */
/* depth: H*W uint16 mm, pose: 12 floats -> xyz: H*W*3 floats (world). */
int dmf_backproject(dmf_volume* v, const dmf_camera* cam, const uint16_t* depth, const float* pose,
                    float* xyz);
int dmf_backproject_device(dmf_volume* v, const dmf_camera* cam, const uint16_t* d_depth,
                           const float* d_poses, int32_t P, float* d_xyz);

/* ---- RayTracingEngine  (RayTracingEngine.hpp:27-564) ---------------------- */
/* reverseRayTraceFast  RayTracingEngine.hpp:136-226, batched over P poses.
 * found[P]; counts[P]; hashes = the P good lists concatenated in pose order, each in
 * occupied_cells_ order.  DMF_ERR_CAPACITY (counts filled) if sum(counts) > cap. */
int dmf_reverse_ray_trace_fast(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P,
                               int32_t viz, uint8_t* found, int64_t* counts, uint64_t* hashes,
                               int64_t cap);
/* Device form: per-pose bitmasks over slots, words = ceil(num_occupied/64) per pose,
 * d_visible / d_good: P*words uint64 (either may be NULL).  d_poses: P*12 floats. */
int dmf_reverse_visibility_device(dmf_volume* v, const dmf_camera* cam, const float* d_poses, int32_t P,
                                  int32_t viz, uint64_t* d_visible, uint64_t* d_good,
                                          uint64_t* d_stats /* 2 counters += {march samples, voxel rays}; may be NULL */);
/* reverseRayTrace  RayTracingEngine.hpp:45-134 (float-accumulated grid enumeration). */
int dmf_reverse_ray_trace(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t viz,
                          uint8_t* found, int64_t* counts, uint64_t* hashes, int64_t cap);
/* Set-cover consumer: Algorithms.hpp:38-86 greedySetCover over the reverseRayTraceFast
 * good sets of P candidate poses (the loop of tests/SetCover.cpp:218-240).  selected[P]
 * receives the chosen pose indices in selection order; the reference stops when no set
 * adds anything or the best adds fewer than min_gain (5) voxels.  min_gain is signed:
 * min_gain <= 0 means "until nothing is added". */
int dmf_greedy_set_cover(dmf_volume* v, const dmf_camera* cam, const float* poses, int32_t P, int32_t min_gain,
                         int32_t* selected, int32_t* nselected);
/* Same over caller bitmasks (P x words uint64, e.g. d_good of dmf_reverse_visibility_device). */
int dmf_greedy_set_cover_masks_device(dmf_volume* v, const uint64_t* d_masks, int32_t P, int64_t words,
                                      int32_t min_gain, int32_t* selected, int32_t* nselected);
/* rayTrace  RayTracingEngine.hpp:268-309 */
int dmf_ray_trace(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta, int32_t sparse);
/* rayTraceAndClassify  RayTracingEngine.hpp:311-375 */
int dmf_ray_trace_and_classify(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                               int32_t view, int32_t sparse);
/* rayTraceAndGetMinimum  RayTracingEngine.hpp:229-264 (-1 if nothing hit) */
int dmf_ray_trace_and_get_minimum(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                                  int32_t sparse, int32_t* minimum);
/* rayTraceAndGetPoints  RayTracingEngine.hpp:447-494 */
int dmf_ray_trace_and_get_points(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zdelta,
                                 int32_t sparse, uint8_t* found, uint64_t* hashes, int64_t cap, int64_t* n);
/* rayTraceAndGetGoodPoints  RayTracingEngine.hpp:377-445 */
int dmf_ray_trace_and_get_good_points(dmf_volume* v, const dmf_camera* cam, const float* pose,
                                      int32_t zdelta, int32_t sparse, uint8_t* found, uint64_t* hashes,
                                      int64_t cap, int64_t* n);
/* Per-pixel first hit of the forward march on the (rdelta, cdelta) lattice:
 * k_out[R*C] depth-plane index (-1 = none), hash_out[R*C]. */
int dmf_forward_first_hits(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t zstart,
                           int32_t zdelta, int32_t rdelta, int32_t cdelta, int32_t* k_out,
                           uint64_t* hash_out);
/* Batched device form for P poses: d_k / d_slot P*R*C int32 (first-hit depth-plane index
 * and occupied slot, -1 = none); d_stats (may be NULL) += {march samples}. */
int dmf_forward_first_hits_device(dmf_volume* v, const dmf_camera* cam, const float* d_poses, int32_t P,
                                  int32_t zstart, int32_t zdelta, int32_t rdelta, int32_t cdelta, int32_t* d_k,
                                  int32_t* d_slot, uint64_t* d_stats);
/* rayTraceVolume  RayTracingEngine.hpp:498-564 (depth_out: H*W int32 z-buffer or NULL). */
int dmf_ray_trace_volume(dmf_volume* v, const dmf_camera* cam, const float* pose, int32_t* depth_out);
/* willCollide  tests/CameraPathGen.cpp:128-156, for n segment pairs a[i] -> b[i]. */
int dmf_will_collide(dmf_volume* v, const float* a, const float* b, int64_t n, uint8_t* collided);
/* Planner::run_tsp cost map  tests/CameraPathGen.cpp:310-331 (also CameraMotionTSP.cpp:
 * 291-306): for all V*V ordered pairs of camera centres (translation of poses[i], P*12
 * floats) map[i*V+j] = INT_MAX if willCollide(c_i, c_j) else int(|c_i - c_j| * 1000).
 * V <= 46340.  Device form: a pair the reference cannot march (non-finite centre, or a
 * segment over INT_MAX mm) gets -1; the host form rejects non-finite centres. */
int dmf_collision_cost_map(dmf_volume* v, const float* poses, int32_t V, int32_t* map);
int dmf_collision_cost_map_device(dmf_volume* v, const float* d_poses, int32_t V, int32_t* d_map);

/* ---- 3D-DDA log-odds fusion (new capability) ------------------ */
/* Host form: depth P*H*W uint16 mm, poses P*12; hits/misses: xdim*ydim*zdim int32 in
 * the reference's x-major voxel order, ACCUMULATED (caller zeroes).
 * stats[3] += {cell updates, rays, hits}. */
int dmf_fuse_depth(dmf_volume* v, const dmf_camera* cam, const uint16_t* depth, const float* poses,
                   int32_t P, const dmf_fuse_params* prm, int32_t* hits, int32_t* misses, int64_t* stats);
/* Device form.  d_hits / d_misses are fusion counters in the TILED layout (2x2x4-cell
 * tiles of 16 int32 = one 64-B line, tiles x-major) of
 * dmf_fuse_counter_cells() elements each, ACCUMULATED; any elementwise sum of them
 * (e.g. an all-reduce across ranks) stays valid.  d_stats (may be NULL): 8 uint64
 * counters += {cell updates, rays, hits, layout faults, LDS rounds | pairs, direct rounds |
 * parts, flushed cell atomics, 0}; layout faults (must stay 0) = the device-side check of
 * the brick pipeline's pair layout (dmf_fuse_status) -- a non-zero count means the counters
 * of that call are invalid. */
int dmf_fuse_depth_device(dmf_volume* v, const dmf_camera* cam, const uint16_t* d_depth,
                          const float* d_poses, int32_t P, const dmf_fuse_params* prm, int32_t* d_hits,
                          int32_t* d_misses, uint64_t* d_stats);
/* Pre-allocate the fusion scratch for calls of up to P frames of `cam`'s size on this
 * volume, so that dmf_fuse_depth_device then neither allocates nor synchronises (e.g. for
 * hipGraph capture).  The brick pipeline fits its ray records, brick tables and (ray,
 * brick) pair records into max_scratch_bytes (0 = keep the current budget; default 45 % of
 * the device's memory, ~130 GB on MI355X): serial calls use one slot of the whole budget,
 * pipelined calls (dmf_fuse_set_input_stream) two staging slots of half each.  A call whose
 * pairs exceed a slot's pair capacity is cut into pose batches on the device
 * (dmf_fuse_plan).  A new budget frees and re-plans the slots.  Synchronises the stream.
 * The budget is PER VOLUME: several volumes fusing on one device (or several processes
 * sharing it) should each reserve their share explicitly, e.g. 0.9 x free memory / volumes;
 * a call whose pairs exceed the share runs in more pose batches (dmf_fuse_batches_used),
 * with identical results. */
int dmf_fuse_reserve(dmf_volume* v, const dmf_camera* cam, int32_t P, uint64_t max_scratch_bytes);
/* Point-cloud fusion: the insertPointCloud(scan, origin) of the same exact
 * log-odds fusion.  S scans of N points each: xyz[S][N][3] packed float32 world-frame ray
 * endpoints, origins[S][3] float32 world-frame sensor positions.  Point i of scan s is the ray
 * origins[s] -> xyz[s][i], from there on exactly the ray of dmf_fuse_depth (endpoint
 * acceptance, clip, 1/256-cell quantisation, integer DDA with ties x < y < z; a miss on every
 * cell before the end cell, a hit on the end cell or a miss there when the endpoint lies
 * outside the grid), so the points dmf_backproject gives for a frame, fused from the pose's
 * translation, make the counters of dmf_fuse_depth on that frame bit for bit.
 *  - A point with a non-finite coordinate is NO ray: no update, not counted in stats[1].  This
 *    is how organised clouds mark invalid returns, and how scans of unequal length are padded
 *    to a common N (pad with NaN).  A scan whose origin has a non-finite coordinate traces
 *    nothing.
 *  - There is NO range gate: dmin_mm / dmax_mm are not applied (a point has no depth value).
 *    The caller filters by range, or marks rejected points NaN.  l_hit .. l_max are used only
 *    by the finalize calls, as for depth frames.
 *  - The order of the points never changes a counter; it decides which 64 rays share a wave
 *    (ray index = s * ceil(N/64) * 64 + i), so spatially coherent order is faster.
 * Host form: linear x-major counters ACCUMULATED, runs the layout check itself, stats[3] +=
 * {cell updates, rays, hits}.  Device form: tiled counters, only enqueues, d_stats[8] as
 * dmf_fuse_depth_device.  Both honour the volume's fusion variant, knobs, phase event and input
 * stream as the depth calls do, and may be mixed with them on one volume without synchronising.
 * Status (checked before the volume is touched): null volume / params / buffer, N < 1 or S
 * outside 1..65535 -> DMF_ERR_INVALID; unconstructed volume -> DMF_ERR_STATE; a grid over 2048
 * cells per axis -> DMF_ERR_RANGE; one scan over the brick pipeline's 32-bit pair offsets or
 * over its budget -> DMF_ERR_RANGE (the depth calls' "one frame exceeds ..." messages): split
 * such a scan into several scans with the same origin. */
int dmf_fuse_points(dmf_volume* v, const float* xyz, const float* origins, int32_t S, int64_t N,
                    const dmf_fuse_params* prm, int32_t* hits, int32_t* misses, int64_t* stats);
int dmf_fuse_points_device(dmf_volume* v, const float* d_xyz, const float* d_origins, int32_t S, int64_t N,
                           const dmf_fuse_params* prm, int32_t* d_hits, int32_t* d_misses, uint64_t* d_stats);
/* dmf_fuse_reserve for point calls of up to S scans of N points. */
int dmf_fuse_points_reserve(dmf_volume* v, int32_t S, int64_t N, uint64_t max_scratch_bytes);
/* Pipelined fusion (an extension, the reference fuses one frame at a time,
 * tests/Raytracing.cpp:70-76).  Declares that the device inputs (d_depth, d_poses) of later
 * dmf_fuse_depth_device calls on this volume are ordered on `stream` (a hipStream_t the
 * caller writes them on) instead of on the volume's stream.  The brick pipeline then runs
 * each call's per-frame pass (pose table + pass A: back-projection, ray records, brick
 * counts) on a staging stream of the volume that waits only for `stream`, for its staging
 * slot's previous reader and (pass A itself) for the previous call's pass B, so that it
 * overlaps the previous call's phase F; the device-side batch cut, brick layout, pass B
 * (pair records) and phase F run on the volume's stream after pass A.  Two staging slots
 * alternate between super-batches, each with its
 * own pair records and half of the fusion budget (dmf_fuse_reserve).  `stream` is made to
 * wait until the call's pass A has read the inputs, so inputs rewritten there afterwards
 * stay ordered.  Results are identical to the serial order, and serial and pipelined calls
 * may be mixed on one volume without synchronising (a pipelined call waits for the serial
 * calls before it that used its slot).  Switching the mode frees the fusion scratch (after
 * synchronising the volume's streams) so that it is re-planned.  stream = NULL restores
 * the serial order (the default); a volume stream that is capturing a graph always runs
 * serially, and so does the host form dmf_fuse_depth (a captured graph must not be launched
 * while pipelined calls of the same volume are in flight: it reads the serial slot). */
int dmf_fuse_set_input_stream(dmf_volume* v, void* stream);
/* Phase-F event: `event` (a hipEvent_t the caller created; NULL = off) is recorded on the
 * volume's stream of every later fusion call right before its (first) phase F launch -- on
 * the brick pipeline after the call's pass B, on k_fuse_l before that kernel.  A caller that
 * pipelines its own steps makes the previous step's merge / finalize wait for it, so that
 * this HBM-bound work runs beside the issue-bound phase F instead of beside the next call's
 * passes A / B (bench.py).  The event is re-recorded by each call: wait on
 * it after the call returns and before the next call.  It must stay valid until it is
 * unregistered (event = NULL) or the volume is destroyed.  A call enqueued while the volume's
 * stream is capturing a graph does not record it (a record inside a graph would not re-record
 * the caller's event when the graph is launched): order captured work by the graph itself. */
int dmf_fuse_set_phase_event(dmf_volume* v, void* event);
/* How a fusion call of P frames of `cam`'s size on this volume is executed (no GPU work,
 * no allocation): brick = 1 for the brick-owned pipeline (k_bk_*), 0 for k_fuse_l.  The
 * brick pipeline runs pass A over super-batches of super_batch_poses frames; the DEVICE cuts
 * each into pose batches by the (ray, brick) pairs they really make against pair_capacity
 * records of record_bytes (no host synchronisation); at most max_batches batches, each of at
 * least poses_per_batch frames (the geometric bound rays x (1 + brick boundaries));
 * scratch_bytes = the pipeline's device scratch over its `slots` staging slots (2 when the
 * calls are pipelined). */
typedef struct dmf_fuse_plan_info {
  int32_t brick;
  int32_t max_batches;
  int32_t poses_per_batch;
  int32_t record_bytes;
  uint64_t pair_capacity;
  uint64_t scratch_bytes;
  int32_t super_batch_poses;
  int32_t slots;
} dmf_fuse_plan_info;
int dmf_fuse_plan(const dmf_volume* v, const dmf_camera* cam, int32_t P, dmf_fuse_plan_info* out);
/* Diagnostic (synchronises the stream): the pose batches the device cut the latest
 * brick-pipeline super-batch of this volume into (0 before any brick-pipeline call). */
int dmf_fuse_batches_used(dmf_volume* v, int32_t* batches);
/* Device-side check of the brick pipeline (synchronises the volume's streams): pass B
 * writes each (ray, brick) pair record into the slot range pass A counted for it; a store
 * outside the call's pair records is dropped, and every workgroup compares the slots it took
 * per brick with pass A's counts.  Returns DMF_ERR_DEVICE_CHECK (and clears the count) when
 * any fusion call since the last dmf_fuse_status disagreed -- their counters are invalid --
 * else DMF_OK; *faults (may be NULL) = the workgroup-brick disagreements seen.  The host
 * form dmf_fuse_depth runs this check itself. */
int dmf_fuse_status(dmf_volume* v, uint64_t* faults);
/* Elements of one tiled counter array (>= xdim*ydim*zdim: dims padded to 2, 2, 4). */
int dmf_fuse_counter_cells(const dmf_volume* v, int64_t* n);
/* Tiled counters -> x-major int32 (xdim*ydim*zdim). */
int dmf_fuse_counters_to_linear_device(dmf_volume* v, const int32_t* d_tiled, int32_t* d_linear);
/* clamp(hits*l_hit + misses*l_miss, l_min, l_max) -> int16 log-odds grid, x-major.
 * Host form: linear counters; device form: tiled counters. */
int dmf_fuse_finalize(dmf_volume* v, const int32_t* hits, const int32_t* misses, const dmf_fuse_params* prm,
                      int16_t* logodds);
int dmf_fuse_finalize_device(dmf_volume* v, const int32_t* d_hits, const int32_t* d_misses,
                             const dmf_fuse_params* prm, int16_t* d_logodds);

/* Ray-cast of a fused log-odds grid: what a camera at each of P poses sees in
 * `logodds` (int16, x-major over xdim*ydim*zdim, as dmf_fuse_finalize* writes it).  Pixel (r, c)
 * of pose p probes along exactly the ray the fusion traces for that pixel with depth range_mm
 * (1..65535) and stops at the first cell of that ray's cell sequence with log-odds >= threshold
 * (any int32).  Outputs, P*H*W each, either may be NULL:
 *   cell   the surface cell's getHashId(x, y, z); DMF_NO_CELL when the ray finds none (decide
 *          "no surface" from this: no hash is all ones);
 *   depth  what rayTraceVolume gives that voxel, int(round(1000 * camera-frame z of its
 *          centre)); -1 without a surface cell (a cell around the camera can legitimately have
 *          depth <= 0).
 * Only the volume's geometry is used, not its point-cloud occupancy, which the call leaves
 * untouched.  The solid mask (L >= threshold) is rebuilt from the grid on every call.
 * Host form: host pointers, synchronises.  Device form: device pointers, runs on the volume's
 * stream without synchronising, allocates only when its scratch must grow; d_logodds may be the
 * front of the merge's padded grid; d_stats (may be NULL): 2 counters += {rays that enter the
 * grid, rays with a surface cell}.  Null v / cam / grid / poses, range_mm outside 1..65535 and
 * P outside 1..65535 are DMF_ERR_INVALID; grids the fusion rejects are rejected alike. */
#define DMF_NO_CELL UINT64_MAX
int dmf_raycast_logodds(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses,
                        int32_t P, int32_t threshold, int32_t range_mm, int32_t* depth, uint64_t* cell);
int dmf_raycast_logodds_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds,
                               const float* d_poses, int32_t P, int32_t threshold, int32_t range_mm,
                               int32_t* d_depth, uint64_t* d_cell, uint64_t* d_stats);

/* View gain over a fused log-odds grid and next-best-view selection: which cells
 * that have not been observed yet would a camera at each of P candidate poses see?  `logodds` is
 * the int16 grid, x-major, as dmf_fuse_finalize* writes it.  A cell is solid iff its log-odds >=
 * occ_threshold, free iff it is not solid and its log-odds <= free_threshold, unknown otherwise
 * (any int32 pair; with (1, -1) unknown is exactly log-odds 0).  Pixel (r, c) of pose p walks the
 * ray-cast's cell sequence (§4.1: the fusion's ray for depth range_mm, 1..65535) and sees the
 * cells strictly before its first solid cell.  seen[p] = the unknown cells seen by at least one
 * pixel; gain[p] = their number.  Only the volume's geometry is used; its point-cloud occupancy
 * is neither read nor changed.
 *
 * Mask layout (§4.5): `words` = 8 x the grid's 8x8x8-cell tiles uint64 per pose; cell (x, y, z)
 * is bit i & 63 of word i >> 6 with i = tile << 9 | (x & 7) << 6 | (y & 7) << 3 | (z & 7), tiles
 * x-major over the grid padded to whole tiles; bits of padding cells are 0.  P x words uint64 is
 * what dmf_greedy_set_cover_masks_device takes.  dmf_view_gain_words and dmf_view_mask_index
 * (§4.5) are host arithmetic over the constructed volume's dimensions: the words per pose, and
 * the bit index i of a cell (DMF_ERR_INVALID outside the grid). */
int dmf_view_gain_words(const dmf_volume* v, int64_t* words);
int dmf_view_mask_index(const dmf_volume* v, int32_t x, int32_t y, int32_t z, uint64_t* bit);
/* §4.5, device form: device pointers, only enqueues on the volume's stream, allocates only when
 * its scratch must grow.  d_seen (P x words, overwritten: the call zeroes it) and d_gain (P) may
 * each be NULL, not both.  With d_seen NULL the masks live in the call's scratch, in pose batches
 * of at most max(1, 256 MiB / bytes per pose) poses: counting many candidates never needs P
 * masks.  d_stats (may be NULL): 3 counters += {rays with a non-empty sequence, rays stopped by
 * a solid cell, unknown cells seen summed over rays (a cell counts once per ray that sees it)}.
 * Status rules are the ray-cast's; all outputs NULL is DMF_ERR_INVALID; every argument is checked
 * before the volume is touched. */
int dmf_view_gain_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds, const float* d_poses,
                         int32_t P, int32_t occ_threshold, int32_t free_threshold, int32_t range_mm,
                         uint64_t* d_seen, uint64_t* d_gain, uint64_t* d_stats);
/* §4.5, host form: host pointers (seen: P x words, gain: P; each may be NULL, not both), uploads
 * the grid and the poses, synchronises. */
int dmf_view_gain(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses, int32_t P,
                  int32_t occ_threshold, int32_t free_threshold, int32_t range_mm, uint64_t* seen, uint64_t* gain);
/* §4.5, next best views: greedySetCover (Algorithms.hpp:38-86) over the P sets seen[p], as
 * dmf_greedy_set_cover_masks_device does it: the pose that adds most cells not yet covered, ties
 * to the lowest index, until the best adds nothing or fewer than min_gain.  The masks of all P
 * poses stay in device scratch (an allocation that fails: DMF_ERR_NOMEM); selected[P] receives
 * the chosen pose indices in selection order and *nselected their number, on the host; gain
 * (host, P, may be NULL) each pose's own gain[p].  Synchronises.  The device form takes a device
 * grid and device poses, the host form host ones. */
int dmf_next_best_views_device(dmf_volume* v, const dmf_camera* cam, const int16_t* d_logodds,
                               const float* d_poses, int32_t P, int32_t occ_threshold, int32_t free_threshold,
                               int32_t range_mm, int32_t min_gain, int32_t* selected, int32_t* nselected,
                               uint64_t* gain);
int dmf_next_best_views(dmf_volume* v, const dmf_camera* cam, const int16_t* logodds, const float* poses,
                        int32_t P, int32_t occ_threshold, int32_t free_threshold, int32_t range_mm,
                        int32_t min_gain, int32_t* selected, int32_t* nselected, uint64_t* gain);

/* Surface of a fused log-odds grid as an oriented cloud, in order: the cloud
 * that integratePointCloud(cloud, normals) (Volume.hpp:199-228) takes, from `logodds` (int16,
 * x-major over xdim*ydim*zdim, as dmf_fuse_finalize* writes it).  A cell is solid iff its
 * log-odds >= occ_threshold and free iff it lies in the grid with log-odds <= free_threshold
 * (any int32 pair; a neighbour outside the grid reads as 0 and is never free).  A surface cell
 * is a solid cell with a free face neighbour (6-neighbourhood).  Per surface cell, in ascending
 * getHashId (Volume.hpp:143-148; the x-major order in which a scan of voxels_[x][y][z] would
 * insert them), each output may be NULL:
 *   hash     getHashId(x, y, z);
 *   xyz      3 floats: the voxel centre as reverseRayTraceFast forms it from the index
 *            (RayTracingEngine.hpp:151-157): x = float(i * delta + min), centre = float(x + delta / 2);
 *   normals  3 floats towards free space: g_a = N(c - e_a) - N(c + e_a) over the face neighbours'
 *            log-odds (outside the grid: 0), n = float(g) / sqrtf(gx*gx + (gy*gy + gz*gz)) in
 *            float32 (Eigen's normalized()); (0, 0, 0) when g = 0.
 * Counts are {surface cells, solid cells} of the whole grid, whatever the capacity.  Only the
 * volume's geometry is used; its point-cloud occupancy is neither read nor changed.
 * Device form: device pointers, only enqueues on the volume's stream, allocates only when its
 * scratch must grow; writes the first min(count, cap) entries and nothing at or past cap, and
 * always d_count[2] (compare d_count[0] with cap).  Host form: host pointers, synchronises;
 * cap < count is DMF_ERR_CAPACITY with *n = the need and the outputs untouched, except that
 * cap = 0 with NULL outputs is the size query (DMF_OK); n and n_solid may be NULL.
 * dmf_volume_integrate_surface extracts on the device and hands xyz and normals to
 * integratePointCloud(cloud, normals) there: after the upload of the grid only the count (*n,
 * may be NULL) comes back.  Null v / grid, a negative cap and, in the device form, a null
 * d_count or three null outputs are DMF_ERR_INVALID; an unconstructed volume is DMF_ERR_STATE;
 * more than 2048 cells on an axis is DMF_ERR_RANGE. */
int dmf_grid_surface_device(dmf_volume* v, const int16_t* d_logodds, int32_t occ_threshold,
                            int32_t free_threshold, uint64_t* d_hash, float* d_xyz, float* d_normals,
                            int64_t cap, uint64_t* d_count);
int dmf_grid_surface(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold, int32_t free_threshold,
                     uint64_t* hash, float* xyz, float* normals, int64_t cap, int64_t* n, int64_t* n_solid);
int dmf_volume_integrate_surface(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold,
                                 int32_t free_threshold, int64_t* n);

/* Exact squared Euclidean distance field of a fused log-odds grid: for every
 * cell of `logodds` (int16, x-major over xdim*ydim*zdim, as dmf_fuse_finalize* writes it) how far
 * the nearest obstacle is.  A cell is solid iff its log-odds >= threshold (any int32), as in the
 * ray-cast: threshold 1 makes the observed-occupied cells the obstacles, threshold 0 also counts
 * every unobserved cell, which suits a conservative planner.
 *   dist2[x][y][z] (uint32, x-major like the grid) = the minimum over the solid cells (x', y', z')
 *   of (x-x')^2 + (y-y')^2 + (z-z')^2, exactly: 0 on solid cells, DMF_NO_DIST on every cell when
 *   the grid has no solid cell; there is no cap and no truncation radius.
 * The unit is the CELL INDEX, not the metre, so the field is an exact integer for every volume.
 * For cubic voxels (the reference drivers size all axes at 125 voxels/m) the distance in metres
 * is sqrtf(dist2) * delta; for anisotropic voxels sqrtf(dist2) * min(delta) is a lower bound.
 * Only the volume's geometry (its dims) is used; its point-cloud occupancy is neither read nor
 * changed.  Host form: host pointers, synchronises; n_solid (may be NULL) = the solid cells.
 * Device form: device pointers, only enqueues on the volume's stream, allocates only when its
 * scratch (8 B per cell) must grow and reuses it on later calls; d_dist2 is also the passes'
 * intermediate; d_count (may be NULL): 1 counter = the solid cells.
 * Null v / grid / dist2 are DMF_ERR_INVALID (checked before the volume is touched); an
 * unconstructed volume is DMF_ERR_STATE; more than 2048 cells on an axis is DMF_ERR_RANGE.
 *
 * Clearance of path segments, the planner's query: a[n][3] and b[n][3] are float32 world-frame
 * points, dist2 a field of this volume.  clear2[i] = the minimum of dist2 over the cells that the
 * ray with origin a[i] and endpoint b[i] updates in the point fusion above (every cell that would
 * receive a miss, or the hit: the same endpoint acceptance, clip, 1/256-cell quantisation and
 * integer DDA with ties x < y < z).  Only the part of a segment inside the grid is examined; a
 * segment with a non-finite coordinate, or one that misses the grid, visits no cell and gives
 * DMF_NO_DIST.  The caller compares clear2 with its own radius^2 in cells: a body of radius r cells
 * collides on the segment iff clear2 < r^2.  Null pointers and n < 0 are DMF_ERR_INVALID; n = 0 is
 * DMF_OK and touches nothing; the volume is checked as above.  Host form: host pointers,
 * synchronises.  Device form: device pointers, only enqueues on the volume's stream. */
#define DMF_NO_DIST UINT32_MAX
int dmf_grid_distance(dmf_volume* v, const int16_t* logodds, int32_t threshold, uint32_t* dist2,
                      int64_t* n_solid);
int dmf_grid_distance_device(dmf_volume* v, const int16_t* d_logodds, int32_t threshold, uint32_t* d_dist2,
                             uint64_t* d_count);
int dmf_grid_clearance(dmf_volume* v, const uint32_t* dist2, const float* a, const float* b, int64_t n,
                       uint32_t* clear2);
int dmf_grid_clearance_device(dmf_volume* v, const uint32_t* d_dist2, const float* d_a, const float* d_b,
                              int64_t n, uint32_t* d_clear2);

/* Travel field over a distance field of this volume: can a body of radius r reach
 * a cell from the seeds at all, and in how many steps?  dist2 is a field of dmf_grid_distance*
 * (DMF_NO_DIST allowed); a cell is traversable iff dist2 >= radius2 (radius2 = 1: every non-solid
 * cell; 0: every cell); seeds are n_seeds x 3 int32 cell indices.
 *   hops[x][y][z] (uint32, x-major like the grid) = the least number of steps of a path from any
 *   valid seed to the cell, a step going to one of the six face neighbours inside the grid and
 *   every cell of the path, both ends included, being traversable; 0 on a valid seed; DMF_NO_PATH
 *   on every cell that is not traversable or not reachable.
 * A seed outside the grid or on a cell that is not traversable is ignored, duplicates are allowed,
 * and no valid seed (n_seeds = 0 too) gives a field of DMF_NO_PATH and DMF_OK.  Steps cross faces
 * only, so hops over-estimates the Euclidean length of the best path, in cells, by up to sqrt(3).
 * info3 (may be NULL) receives 3 counters, written, not accumulated: {traversable cells, reached
 * cells, the largest finite hop count (0 when nothing is reached)}.  Only the volume's dims are
 * used; its point-cloud occupancy is neither read nor changed.
 * Host form: host pointers, synchronises.  Device form: device pointers on the volume's stream;
 * d_hops is also the rounds' work buffer.  The relaxation runs in rounds, one launch each, and the
 * host has to learn when a round changed nothing, so the device form WAITS FOR ITS OWN WORK like
 * dmf_next_best_views_device; d_info3 is complete when it returns.  Scratch (1 bit per cell and 8
 * B per 8x8x8 tile) is allocated when it must grow and reused.  Rounds are bounded by the
 * traversable count; past the bound the call returns DMF_ERR_DEVICE_CHECK.
 * Null v / dist2 / hops, null seeds with n_seeds > 0 and n_seeds < 0 are DMF_ERR_INVALID (checked
 * before the volume is touched); an unconstructed volume is DMF_ERR_STATE; more than 2048 cells
 * on an axis, or more than 2^31 cells in all, is DMF_ERR_RANGE.
 *
 * Path back from a cell: target3 is one int32 cell index, hops a field of the call above.  The
 * path is the cell sequence target, ..., seed of hops[target] + 1 cells: from a cell with value
 * k > 0 the next cell is the first face neighbour, in the order -x +x -y +y -z +z and skipping
 * those outside the grid, that holds k - 1.  A target outside the grid or with DMF_NO_PATH gives 0
 * cells and DMF_OK.  The walk ends on any field: where no neighbour holds k - 1 it stops and
 * returns what it has.  cells is cap x 3 int32.  Capacity as in dmf_grid_surface: the device form
 * writes the first min(length, cap) cells, nothing at or past cap, and always *d_n (compare it
 * with cap), and only enqueues; the host form returns DMF_ERR_CAPACITY with *n = the need and
 * cells untouched when cap < length, except that cap = 0 with NULL cells is the size query
 * (DMF_OK).  Null v / hops / target3 / n, cap < 0 and NULL cells with cap > 0 are DMF_ERR_INVALID;
 * the volume is checked as above. */
#define DMF_NO_PATH UINT32_MAX
int dmf_grid_travel(dmf_volume* v, const uint32_t* dist2, uint32_t radius2, const int32_t* seeds, int64_t n_seeds,
                    uint32_t* hops, uint64_t* info3);
int dmf_grid_travel_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_seeds,
                           int64_t n_seeds, uint32_t* d_hops, uint64_t* d_info3);
int dmf_grid_path(dmf_volume* v, const uint32_t* hops, const int32_t* target3, int32_t* cells, int64_t cap,
                  int64_t* n);
int dmf_grid_path_device(dmf_volume* v, const uint32_t* d_hops, const int32_t* d_target3, int32_t* d_cells,
                         int64_t cap, uint64_t* d_n);

/* The travel cost map of V cells: map[i][j] (int32, V x V, row-major) = the hop
 * count from cells[i] to cells[j] of the travel field above seeded at cells[i] alone, INT_MAX where
 * that is DMF_NO_PATH or cells[j] lies outside the grid (a row whose own cell is outside or blocked
 * is INT_MAX throughout) -- the fused grid's counterpart of dmf_collision_cost_map, with detours,
 * and what dmf_tour* takes.  cells is V x 3 int32.  One travel field per row into one reused hop
 * buffer of the volume's scratch, then a gather of the row's V entries; in the device form nothing
 * crosses to the host but the rounds' own "anything left?" words, and like dmf_grid_travel_device
 * it WAITS FOR ITS OWN WORK.  V = 0 is DMF_OK and writes nothing.  Null v / dist2, V < 0 and null
 * cells / map with V > 0 are DMF_ERR_INVALID; V > 46340 is DMF_ERR_RANGE; the volume is checked as
 * for dmf_grid_travel. */
int dmf_grid_travel_cost_map(dmf_volume* v, const uint32_t* dist2, uint32_t radius2, const int32_t* cells, int32_t V,
                             int32_t* map);
int dmf_grid_travel_cost_map_device(dmf_volume* v, const uint32_t* d_dist2, uint32_t radius2, const int32_t* d_cells,
                                    int32_t V, int32_t* d_map);

/* An open tour over a cost map: the order in which to visit V views, as the
 * reference's planners compute it from their cost map -- TSP::NearestNeighborSearch, then
 * TSP::TwoOptSearch (include/TSPSolver.hpp:76-98, :136-156).  map is V x V int32, row-major,
 * map[a][b] = the cost of going from a to b: what dmf_collision_cost_map* and
 * dmf_grid_travel_cost_map* write.  It may be asymmetric and may hold any int32; INT_MAX is "no
 * edge".  A tour is an OPEN path: V distinct indices, no edge back to the start.
 *   Nearest neighbour: path[0] = 0; from the current node the next one is the unvisited node with
 *   the smallest entry below INT_MAX in the current node's row, the lowest index among equals.
 *   Where every unvisited entry of the row is INT_MAX the reference aborts; here the lowest
 *   unvisited index is taken (a "forced pick") and counted.
 *   2-opt: the length of a path is INT_MAX if one of its edges is INT_MAX, else the sum of its
 *   edges.  The candidates (i, k), 1 <= i < k <= V - 1, are scanned in lexicographic order; the
 *   first one for which the path with positions i..k reversed is STRICTLY shorter is applied and
 *   the scan starts again; the solve ends with the scan that finds none.  Position 0 never moves.
 *   A path of length INT_MAX is not improved by another such path, however many INT_MAX edges go
 *   away.  max_rounds > 0 ends the solve after that many applied reversals; 0 runs to the end,
 *   which comes because every reversal lowers an integer length.
 * Sums are int64 here, so the result is defined for every input; it EQUALS THE REFERENCE'S WHEREVER
 * THE REFERENCE'S int SUMS DO NOT OVERFLOW, that is where no path's edges below INT_MAX sum to
 * INT_MAX or more in magnitude.
 * dmf_tour_nearest_neighbour* writes path; dmf_tour_two_opt* improves the caller's path in place
 * (any permutation of 0..V-1; the reference starts from 0, 1, 2, ...); dmf_tour* does the first,
 * then the second.  info5 (uint64, may be NULL) is written, not accumulated: {forced picks (0 for
 * dmf_tour_two_opt*), reversals applied, 1 if a scan found no improving candidate (never after
 * nearest neighbour alone, nor when max_rounds ended the solve) else 0, the sum of the final
 * path's edges below INT_MAX as an int64, the number of its INT_MAX edges}.
 * The calls need only a CREATED volume, for its device, stream and scratch (28 B per node), like
 * dmf_cloud_nearest*.  Host forms: host pointers, synchronise.  Device forms: device pointers on
 * the volume's stream.  2-opt runs in rounds of two launches, and the host has to learn when a
 * scan found nothing, so the device forms WAIT FOR THEIR OWN WORK like dmf_grid_travel_device;
 * d_info5 is complete when they return.
 * V = 0, 1 and 2 are DMF_OK with the only possible path.  A null v, V < 0, max_rounds < 0 and a
 * null map or path with V > 0 are DMF_ERR_INVALID; V > 46340 (V * V must stay below 2^31) is
 * DMF_ERR_RANGE and is checked before the pointers.  A path given to dmf_tour_two_opt* that
 * repeats an index or holds one outside 0..V-1 is DMF_ERR_INVALID: it is checked on the device,
 * before anything walks it, and left as it was.  Every applied reversal is checked on the device
 * to have made the path strictly shorter, which is what ends the solve; a round that did not (the
 * map was changed under the call) ends it with DMF_ERR_DEVICE_CHECK. */
int dmf_tour_nearest_neighbour(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, uint64_t* info5);
int dmf_tour_nearest_neighbour_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path,
                                      uint64_t* d_info5);
int dmf_tour_two_opt(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, int64_t max_rounds, uint64_t* info5);
int dmf_tour_two_opt_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path, int64_t max_rounds,
                            uint64_t* d_info5);
int dmf_tour(dmf_volume* v, const int32_t* map, int32_t V, int32_t* path, int64_t max_rounds, uint64_t* info5);
int dmf_tour_device(dmf_volume* v, const int32_t* d_map, int32_t V, int32_t* d_path, int64_t max_rounds,
                    uint64_t* d_info5);

/* Exact nearest neighbour of every point of one cloud in another, and the cloud error built on it
 * (DESIGN.md §4.7): what the reference's tests/ErrorCalc.cpp:71-97 asks of PCL's k-d tree
 * (nearestKSearch(pt, 1, ...)) one point at a time -- how far a reconstruction lies from a model.
 * query[n][3] and ref[m][3] are packed float32 points in the world frame; no alignment beyond 4
 * bytes is owed.  For a query q and a reference point r, all in float32 with no contraction,
 *   d2(q, r) = (dx*dx + dy*dy) + dz*dz,  dx = q.x - r.x and likewise dy, dz
 * (the accumulation order of the L2_Simple<float> functor of PCL's KdTreeFLANN).  A point is valid
 * iff its three coordinates are finite.  Each output may be NULL (not all four):
 *   dist2[i]  (float)  the minimum of d2(query[i], ref[j]) over the valid j;
 *   index[i]  (int32)  the LOWEST j that attains it;
 *             an invalid query gives dist2 = +inf and index = DMF_NO_POINT, and so does every query
 *             when no reference point is valid (m = 0 included);
 *   counts[2 + T] (uint64), written, not accumulated: {the valid queries that have a neighbour, the
 *             valid reference points, then for each of the T <= 8 thresholds t_k (doubles, read
 *             from a HOST pointer in both forms) how many of those queries have
 *             (double)sqrtf(dist2) > t_k} -- the reference's compare (ErrorCalc.cpp:82-91, 3 mm and
 *             5 mm; its else-if branch for 5 mm can never be taken, hence counts, not a colour);
 *   sums[2]   (double) {the largest (double)sqrtf(dist2) over the queries counted in counts[0],
 *             exact, and -1.0 when there are none (the reference's initial value); the sum of those
 *             distances, in an unspecified order (ErrorCalc.cpp's avg_error times its count, up to
 *             the rounding of the additions)}.
 * There is no search radius and no approximation: the result equals a brute-force scan bit for bit
 * on any input.  Limits: m <= 2^31 - 1; n is an int64.  A strongly clustered reference (one
 * outlier that stretches the box until the rest falls into one cell of the index) stays exact but
 * degenerates towards brute force over that cell.
 * The calls need only a CREATED volume, for its device, stream and scratch: the volume's geometry
 * and point-cloud occupancy are neither read nor changed, and an UNCONSTRUCTED volume is fine here
 * (every other grid call returns DMF_ERR_STATE for one).
 * Device form: device pointers (thresholds: host), only enqueues on the volume's stream, allocates
 * only when its scratch (16 B per reference point, at most 32 MiB of cells) must grow and reuses it
 * otherwise.  Host form: host pointers, synchronises.
 * A null v, a null query with n > 0, a null ref with m > 0, all four outputs null, a negative n or
 * m, T outside 0..8 and T > 0 with null thresholds are DMF_ERR_INVALID, all checked before anything
 * is touched; m >= 2^31 is DMF_ERR_RANGE.  n = 0 is DMF_OK and writes only the summaries
 * (counts[0] = 0, sums = {-1, 0}). */
#define DMF_NO_POINT (-1)
int dmf_cloud_nearest(dmf_volume* v, const float* query, int64_t n, const float* ref, int64_t m, float* dist2,
                      int32_t* index, const double* thresholds, int32_t T, uint64_t* counts, double* sums);
int dmf_cloud_nearest_device(dmf_volume* v, const float* d_query, int64_t n, const float* d_ref, int64_t m,
                             float* d_dist2, int32_t* d_index, const double* thresholds, int32_t T,
                             uint64_t* d_counts, double* d_sums);

/* Candidate views from an oriented cloud: the voxel-grid downsample that every
 * planner of the reference runs over its cloud (PointCloudProcessing::downsample, PCL's
 * VoxelGrid<PointXYZRGBNormal>) and the camera placement that follows it
 * (Algorithms::positionCameras, Algorithms.hpp:189-234, 281-298), bit for bit what the drop-in's
 * host code (compat/shims/pcl/filters/voxel_grid.h, compat/Algorithms.hpp) computes, and the
 * chain surface -> downsample -> placement over a fused grid.
 *
 * dmf_cloud_downsample*: xyz[n][3] and normals[n][3] (or NULL) are packed float32, n <= 2^31 - 1;
 * leaf[3] (a HOST pointer in both forms) is the leaf size, each finite and > 0.  All in float32
 * with no contraction: inv_a = 1.0f / leaf_a.  A point takes part iff its three coordinates are
 * finite; other points are skipped everywhere (the bounds too) and their normals are never read.
 * min_b_a = (int)floorf(min_a * inv_a) and max_b_a likewise over the participating points,
 * div_a = max_b_a - min_b_a + 1; a point's leaf is i0 + i1 div0 + i2 div0 div1 with
 * i_a = (int)floorf(p_a * inv_a) - min_b_a.  One entry per non-empty leaf, in ascending leaf,
 * each output may be NULL:
 *   out_xyz      3 floats: acc / (float)count, where acc starts at 0.0f and adds the leaf's points
 *                in ascending input index, one float32 add at a time;
 *   out_normals  3 floats: the same mean of the normals (a non-finite normal propagates); with
 *                DMF_DOWNSAMPLE_UNIT_NORMALS in flags (PCL >= 1.8 renormalises) the mean is divided
 *                by sqrtf(x*x + (y*y + z*z)) unless all three components are zero;
 *   out_points   int32: the leaf's population.
 * count[3] = {leaves, participating points, largest leaf population}, whatever the capacity.
 * A grid of more than 2^31 - 1 leaves (PCL: "leaf size is too small"), or a bound whose leaf
 * coordinate floorf(. * inv_a) is at or beyond 2^31 in magnitude, is refused: the host form returns
 * DMF_ERR_RANGE, the device form, which only enqueues, writes count[0] = DMF_LEAVES_REFUSED; no
 * output is touched in either.
 * Device form: device pointers, only enqueues on the volume's stream, allocates only when its
 * scratch (20 B per point, and the sort's) must grow; writes the first min(leaves, cap) entries and
 * nothing at or past cap, and always d_count[3].  Host form: host pointers, synchronises; cap <
 * leaves is DMF_ERR_CAPACITY with count[0] = the need and the outputs untouched, except that cap = 0
 * with NULL outputs is the size query (DMF_OK); count may be NULL.  n = 0, or no finite point,
 * gives 0 leaves and DMF_OK.  The volume only lends its device, stream and scratch, as for
 * dmf_cloud_nearest*: an UNCONSTRUCTED volume is fine.  A null v / leaf, a null xyz with n > 0, a
 * negative n or cap, a leaf that is not finite and > 0, unknown flags, out_normals without normals
 * and, in the device form, a null d_count are DMF_ERR_INVALID; n >= 2^31 is DMF_ERR_RANGE.
 *
 * dmf_position_cameras*: for each of m locations xyz[i] with normal n = normals[i], one pose of 12
 * floats (rows 0..2 of the camera-to-world transform, as every other call takes them):
 *   first, unless DMF_PLACE_KEEP_NORMALS is in flags (positionCameras): a normal with n[2] <= 0 is
 *   negated IN `normals`, all three components (-0.0 flips, NaN does not);
 *   then (positionCamera(locations, i, distance)): columns x = (0, -1, 0), y = (1, 0, 0), z = -n,
 *   position_a = (float)((double)((float)(distance_mm / 1000.0) * n_a) + (double)p_a).
 * DMF_PLACE_KEEP_NORMALS is the plain positionCamera loop of CameraPathGen.cpp:77-81: a fused grid
 * has surfaces that face down, and flipping those would put the camera behind the surface.  The
 * volume as above.  Null v, negative m, null pointers with m > 0 and unknown flags are
 * DMF_ERR_INVALID; m = 0 is DMF_OK.
 *
 * dmf_grid_surface_views*: dmf_grid_surface_device (xyz and normals) -> downsample -> placement
 * over `logodds`, with nothing but counts crossing to the host: poses[cap][12], and the candidate
 * locations xyz[cap][3] and their normals[cap][3] after the placement's flip (each may be NULL);
 * count[3] = {views, surface cells, solid cells}.  The poses can go straight into
 * dmf_view_gain_device, dmf_next_best_views_device or dmf_reverse_visibility_device.  Capacity,
 * the size query and the refusal as for the downsample (count[0] = DMF_LEAVES_REFUSED).  The device
 * form reads the surface count back (16 bytes, synchronises once) to size the cloud's scratch
 * before it enqueues the rest.  The surface call's conditions hold: an unconstructed volume is
 * DMF_ERR_STATE, more than 2048 cells on an axis DMF_ERR_RANGE. */
#define DMF_LEAVES_REFUSED 0xFFFFFFFFFFFFFFFFull /* UINT64_MAX */
#define DMF_DOWNSAMPLE_UNIT_NORMALS 1u
#define DMF_PLACE_KEEP_NORMALS 1u
int dmf_cloud_downsample(dmf_volume* v, const float* xyz, const float* normals, int64_t n, const float* leaf,
                         uint32_t flags, float* out_xyz, float* out_normals, int32_t* out_points, int64_t cap,
                         uint64_t* count);
int dmf_cloud_downsample_device(dmf_volume* v, const float* d_xyz, const float* d_normals, int64_t n,
                                const float* leaf, uint32_t flags, float* d_out_xyz, float* d_out_normals,
                                int32_t* d_out_points, int64_t cap, uint64_t* d_count);
int dmf_position_cameras(dmf_volume* v, const float* xyz, float* normals, int64_t m, uint32_t distance_mm,
                         uint32_t flags, float* poses);
int dmf_position_cameras_device(dmf_volume* v, const float* d_xyz, float* d_normals, int64_t m, uint32_t distance_mm,
                                uint32_t flags, float* d_poses);
int dmf_grid_surface_views(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold, int32_t free_threshold,
                           const float* leaf, uint32_t downsample_flags, uint32_t distance_mm,
                           uint32_t placement_flags, float* poses, float* xyz, float* normals, int64_t cap,
                           uint64_t* count);
int dmf_grid_surface_views_device(dmf_volume* v, const int16_t* d_logodds, int32_t occ_threshold,
                                  int32_t free_threshold, const float* leaf, uint32_t downsample_flags,
                                  uint32_t distance_mm, uint32_t placement_flags, float* d_poses, float* d_xyz,
                                  float* d_normals, int64_t cap, uint64_t* d_count);

/* ---- multi-GPU merge over RCCL ------------------------
 * Poses shard across ranks, each rank fuses into its own replica of the counters, and
 * the replicas merge with integer collectives (bit-identical to one rank fusing all
 * poses).  `comm` is an ncclComm_t (RCCL) as void*: torch's ProcessGroupNCCL._comm_ptr()
 * or one made with dmf_comm_init_rank.  Collectives (and the slab finalize) run on
 * `stream` (hipStream_t; NULL = the volume's stream), e.g. a communication stream that
 * overlaps the next fusion call on the volume's stream. */
#define DMF_COMM_ID_BYTES 128
int dmf_rccl_version(int32_t* version);
/* ncclGetUniqueId into id[DMF_COMM_ID_BYTES] (rank 0; share it with the other ranks). */
int dmf_comm_unique_id(void* id);
int dmf_comm_init_rank(void** comm, int32_t nranks, const void* id, int32_t rank, int32_t device);
int dmf_comm_destroy(void* comm);
/* ncclCommCount / ncclCommUserRank of a communicator (e.g. torch's, to report the ranks the
 * merge's collectives span). */
int dmf_comm_shape(void* comm, int32_t* nranks, int32_t* rank);
/* Tiled counter elements per array padded to whole tile rows per rank (>= the unpadded
 * dmf_fuse_counter_cells), and the padded int16 log-odds grid (>= xdim*ydim*zdim) used by
 * dmf_fuse_merge_finalize_device.  Counters = [hits | misses], each n_padded elements. */
int dmf_fuse_counter_cells_padded(const dmf_volume* v, int32_t nranks, int64_t* n_padded);
int dmf_fuse_logodds_cells_padded(const dmf_volume* v, int32_t nranks, int64_t* n_padded);
/* The merge's slab arithmetic for `rank` of `nranks` (rank = -1: the whole grid), so a
 * caller with its own collectives (MPI, gloo, a test emulating ranks on one GPU) can
 * reproduce dmf_fuse_merge_finalize_device exactly: each counter array holds n_padded
 * elements; the reduce-scatter gives rank r the sums of elements [chunk_offset,
 * chunk_offset + chunk) of each array (in place); rank r finalizes counter tiles
 * [tile_begin, tile_end) (tile rows of 2 x-rows, clipped to the grid); the all-gather moves
 * slab_bytes of int16 log-odds from byte slab_offset of each rank's padded grid
 * (logodds_padded elements). */
typedef struct dmf_merge_plan {
  int64_t n_padded;
  int64_t chunk;
  int64_t chunk_offset;
  int64_t tile_begin;
  int64_t tile_end;
  int64_t logodds_padded;
  int64_t slab_bytes;
  int64_t slab_offset;
} dmf_merge_plan;
int dmf_fuse_merge_plan(const dmf_volume* v, int32_t nranks, int32_t rank, dmf_merge_plan* out);
/* The same for a grid of xdim x ydim x zdim cells (host only: no volume, no GPU). */
int dmf_fuse_merge_plan_dims(int32_t xdim, int32_t ydim, int32_t zdim, int32_t nranks, int32_t rank,
                             dmf_merge_plan* out);
/* Finalize rank `rank`'s slab (rank = -1: every slab) of the padded [hits | misses]
 * counters (n_padded per array for nranks) into the padded int16 log-odds grid, on
 * `stream` (NULL = the volume's).  The merge's own finalize step. */
int dmf_fuse_finalize_slab_device(dmf_volume* v, const int32_t* d_counters, const dmf_fuse_params* prm,
                                  int16_t* d_logodds, int32_t nranks, int32_t rank, void* stream);
/* In-place all-reduce(sum) of [hits | misses] (2*n_per_array int32). */
int dmf_fuse_allreduce_device(dmf_volume* v, int32_t* d_counters, int64_t n_per_array, void* comm, void* stream);
/* Merge + finalize: reduce-scatter(sum) of hits and of misses over whole tile rows, this
 * rank finalizes its slab, all-gather of the int16 slabs: every rank ends with the full
 * log-odds grid in d_logodds (x-major; the first xdim*ydim*zdim of the padded buffer).
 * d_counters: padded [hits | misses]; afterwards only this rank's slab holds sums.
 * comm = NULL: a single rank (no collective): the whole grid is finalized on `stream`. */
int dmf_fuse_merge_finalize_device(dmf_volume* v, int32_t* d_counters, const dmf_fuse_params* prm,
                                   int16_t* d_logodds, void* comm, void* stream);
/* Voxel::view / Voxel::good of the replicated occupied list after pose-sharded queries:
 * good = all-reduce(max); view = the smallest non-zero id over the ranks (classify sets
 * view only while it is 0, RayTracingEngine.hpp:354, so a single rank keeps the first
 * pose's id: the same when view ids grow with pose order, as in the reference's loops). */
int dmf_flags_allreduce(dmf_volume* v, void* comm, void* stream);

/* ---- persistent fused grid (checkpoint / resume; host only, no GPU needed) ------
 * The clamped int16 log-odds grid (x-major, dims[0]*dims[1]*dims[2] cells) with its
 * geometry and fusion parameters, little-endian, CRC-32 checked (csrc/dmf_io.hip).  The
 * reference's only persistent outputs are text (FileRoutines.hpp:98-112
 * writeCameraLocations); this is the fusion engine's counterpart.  dmf_grid_load with
 * logodds = NULL reads the header only; DMF_ERR_CAPACITY if cap < the grid's cells; a bad
 * magic, version, size or checksum is DMF_ERR_INVALID. */
typedef struct dmf_grid_header {
  int32_t dims[3];
  int32_t reserved;
  double bounds[6]; /* xmin, xmax, ymin, ymax, zmin, zmax (setDimensions) */
  dmf_fuse_params params;
} dmf_grid_header;
int dmf_grid_save(const char* path, const dmf_grid_header* h, const int16_t* logodds);
int dmf_grid_load(const char* path, dmf_grid_header* h, int16_t* logodds, int64_t cap);

/* ---- OccupancyGrid  (include/OccupancyGrid.hpp:50-318) ----------------------- */
/* The reference's second fusion path.  updateStates is computed in the deterministic
 * single-threaded order (the reference's OpenMP loops race); state is dense, x-major,
 * persistent across calls. */
typedef struct dmf_ogrid dmf_ogrid;
int dmf_ogrid_create(dmf_ogrid** out, int32_t device);
int dmf_ogrid_destroy(dmf_ogrid* g);
int dmf_ogrid_set_stream(dmf_ogrid* g, void* hip_stream);
/* setDimensions(bounds[6]) + setResolution(float x3) + setK + construct (:323-352). */
int dmf_ogrid_setup(dmf_ogrid* g, const double* bounds, float xres, float yres, float zres, int32_t k);
int dmf_ogrid_get_dims(const dmf_ogrid* g, int32_t* dims);
/* updateStates(cloud, normals) (:99-164): cloud n_cloud x 3 floats, normals n_normals x 6
 * floats (x, y, z, nx, ny, nz).  Host and device-pointer forms. */
int dmf_ogrid_update_states(dmf_ogrid* g, const float* cloud, int64_t n_cloud, const float* normals,
                            int64_t n_normals);
int dmf_ogrid_update_states_device(dmf_ogrid* g, const float* d_cloud, int64_t n_cloud, const float* d_normals,
                                   int64_t n_normals);
/* Dense state copies (any may be NULL): normal / centroid 3 floats per voxel, count,
 * flags (bit 0 occupied, bit 1 normal_found). */
int dmf_ogrid_state(const dmf_ogrid* g, float* normal, float* centroid, int32_t* count, uint8_t* flags);
/* Write the dense state (the reference's public voxels_ fields; any may be NULL). */
int dmf_ogrid_set_state(dmf_ogrid* g, const float* normal, const float* centroid, const int32_t* count,
                        const uint8_t* flags);
/* mode 0 downloadCloud (:166-193), 1 downloadHQCloud (count > 100, :283-318): occupied
 * voxels in x-major order as (cx, cy, cz, nx, ny, nz).  Modes 2 / 3 downloadReorganizedCloud
 * (:200-286) with clean = false / true: every occupied voxel (clean: count >= 100 at its
 * turn) merges into the voxel holding its centroid, in the single-threaded x-major order
 * the reference's OpenMP loop races over; the merged voxels, x-major.  DMF_ERR_CAPACITY
 * (n set) if n > cap. */
int dmf_ogrid_download(dmf_ogrid* g, int32_t mode, float* out, int64_t cap, int64_t* n);

/* ---- device memory helpers for callers without their own allocator ---------- */
int dmf_device_malloc(dmf_volume* v, void** d_ptr, size_t bytes);
int dmf_device_free(dmf_volume* v, void* d_ptr);
int dmf_memcpy_h2d(dmf_volume* v, void* d_dst, const void* h_src, size_t bytes);
int dmf_memcpy_d2h(dmf_volume* v, void* h_dst, const void* d_src, size_t bytes);
int dmf_memset_device(dmf_volume* v, void* d_ptr, int value, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* DMF_H_ */
