/*
 * lo_gmap.h — C ABI of the MI355X-native global-map builder: keyframe feature clouds + keyframe poses -> the
 * voxel-grid-downsampled world map, the product of a finished (or loop-corrected) run.
 *
 * Replaces, for a host that keeps the reference's frame loop:
 *   Estimator::save_map_to_ply     (src/processing/Estimator.cpp:1248-1305)  transform, concatenate, downsample, save
 *   util::VoxelGrid::filter        (src/util/PointCloudUtils.h:462-557)      fp32 running average per voxel
 *   util::save_point_cloud_ply     (src/util/PointCloudUtils.cpp:146-184)    lo_save_ply in lo_io.h
 *
 * The arithmetic, bit for bit (every fp32 operation separately rounded, no FMA):
 *   world point   Matrix4f * (x, y, z, 1) in transform_point_cloud's order;
 *   voxel key     k = (int)floorf(p / leaf) per axis, one correctly rounded fp32 division;
 *   per voxel     its points in input order (keyframe insertion order, then index inside the keyframe): the first is
 *                 copied with w = 1; each further one: tw = w + 1.0f, a = w / tw, b = 1.0f / tw,
 *                 c = a * c + b * p per axis, w = tw;
 *   output order  voxels ascending in (kx, ky, kz), signed, x most significant (std::map<VoxelKey, ...> iteration).
 *
 * The one stated limit: voxel keys must lie in [-2^20, 2^20) per axis and every world point must be finite.  A build
 * that meets a point outside that returns LO_ERR_ARG, names the number of such points in lo_gmap_last_error and
 * produces no result (the reference's int cast is undefined there; with leaf 0.2 the range is +-209 km).
 *
 * Conventions as lo_iris.h: an opaque handle created against a context (its device; its stream, looked up on every
 * call so lo_set_stream is followed), plain pointers and sizes, the caller owns every host buffer, LO_* return codes
 * (LO_INSUFFICIENT = the reference's `false` for an empty map), negative = errors with the text in
 * lo_gmap_last_error.  Not thread-safe.  Every call is synchronous.  The context must outlive the handle.
 */
#ifndef LO_GMAP_H
#define LO_GMAP_H

#include <stddef.h>
#include <stdint.h>

#include "lo_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LO_GMAP_STAGES 4   /* lo_gmap_stage_ms: transform + key, sort, heads + gather + scan, centroids */

typedef struct lo_gmap lo_gmap;

/* max_points: stored points over all keyframes; max_keyframes: keyframes.  Every device buffer (84 B per point of
 * max_points plus the sort's work space) is allocated here; nothing is allocated per keyframe or per build. */
lo_gmap*    lo_gmap_create(lo_ctx* ctx, size_t max_points, size_t max_keyframes, int* err);
void        lo_gmap_destroy(lo_gmap* g);
const char* lo_gmap_last_error(const lo_gmap* g);
int         lo_gmap_clear(lo_gmap* g);              /* forgets the keyframes and the last build's result */
size_t      lo_gmap_keyframes(const lo_gmap* g);
size_t      lo_gmap_points(const lo_gmap* g);       /* stored points over all keyframes */

/* Appends a keyframe's feature cloud (sensor frame, AoS float3) to the device arena.  pts_xyz: host pointer, or
 * (on_device != 0) a device pointer on the context's device.  n = 0 keeps the keyframe without points (the
 * reference's `continue`: it still takes a pose in lo_gmap_build).  LO_ERR_CAPACITY past either limit; the builder
 * is then unchanged. */
int lo_gmap_add_keyframe(lo_gmap* g, int64_t keyframe_id, const float* pts_xyz, size_t n, int on_device);
/* The same for the context's last device-filtered scan (lo_icp_optimize_raw / lo_voxel_filter_gpu: the keyframe's
 * feature cloud), copied device to device; only its 4-byte count is read back.  LO_ERR_STATE when the context has no
 * such scan. */
int lo_gmap_add_from_scan(lo_gmap* g, int64_t keyframe_id);
/* Keyframe `index` (insertion order) in place: its id (nullable), the device pointer of its stored cloud inside the
 * arena (sensor frame, AoS float3) and its point count -- no copy, e.g. the matched cloud of lo_icp_optimize_loop_dev.
 * The pointer is valid until lo_gmap_clear or lo_gmap_destroy (the arena never moves).  A keyframe stored with 0
 * points gives n = 0 (its pointer is then not to be read).  LO_ERR_ARG for an index past the end. */
int lo_gmap_keyframe_points(lo_gmap* g, size_t index, int64_t* keyframe_id, const float** d_xyz, size_t* n);

/* The map at the given poses: poses_3x4 is n_poses row-major 3x4 world-from-sensor matrices, one per keyframe in
 * insertion order; n_poses must equal lo_gmap_keyframes (else LO_ERR_ARG).  voxel_size > 0: the voxel-grid filter of
 * the transformed concatenation; otherwise (Estimator.cpp:1284-1285) the transformed concatenation itself, in input
 * order.  *out_n (nullable) receives the number of result points.  LO_INSUFFICIENT when no point is stored.  May be
 * called again with other poses: the stored clouds are never modified. */
int lo_gmap_build(lo_gmap* g, const float* poses_3x4, size_t n_poses, float voxel_size, size_t* out_n);

/* The last build's result.  out_xyz = NULL returns its size; otherwise at most cap points are written and their
 * number is returned.  LO_ERR_STATE (negative) when there is no result. */
long long lo_gmap_download(lo_gmap* g, float* out_xyz, size_t cap);
/* ... in place: valid until the next build, clear or destroy. */
int lo_gmap_device_points(lo_gmap* g, const float** d_xyz, size_t* n);
/* ... written with lo_save_ply (lo_io.h). */
int lo_gmap_save_ply(lo_gmap* g, const char* path);

/* Timing harness (scripts/gmap_bench.py): one warm-up build, then reps back-to-back builds without the final count
 * readback; average device time per build (HIP events).  A second set of reps with an event after every stage fills
 * the per-stage averages lo_gmap_stage_ms returns (LO_GMAP_STAGES floats; the stages past the first are 0 for
 * voxel_size <= 0). */
int lo_gmap_bench_build(lo_gmap* g, const float* poses_3x4, size_t n_poses, float voxel_size, int reps, float* avg_ms);
int lo_gmap_stage_ms(const lo_gmap* g, float* out_ms);

/* util::VoxelGrid::filter on one core (context-free, host-only, no GPU needed): the CPU baseline and the host-side
 * parity anchor of lo_gmap_build.  out_xyz = NULL returns the number of voxels; otherwise at most cap centroids are
 * written in key order.  n = 0 or voxel_size <= 0 gives 0 (the reference clears the output); LO_ERR_ARG when a point
 * is non-finite or its key is out of range (the limit above). */
long long lo_gmap_voxelgrid_host(const float* xyz, size_t n, float voxel_size, float* out_xyz, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LO_GMAP_H */
