/*
 * lo_map.h — map-side C ABI: the 2-level voxel/surfel map that feeds the ICP's surfel table, and the
 * scan downsampler that feeds its point cloud.  Host C++ (host form).
 *
 *   lo_voxelmap_*   replaces map::VoxelMap's build side: UpdateVoxelMap (src/database/VoxelMap.cpp:128-262),
 *                   AddPoint (:99-120), surfel PCA + planarity erase (:187-261), GetPointCloud (:388-403).
 *   lo_voxel_filter replaces map::FastVoxelFilter::filter (src/database/VoxelMap.h:73-104).
 *
 * Results are bit-identical to the reference's fp32 arithmetic (insertion-ordered containers with
 * unordered_dense's swap-with-last erase, Eigen JacobiSVD<Matrix3f> restated), checked against the oracle.
 * Every lo_voxelmap_* call (the const readers included: they apply pending device fits) locks the map's recursive
 * mutex, as the reference's VoxelMap does, so one map may be used from several threads.
 */
#ifndef LO_MAP_H
#define LO_MAP_H

#include <stddef.h>
#include <stdint.h>

#include "lo_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lo_voxelmap lo_voxelmap;

lo_voxelmap* lo_voxelmap_create(float voxel_size, int hierarchy_factor, float planarity_threshold, int compute_surfels);
void         lo_voxelmap_destroy(lo_voxelmap* m);
/* UpdateVoxelMap(new_cloud (world frame), sensor_position, max_distance, is_keyframe) */
int          lo_voxelmap_update(lo_voxelmap* m, const float* world_xyz, size_t n, const double sensor[3],
                                double max_distance, int is_keyframe);
/* ApplyTransformAndRehash(T_correction) (VoxelMap.cpp:264-302; called after pose-graph optimisation, Estimator.cpp:877,
 * :1181): every L0 centroid moved by T (row-major 3x4) and re-keyed, collisions merged, surfels recomputed.
 * The next lo_map_sync_voxelmap uploads the whole map. */
int          lo_voxelmap_apply_transform(lo_voxelmap* m, const float T[12]);
/* Device surfel fits: with enable, UpdateVoxelMap records each touched L1 voxel's refit
 * (its children's centroids in child order) instead of fitting on the host; the next lo_map_sync_voxelmap of a
 * context that mirrors this map runs them there (k_surfel_fit: the same fp32 mean / covariance / JacobiSVD code)
 * and patches its table, and the results come back to the map before anything reads it -- surfel fields, or the
 * planarity erase of the voxel and its children in the sequential loop's order.  Bit-identical to enable = 0.
 * Without such a sync the map fits on the host when it is next read. */
int          lo_voxelmap_set_device_fit(lo_voxelmap* m, int enable);
size_t       lo_voxelmap_l0_count(const lo_voxelmap* m);
size_t       lo_voxelmap_l1_count(const lo_voxelmap* m);
size_t       lo_voxelmap_surfel_count(const lo_voxelmap* m);
/* L1 voxels with has_surfel, in L1 iteration order. Returns the number written. */
size_t       lo_voxelmap_get_surfels(const lo_voxelmap* m, int32_t* keys_xyz, float* normals, float* centroids,
                                     float* planarity, size_t cap);
/* The L1 keys whose surfel the last lo_voxelmap_update may have changed -- created, refitted, lost its planarity or
 * its children, erased by the radius prune or the planarity test (VoxelMap.cpp:146-169, :187-261) -- each key once,
 * ordered by key (an update that changed nothing gives none).  What the reference's UpdateVoxelMap
 * collects with the two-line hook INTEGRATION.md shows, for the adapter's keyed sync_map (only these voxels patched:
 * GetSurfelAtPoint at each key's centre, lo_map_patch_surfels).  After lo_voxelmap_apply_transform every key moved:
 * none are listed, upload the whole map.  Returns the count; writes up to cap keys. */
size_t       lo_voxelmap_changed_l1(const lo_voxelmap* m, int32_t* keys_xyz, size_t cap);
/* GetSurfelAtPoint (VoxelMap.cpp:368-386): 1 and the normal / centroid of the surfel of p's L1 voxel
 * (PointToVoxelKey(p, 1)) if it has one, else 0. */
int          lo_voxelmap_surfel_at(const lo_voxelmap* m, const float p[3], float normal[3], float centroid[3]);
/* The keyed sync's lookup loop in one call: for each of n L1 keys, GetSurfelAtPoint at the key's voxel centre
 * ((k + 0.5) * voxel * factor per axis, fp32) -- present[i] = 1 and its normal / centroid, or 0 and zeros.  The
 * arrays go straight to lo_map_patch_surfels.  Returns the number present. */
size_t       lo_voxelmap_surfels_at_keys(const lo_voxelmap* m, const int32_t* keys_xyz, size_t n, float* normals,
                                         float* centroids, uint8_t* present);
/* GetPointCloud: L0 centroids in L0 iteration order. */
size_t       lo_voxelmap_get_l0(const lo_voxelmap* m, float* xyz, size_t cap);
/* Upload the map's surfels to an ICP context (lo_map_set_surfels). */
int          lo_map_set_from_voxelmap(lo_ctx* ctx, const lo_voxelmap* m);
/* Bring the context's device surfel table up to date with the map after UpdateVoxelMap (Estimator.cpp:457): when the
 * table was last synced from this map, only the L1 voxels changed since then are patched in place
 * (lo_map_patch_surfels); otherwise (first sync, another map, KDTree mode, table full) the whole map is uploaded.
 * patched (nullable): the number of patched voxels, or -1 after a full upload. */
int          lo_map_sync_voxelmap(lo_ctx* ctx, const lo_voxelmap* m, int* patched);

/* FastVoxelFilter::filter(input, output, stride): returns the number of output points (<= n). */
size_t       lo_voxel_filter(const float* in_xyz, size_t n, float voxel_size, int stride, float* out_xyz);

/* ---- device-resident map ----
 * The same UpdateVoxelMap / AddPoint / radius prune / planarity erase / ApplyTransformAndRehash as lo_voxelmap_*,
 * kept in HBM next to an ICP context (surfel mode) whose surfel table it maintains in place: every update is ten
 * kernel launches on the context's stream and no host work, and the containers (L0 / L1 order, children order,
 * centroids, surfels) equal the host map's bit for bit.  Capacities are fixed at creation (max_l0 L0 voxels,
 * max_l0 / 2 L1 voxels, max_points per update); an overflow or a key beyond +-2^20 sets an error bit reported by
 * lo_devmap_counts / lo_devmap_status.  hierarchy_factor 1 or 3.  Destroy the map before its context.  The map
 * follows the context's stream: after lo_set_stream its launches go to the new stream. */
typedef struct lo_devmap lo_devmap;
lo_devmap*  lo_devmap_create(lo_ctx* ctx, float voxel_size, int hierarchy_factor, float planarity_threshold,
                             size_t max_l0, size_t max_points, int* err);
void        lo_devmap_destroy(lo_devmap* m);
const char* lo_devmap_last_error(const lo_devmap* m);
/* UpdateVoxelMap(cloud, sensor, max_distance, is_keyframe): world_xyz on the host (on_device = 0, copied) or a device
 * pointer (on_device = 1, read by the kernels, valid until they ran) */
int         lo_devmap_update(lo_devmap* m, const float* world_xyz, size_t n, int on_device, const double sensor[3],
                             double max_distance, int is_keyframe);
/* the context's last device-filtered scan moved to the world frame by T (util::transform_point_cloud) and inserted,
 * sensor = T's translation: create_keyframe's update (Estimator.cpp:370-530) without the scan leaving the device */
int         lo_devmap_update_from_scan(lo_devmap* m, const float T[12], double max_distance);
/* ApplyTransformAndRehash(T) (VoxelMap.cpp:264-302) + RecomputeAllSurfels (:304-366) */
int         lo_devmap_apply_transform(lo_devmap* m, const float T[12]);
/* out = {L0 voxels, L1 voxels, surfels, error bits}; syncs the stream.  LO_ERR_CAPACITY when error bits are set. */
int         lo_devmap_counts(lo_devmap* m, size_t out[4]);
/* the error bits only (one 64-byte copy; syncs the stream): LO_OK, or LO_ERR_CAPACITY with lo_devmap_last_error set
 * when an update overflowed a capacity or met a key beyond +-2^20 (the update aborted, the map is stale) */
int         lo_devmap_status(lo_devmap* m);
/* the same check without a stream sync: _async enqueues the copy of the error bits (pinned memory + an event) behind
 * the work enqueued so far; _poll returns LO_ERR_CAPACITY once that copy has landed and shows error bits, else LO_OK
 * (also while it is still in flight).  The frame loop enqueues after every keyframe's update and polls after each
 * frame's synchronous ICP, so an aborted update is reported at the first frame tracked after it. */
int         lo_devmap_status_async(lo_devmap* m);
/* KDTree-mode context (use_surfel_correspondence = 0): RebuildKdTree (VoxelMap.cpp:420-438) on the device -- the
 * context's correspondence grid rebuilt from the map's L0 centroids in L0 (GetPointCloud) order, equal to
 * lo_map_set_points on the same points; one small readback (count, bounds) per call.  Distance ties that the
 * reference's kd visit order would decide re-run the scan with that order (lo_kd_reruns). */
int         lo_devmap_sync_points(lo_devmap* m);
int         lo_devmap_status_poll(lo_devmap* m);
/* the containers in their order (tests / GetPointCloud): L0 keys, centroids, point counts; L1 keys, surfel flag,
 * normal, centroid, planarity, child count and children keys (27 per voxel) */
size_t      lo_devmap_get_l0(lo_devmap* m, int32_t* keys, float* xyz, int32_t* point_counts, size_t cap);
size_t      lo_devmap_get_l1(lo_devmap* m, int32_t* keys, uint8_t* has_surfel, float* normals, float* centroids,
                             float* planarity, int32_t* child_counts, int32_t* children, size_t cap);

/* ---- the maps of a batch (lo_icp.h lo_batch_*) ----
 * UpdateVoxelMap for the keyframes of a batch: for every job j with active[j] != 0, what
 * lo_devmap_update_from_scan(maps[j], T + 12*j, max_distance) does, in one set of launches for all active jobs on the
 * batch stream (24 launches, blockIdx.y = active job; the single-workgroup phases run one workgroup per job).
 * maps[j] was created on the batch's context j (else LO_ERR_ARG; entries of inactive jobs are not read).  Each job
 * reads its own context's device-filtered scan and device count (lo_batch_filter_raw* or lo_voxel_filter_gpu left
 * them there), and its map afterwards equals the single call's bit for bit; a job whose count is 0 changes nothing; a
 * job that overflows a capacity aborts its own update and sets its own error bits.  Maps of different capacities may
 * share a batch; single and batched updates may alternate on one map.  Enqueues and returns; the contexts must be
 * idle, as for every batch call, and whatever the next batch call runs on a context stream is ordered behind the
 * update.  Before a map is used through its own context (lo_devmap_counts, lo_devmap_update...), wait for the batch
 * stream: lo_batch_maps_status does.  A context whose table was replaced since the last update (an unrelated
 * lo_map_set_surfels, say) has it emptied and refilled on its own stream before this update; the call first waits
 * on the host for the batch's previous update.  LO_ERR_STATE while a batch optimize is in flight. */
int         lo_batch_update_maps(lo_batch* b, lo_devmap* const* maps, const unsigned char* active, const float* T,
                                 double max_distance);
/* The map correction after accepted loops, for the jobs of a batch: for every job j with active[j] != 0, what
 * lo_devmap_apply_transform(maps[j], T + 12*j) does -- ApplyTransformAndRehash (VoxelMap.cpp:264-302), then
 * RecomputeAllSurfels (:304-366) -- for all active jobs together on the batch stream.  T: count x 12, one row-major 3x4
 * correction per job; the entries of inactive jobs are not read.  Per call, whatever the number of active jobs: the
 * single call's nine launches (new keys, rebuild, flag, clear, fill, recompute, flag, clear, fill; blockIdx.y = active
 * job, the rebuild one workgroup per job, all of them side by side), one host-to-device copy of the corrections, a
 * descriptor upload only for a job whose entry changed, no synchronise.  Job j's map -- L0 order, keys, centroids and
 * point counts with the merged voxels; L1 order, children, surfels -- and context j's surfel table afterwards equal
 * the single call's on an identical map, bit for bit.  The contracts are lo_batch_update_maps': enqueues and returns;
 * the contexts must be idle; LO_ERR_STATE while a batch optimize is in flight; LO_ERR_ARG for a null argument or an
 * active job's map that was not created on context j; maps of different capacities may share a batch; single and
 * batched corrections and updates may alternate on one map (wait for the batch stream before the single call:
 * lo_batch_maps_status does); a replaced table is refilled first.  A job whose correction gives a key beyond +-2^20 or
 * overflows a capacity sets its own error bits, which lo_batch_maps_status reports for that job only; a job whose map
 * is empty changes nothing.  No scan is read: a context that has filtered none is fine.  In a KDTree batch the
 * contexts' grids still hold the old centroids: the caller follows with lo_batch_sync_points on the same `active`;
 * this call does not. */
int         lo_batch_apply_transform(lo_batch* b, lo_devmap* const* maps, const unsigned char* active, const float* T);
/* Error bits of all jobs' maps in one copy (synchronises the batch stream): rc[j] (nullable) = LO_OK or
 * LO_ERR_CAPACITY; returns LO_OK when every job is LO_OK, else LO_ERR_CAPACITY (lo_batch_last_error names the first
 * such job, and each such map's lo_devmap_last_error is set).  maps[j] may be NULL for a job that has no map: it
 * reports LO_OK. */
int         lo_batch_maps_status(lo_batch* b, lo_devmap* const* maps, int* rc);
/* RebuildKdTree for the keyframes of a KDTree batch (every context use_surfel_correspondence = 0): for every job j with
 * active[j] != 0, what lo_devmap_sync_points(maps[j]) does -- context j's correspondence grid rebuilt from map j's L0
 * centroids in L0 order -- for all active jobs together on the batch stream, behind a preceding lo_batch_update_maps.
 * Per call, whatever the number of jobs: eight launches (blockIdx.y = active job: the bounds, the clear of the cell
 * counts, the cells and counts, a three-launch exclusive scan into the cell starts, the slot claim and the placement
 * by in-cell rank -- no per-job sort), two host-to-device copies (the jobs' point arrays, then the grids' descriptors)
 * and one device-to-host copy of seven words per job (the six bounds and the raw device count) with the call's one
 * synchronise of the batch stream; the host sizes every grid from them and grows the contexts' buffers.  Context j
 * afterwards holds what the single call gives on an identical map, bit for bit: geometry, point count, cell starts and
 * points (sorted by cell, x fastest, index order inside a cell), no kd visit order, and the next optimize -- single or
 * batched -- searches the new grid.  Distance ties re-run as after the single call (lo_kd_reruns).  The grids are
 * built on the batch stream: before a context is used on its own (lo_icp_optimize, lo_knn_search), wait for it --
 * lo_batch_maps_status does.  LO_ERR_STATE on a surfel-mode batch and while a batch optimize is in flight; LO_ERR_ARG
 * when maps[j] of an active job was not created on context j; LO_ERR_CAPACITY when a job's raw count exceeds its
 * array (lo_batch_last_error names the first such job; its grid is left as it was and the other jobs' grids are still
 * built).  An inactive job's entry, grid and context are not touched. */
int         lo_batch_sync_points(lo_batch* b, lo_devmap* const* maps, const unsigned char* active);

#ifdef __cplusplus
}
#endif
#endif /* LO_MAP_H */
