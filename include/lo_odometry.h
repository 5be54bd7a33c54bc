/* lo_odometry.h — the frame loop around the ICP step (the hot path's caller), MI355X device path.
 *
 * Replaces Estimator::process_frame (src/processing/Estimator.cpp:115-233).  Loop closure / PGO is opt-in
 * (lo_odom_enable_loop_closure, below) and off in all odometry parity runs; without it the loop is:
 *   preprocess_frame (:561-589)            -> device FastVoxelFilter (lo_icp_optimize_raw)
 *   first frame (:235-269)                 -> pose = initial pose, create_keyframe
 *   guess = previous_frame->get_pose() * velocity (:154)
 *                                          -> SE3f product with SO3 re-projection (MathUtils.h:144-147).  get_pose()
 *                                             (LidarFrame.cpp:113-128) is the stored pose only for a keyframe; for any
 *                                             other frame it is last_keyframe_pose * relative_pose, recomposed through
 *                                             two more re-projections (relative_pose = last_keyframe_pose^-1 * pose,
 *                                             :186-191), so it is not the stored pose to the bit
 *   estimate_motion_dual_frame (:271-320) -> lo_icp_optimize_raw on the device map; failure keeps the guess
 *   velocity = previous_frame->get_pose()^-1 * pose (:177), the same recomposed previous pose
 *   should_create_keyframe (:349-368)      -> |dt| > keyframe_distance or |Log(R_kf^-1 R)| > keyframe_rotation
 *   create_keyframe (:370-530)             -> VoxelMap::UpdateVoxelMap(world cloud, position, 1.2 * max_range):
 *                                             surfel mode: the device-resident map (lo_devmap_update_from_scan,
 *                                             lo_map.h), which patches the context's table in place -- ten kernel
 *                                             launches, no host sync (LO_HOST_MAP=1: the host map + patch sync);
 *                                             KDTree mode: the host map + RebuildKdTree upload
 */
#ifndef LO_ODOMETRY_H
#define LO_ODOMETRY_H

#include <stddef.h>

#include "lo_icp.h"
#include "lo_iris.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    lo_config icp;                 /* ICP + PKO + map geometry (voxel_size = map voxel, hierarchy_factor) */
    int    point_stride;           /* point_cloud.point_stride: 8 (kitti.yaml:18) */
    float  filter_voxel_size;      /* point_cloud.voxel_size: 0.5 (kitti.yaml:17) */
    double max_range;              /* point_cloud.max_range: 100 (kitti.yaml:20); map radius = 1.2 x */
    double keyframe_distance;      /* estimator.keyframe_distance_threshold: 1.0 m (kitti.yaml:55) */
    double keyframe_rotation;      /* estimator.keyframe_rotation_threshold: 0.3 rad (kitti.yaml:56) */
    float  planarity_threshold;    /* surfel planarity: 0.1 (kitti.yaml:22) */
} lo_odom_config;

typedef struct {
    int    status;                 /* LO_OK, or LO_INSUFFICIENT when ICP failed and the guess was kept */
    int    keyframe;               /* 1 if this frame became a keyframe (map updated) */
    int    icp_iterations;
    int    n_filtered;             /* feature cloud size */
    int    n_corr;
    double device_ms;              /* preprocessing + ICP on the device (HIP events) */
    double map_ms;                 /* keyframe map update (host wall time: enqueue only with the device map), 0 otherwise */
    float  guess[12];              /* debug: the guess of :154 this frame started from (row-major 3x4), before the
                                      re-projection of :288; the returned pose for the first frame and the early return */
} lo_odom_frame;

typedef struct lo_odometry lo_odometry;

void          lo_odom_config_default_kitti(lo_odom_config* cfg);
/* The device map holds up to 2^21 L0 voxels (LO_DEVMAP_MAX_L0 in the environment overrides it).  An update that
 * overflows a capacity aborts and sets the map's error bits; lo_odom_process reports it (LO_ERR_CAPACITY) at the first
 * frame after that keyframe, read without a stream sync (lo_devmap_status_async / _poll). */
lo_odometry*  lo_odom_create(const lo_odom_config* cfg, int device, int* err);
void          lo_odom_destroy(lo_odometry* o);
const char*   lo_odom_last_error(const lo_odometry* o);
/* Pose of the first frame (LidarFrame::get_initial_pose); identity by default. */
int           lo_odom_set_initial_pose(lo_odometry* o, const float T[12]);
/* The frame loop's ICP arithmetic mode (lo_set_exact on its context): 1 = reference-exact, the default; 0 = the
 * opt-in fast mode (not parity-safe, see lo_set_exact).  Feature clouds whose bound ceil(n_raw / point_stride) exceeds
 * 16384 take the exact mode's device radix-sort path for the iteration-0 scale (slower, same bits). */
int           lo_odom_set_exact(lo_odometry* o, int enable);
/* One raw scan (AoS float3, host memory) -> its world pose (row-major 3x4).  Returns LO_OK / LO_INSUFFICIENT
 * (the guess was kept, as :304-307) or a negative error. */
int           lo_odom_process(lo_odometry* o, const float* raw_xyz, size_t n, float T_out[12], lo_odom_frame* info);
/* Wait for the last keyframe's map update and report its status: LO_ERR_CAPACITY if it overflowed (an overflow at the
 * final keyframe of a run is otherwise never read, since no later frame polls it).  Call before trusting the map after
 * the last frame; lo_odom_destroy does not report. */
int           lo_odom_flush(lo_odometry* o);
size_t        lo_odom_keyframe_count(const lo_odometry* o);
size_t        lo_odom_map_surfels(const lo_odometry* o);
int           lo_odom_kd_reruns(const lo_odometry* o);   /* lo_kd_reruns of the loop's context (KDTree mode) */

/* ---- loop closure in the frame loop (opt-in) ----
 * The reference's SLAM back end around the frame loop: create_keyframe's loop bookkeeping (Estimator.cpp:370-530),
 * run_pgo_for_loop (:959-1137) and apply_pending_pgo_result_if_available (:1139-1194), joined from the library's own
 * pieces: lo_iris (candidates), lo_icp_optimize_loop_dev (verification, on the keyframe clouds where they already
 * are: the context's filtered scan and the lo_gmap arena), lo_pgo (the graph), lo_devmap_apply_transform (the map)
 * and lo_gmap (the corrected global map).
 *
 * At every keyframe, after the map update: the feature cloud is stored (lo_gmap_add_from_scan), the pose graph is
 * extended (first keyframe: prior; later: odometry factor with relative = prev_keyframe_pose^-1 * pose, SE3f algebra,
 * the previous keyframe's CURRENT pose, its rotation normalised and re-projected as Estimator.cpp:385-390 does), and when keyframe_id - last_successful_loop_keyframe >= cooldown_keyframes
 * (that counter starts at -1, Estimator.cpp:38) the detector is queried with the device scan, THEN the keyframe is
 * added to it.  The reference adds first and queries afterwards; the order is equivalent because a database entry
 * closer than min_keyframe_gap ids -- the keyframe itself included -- is skipped by the selection, for every
 * min_keyframe_gap >= 1 (lo_odom_enable_loop_closure refuses smaller values).
 * A candidate is verified by the loop ICP at the two keyframes' current poses and accepted when it returns LO_OK and
 * inlier_ratio >= min_inlier_ratio.  Then T_corrected = T_curr * T_rel, constraint = T_matched^-1 * T_corrected,
 * lo_pgo_add_loop_and_optimize(matched, curr, constraint).  On PGO success every keyframe takes its optimized pose;
 * correction = after * before^-1 of the last keyframe moves the map (lo_devmap_apply_transform, then
 * lo_devmap_sync_points in KDTree mode; LO_HOST_MAP=1: lo_voxelmap_apply_transform + lo_map_sync_voxelmap); the
 * previous-frame pose behind the next guess becomes the keyframe's optimized pose (the reference's m_previous_frame
 * IS that keyframe); the stored velocity is kept; the cooldown counter becomes this keyframe's id.
 * The pose should_create_keyframe compares against does NOT move: the reference keeps it as a copy
 * (m_last_keyframe_pose, set at Estimator.cpp:494, read at :356-359) that apply_pending_pgo_result_if_available
 * never touches, so the next keyframe test still measures from the uncorrected keyframe pose.
 *
 * Synchronous by design.  The reference runs detection, loop ICP and PGO on a background thread and applies the
 * result at the start of the first process_frame after the thread finished, so the frame at which a correction lands
 * depends on wall-clock time.  Here everything runs inside the keyframe's own lo_odom_process call and lands before
 * the next frame is tracked -- what the reference does when its thread finishes between two frames.  Runs are
 * therefore reproducible.
 *
 * Without lo_odom_enable_loop_closure the frame loop does exactly what it did: no allocation, launch or sync more. */
typedef struct lo_loop_config {      /* defaults: ConfigUtils.h:117-134 */
    lo_iris_config iris;             /* 0.3f, 50, 10.0f */
    int    cooldown_keyframes;       /* loop_min_keyframe_gap's second use (kitti.yaml:70): 50 */
    float  min_inlier_ratio;         /* 0.3f (Estimator.cpp:1015) */
    double odom_trans_noise, odom_rot_noise, loop_trans_noise, loop_rot_noise;   /* 0.5, 0.5, 1.0, 1.0 */
    size_t max_keyframes;            /* iris database + gmap keyframes (default 4096) */
    size_t max_points;               /* gmap arena, points over all keyframes (default 2^22) */
} lo_loop_config;

/* The last keyframe's loop attempt. */
typedef struct lo_loop_event {
    int    keyframe_id;              /* the keyframe (-1: no keyframe yet) */
    int    queried;                  /* 1: the detector was queried; 0: cooled down */
    int    candidate_id;             /* matched keyframe id, -1: none */
    float  candidate_distance;       /* its iris distance and bias (0 / 0 without a candidate) */
    int    candidate_bias;
    int    icp_status;               /* lo_icp_optimize_loop_dev's return (meaningful with a candidate only) */
    int    icp_iterations;
    float  inlier_ratio;
    int    accepted;                 /* 1: verified, PGO succeeded, poses and map corrected */
    int    pgo_converged;
    int    pgo_iterations;
    float  correction_translation;   /* |t| of the last keyframe's correction, m */
    float  correction_angle;         /* |Log(R)| of it, rad */
    double detect_ms, icp_ms, pgo_ms, map_ms;   /* host wall time of the four stages */
    float  odom_edge[12];            /* debug: the odometry edge handed to the pose graph at this keyframe (row-major
                                        3x4; identity for keyframe 0, which gets the prior instead) */
} lo_loop_event;

void      lo_loop_config_default(lo_loop_config* cfg);
/* Creates the detector, the keyframe store and the pose graph.  Before the first frame, else LO_ERR_STATE (also when
 * already enabled); LO_ERR_ARG for a null pointer, iris.min_keyframe_gap < 1 or a zero capacity. */
int       lo_odom_enable_loop_closure(lo_odometry* o, const lo_loop_config* cfg);
/* LO_ERR_STATE when loop closure is not enabled.  A keyframe that exceeds max_keyframes or max_points makes its
 * lo_odom_process return LO_ERR_CAPACITY (text in lo_odom_last_error). */
int       lo_odom_last_loop(const lo_odometry* o, lo_loop_event* out);
size_t    lo_odom_loop_count(const lo_odometry* o);          /* loops closed */
/* The keyframes' current (corrected) poses in keyframe order; ids / poses_3x4 nullable; returns the keyframe count
 * (at most cap entries are written).  0 when loop closure is not enabled. */
size_t    lo_odom_keyframe_poses(const lo_odometry* o, int* ids, float* poses_3x4, size_t cap);
/* lo_gmap_build of the stored keyframe clouds at those poses; then lo_gmap_download / lo_gmap_save_ply of it
 * (Estimator::save_map_to_ply, Estimator.cpp:1248-1305).  LO_ERR_STATE when loop closure is not enabled. */
int       lo_odom_build_map(lo_odometry* o, float voxel_size, size_t* out_n);
long long lo_odom_map_points(lo_odometry* o, float* out_xyz, size_t cap);
int       lo_odom_save_map_ply(lo_odometry* o, const char* path, float voxel_size);

/* ---- the frame loop for B sequences on one GPU ----
 * lo_odom_process for `count` independent sequences in lockstep, joined from the batch's pieces (lo_icp.h lo_batch_*,
 * lo_map.h lo_batch_update_maps): `count` contexts, one lo_batch, one device map per context (max_l0 L0 voxels each)
 * and one pose bookkeeping per sequence.  Per call: one batched voxel filter (lo_batch_filter_raw_host), every
 * sequence's guess, one batched optimize (lo_batch_optimize_async + lo_batch_result), every sequence's pose update and
 * keyframe test, and one batched map update (lo_batch_update_maps) over the sequences that made a keyframe.  The first
 * call makes every sequence with a non-empty filtered scan a keyframe at its initial pose; a sequence whose first scan
 * filtered to nothing takes lo_odom_process's early return on every later call.  Sequence j's poses, keyframe flags,
 * iteration counts and guesses equal, bit for bit, those of a lo_odometry fed sequence j alone with the same config
 * and mode.  The maps' error bits are read once per call for all sequences, after the next call's ICP result (an
 * aborted update is reported -- LO_ERR_CAPACITY, the call returns before the poses are committed -- at the first call
 * after its keyframe); lo_odom_batch_flush reads them at once.
 * lo_odom_batch_create is surfel mode only: a KDTree config (use_surfel_correspondence = 0) is refused with LO_ERR_ARG
 * and belongs to lo_odom_batch_create_kdtree, which in turn refuses a surfel config with LO_ERR_ARG and is otherwise
 * the same constructor: everything after creation is this one set of calls.  A KDTree loop rebuilds the grids of the
 * sequences that made a keyframe with one lo_batch_sync_points (lo_map.h) directly after their lo_batch_update_maps
 * (RebuildKdTree, Estimator.cpp:460-462), and equals a solo KDTree lo_odometry in the same fields and in lo_kd_reruns.
 * lo_odom_batch_last_error(NULL) says why the calling thread's last create failed.  No loop closure in this
 * loop yet: the batched detector exists (lo_iris_batch.h: the candidates of any subset of sequences in one set of
 * launches), so does the batched loop ICP (lo_icp.h: lo_batch_optimize_loop_dev, the candidates' verification in
 * one lockstep run) and so does the batched map correction (lo_map.h: lo_batch_apply_transform, the corrected
 * sequences' maps moved and rehashed in one set of launches), but none is wired in here yet -- what remains is
 * per-sequence PGO (host code, lo_pgo.h) and the wiring.
 * info[j].device_ms is the whole batch's optimize; info[j].map_ms the batched update's enqueue (KDTree: and the grid
 * build with its synchronise). */
typedef struct lo_odom_batch lo_odom_batch;
lo_odom_batch* lo_odom_batch_create(const lo_odom_config* cfg, int count, int device, size_t max_l0, int* err);
lo_odom_batch* lo_odom_batch_create_kdtree(const lo_odom_config* cfg, int count, int device, size_t max_l0, int* err);
void        lo_odom_batch_destroy(lo_odom_batch* o);
const char* lo_odom_batch_last_error(const lo_odom_batch* o);
int lo_odom_batch_set_initial_pose(lo_odom_batch* o, int job, const float T[12]);
int lo_odom_batch_set_exact(lo_odom_batch* o, int enable);
/* One raw scan per sequence (host memory; pinned memory is read in place) -> one pose per sequence (count x 12) and,
 * nullable, count lo_odom_frame.  Returns LO_OK, or the first negative error; per-job LO_OK / LO_INSUFFICIENT is in
 * info[j].status. */
int lo_odom_batch_process(lo_odom_batch* o, const float* const* raw, const size_t* n, float* T_out, lo_odom_frame* info);
int lo_odom_batch_flush(lo_odom_batch* o);     /* lo_batch_maps_status of the last keyframes */
size_t lo_odom_batch_keyframe_count(const lo_odom_batch* o, int job);
int lo_odom_batch_kd_reruns(const lo_odom_batch* o, int job);   /* lo_kd_reruns of sequence job's context */

#ifdef __cplusplus
}
#endif

#endif
