// lo_odometry.cpp — Estimator::process_frame, with opt-in loop closure / PGO (see include/lo_odometry.h), host C++
// driving the device path: each frame is one lo_icp_optimize_raw call (device voxel filter + GN loop); the
// pose bookkeeping is lo::FrameState (lo_frame_state.h: the reference's frame objects, flattened, on its SE3f algebra of
// lo_math.h) -- this file keeps no pose of its own; keyframes update the voxel map: in surfel mode the
// device-resident map (lo_devmap: the filtered scan never leaves the device, the context's table is patched in
// place, no host sync), in KDTree mode the host VoxelMap (bit-identical UpdateVoxelMap restatement) + re-upload.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/lo_gmap.h"
#include "../../include/lo_map.h"
#include "../../include/lo_odometry.h"
#include "../../include/lo_pgo.h"
#include "lo_ctx_internal.h"
#include "lo_frame_state.h"
#include "lo_math.h"

using lo::SE3f;

struct lo_odometry {
    lo_odom_config cfg{};
    lo_ctx* icp = nullptr;
    lo_voxelmap* map = nullptr;
    lo_devmap* dmap = nullptr;            // surfel mode (LO_HOST_MAP=1: the host map + patch sync instead)
    std::string err;
    bool initialized = false;
    SE3f initial;
    lo::FrameState fs;                    // previous frame, last keyframe, velocity, keyframe poses (loop closure)
    size_t keyframes = 0;
    std::vector<float> feat, world;
    // loop closure (lo_odom_enable_loop_closure); all null / empty otherwise
    bool loop_on = false;
    lo_loop_config lcfg{};
    lo_iris* iris = nullptr;
    lo_gmap* gmap = nullptr;
    lo_pgo* pgo = nullptr;
    int last_loop_kf = -1;                // m_last_successful_loop_keyframe_id (Estimator.cpp:38)
    size_t loops = 0;
    lo_loop_event ev{};
    long long last_nf = 0;                // the current frame's filtered count
};

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// ApplyTransformAndRehash(correction) on whichever map the loop keeps (apply_pending_pgo_result_if_available, step 3)
static int loop_move_map(lo_odometry* o, const SE3f& corr) {
    float T[12];
    lo::se3_to12(corr, T);
    if (o->dmap) {
        int rc = lo_devmap_apply_transform(o->dmap, T);
        if (rc == LO_OK && !o->cfg.icp.use_surfel_correspondence) rc = lo_devmap_sync_points(o->dmap);
        if (rc == LO_OK) rc = lo_devmap_status_async(o->dmap);
        if (rc != LO_OK) o->err = lo_devmap_last_error(o->dmap);
        return rc;
    }
    int rc = lo_voxelmap_apply_transform(o->map, T);
    if (rc == LO_OK) rc = lo_map_sync_voxelmap(o->icp, o->map, nullptr);
    if (rc != LO_OK) o->err = "loop closure: map correction failed";
    return rc;
}

// The loop bookkeeping of one new keyframe (id = its index) at `pose`, after its map update: create_keyframe's PGO /
// detector part (:399-421, :496-517), then -- synchronously -- run_pgo_for_loop and the application of its result.
static int loop_on_keyframe(lo_odometry* o, const SE3f& pose, const SE3f* edge) {
    const std::vector<SE3f>& kf_poses = o->fs.kf_poses;      // this keyframe's pose is already its last entry
    const int id = static_cast<int>(kf_poses.size()) - 1;
    lo_loop_event& ev = o->ev;
    ev = lo_loop_event{};
    ev.keyframe_id = id;
    ev.candidate_id = -1;
    ev.icp_status = LO_INSUFFICIENT;
    lo::se3_to12(edge ? *edge : SE3f(), ev.odom_edge);
    float T[12];
    lo::se3_to12(pose, T);
    int rc = lo_gmap_add_from_scan(o->gmap, id);
    if (rc != LO_OK) { o->err = std::string("loop closure keyframe store: ") + lo_gmap_last_error(o->gmap); return rc; }
    if (!edge) {
        lo_pgo_add_first_keyframe(o->pgo, id, T);
    } else {                                                 // the normalised relative pose (:385-390)
        lo_pgo_add_keyframe_with_odom(o->pgo, id - 1, id, T, ev.odom_edge, o->lcfg.odom_trans_noise,
                                      o->lcfg.odom_rot_noise);
    }
    const size_t n_curr = static_cast<size_t>(std::max<long long>(o->last_nf, 0));
    const float* d_curr = nullptr;
    const int* d_n = nullptr;
    if (lo::ctx_filtered_device(o->icp, &d_curr, &d_n) != LO_OK) { o->err = lo_last_error(o->icp); return LO_ERR_STATE; }
    lo_iris_candidate cand{};
    bool have = false;
    if (id - o->last_loop_kf >= o->lcfg.cooldown_keyframes) {
        const auto t0 = std::chrono::steady_clock::now();
        ev.queried = 1;
        rc = lo_iris_detect(o->iris, &o->lcfg.iris, id, pose.t, d_curr, n_curr, 1, &cand);
        ev.detect_ms = ms_since(t0);
        if (rc < 0) { o->err = std::string("loop detector: ") + lo_iris_last_error(o->iris); return rc; }
        have = rc == LO_OK;
    }
    rc = lo_iris_add_from_scan(o->iris, id, pose.t);        // (LO_INSUFFICIENT: an empty cloud is not added)
    if (rc < 0) { o->err = std::string("loop detector: ") + lo_iris_last_error(o->iris); return rc; }
    if (!have) return LO_OK;
    ev.candidate_id = static_cast<int>(cand.match_keyframe_id);
    ev.candidate_distance = cand.distance;
    ev.candidate_bias = cand.bias;
    const int mid = ev.candidate_id;
    if (mid < 0 || mid >= id) { o->err = "loop detector: candidate id out of range"; return LO_ERR_STATE; }
    const float* d_m = nullptr;
    size_t n_m = 0;
    rc = lo_gmap_keyframe_points(o->gmap, static_cast<size_t>(mid), nullptr, &d_m, &n_m);
    if (rc != LO_OK) { o->err = lo_gmap_last_error(o->gmap); return rc; }
    if (n_m == 0 || n_curr == 0) return LO_OK;               // "Empty feature clouds for loop" (:989-995)
    float Tm[12], Trel[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    lo::se3_to12(kf_poses[mid], Tm);
    lo_stats st{};
    float inl = 0.0f;
    const auto t1 = std::chrono::steady_clock::now();
    rc = lo_icp_optimize_loop_dev(o->icp, d_curr, n_curr, T, d_m, n_m, Tm, Trel, &inl, nullptr, &st);
    ev.icp_ms = ms_since(t1);
    if (rc < 0) { o->err = lo_last_error(o->icp); return rc; }
    ev.icp_status = rc;
    ev.icp_iterations = st.iterations;
    ev.inlier_ratio = st.converged ? inl : 0.0f;
    if (rc != LO_OK || inl < o->lcfg.min_inlier_ratio) return LO_OK;          // :1008-1020
    const SE3f corrected = lo::se3_mul(pose, lo::se3_from12(Trel));            // :1027
    float con[12];
    lo::se3_to12(lo::se3_mul(lo::se3_inv(kf_poses[mid]), corrected), con);  // :1039
    const auto t2 = std::chrono::steady_clock::now();
    const int ok = lo_pgo_add_loop_and_optimize(o->pgo, mid, id, con, o->lcfg.loop_trans_noise, o->lcfg.loop_rot_noise,
                                                &ev.pgo_converged, &ev.pgo_iterations, nullptr);
    ev.pgo_ms = ms_since(t2);
    if (ok != 1) return LO_OK;                                                 // "PGO failed!" (:1080-1083)
    // apply_pending_pgo_result_if_available, here and now: poses, map, cooldown
    const SE3f before = kf_poses.back();
    std::vector<SE3f> opt(kf_poses);
    for (int k = 0; k <= id; ++k) {
        float P[12];
        if (lo_pgo_get_optimized_pose(o->pgo, k, P) == 1) opt[k] = lo::se3_from12(P);
    }
    o->fs.on_correction(opt.data(), opt.size());             // :1158-1175
    const SE3f corr = lo::se3_mul(kf_poses.back(), lo::se3_inv(before));       // :1121
    ev.correction_translation = std::sqrt(lo::dot3e(corr.t[0], corr.t[1], corr.t[2], corr.t[0], corr.t[1], corr.t[2]));
    ev.correction_angle = lo::so3_log_norm(corr.R);
    const auto t3 = std::chrono::steady_clock::now();
    rc = loop_move_map(o, corr);
    ev.map_ms = ms_since(t3);
    if (rc != LO_OK) return rc;
    // (m_previous_frame is this keyframe, so the next guess starts from its corrected pose; m_velocity is kept;
    // m_last_keyframe_pose, FrameState::last_kf, is NOT moved (:494))
    o->last_loop_kf = id;
    ++o->loops;
    ev.accepted = 1;
    return LO_OK;
}

static int create_keyframe(lo_odometry* o, const SE3f& pose, lo_odom_frame* info) {
    // create_keyframe (:370-530): world feature cloud -> UpdateVoxelMap(cloud, position, 1.2 max_range) -> device
    const auto t0 = std::chrono::steady_clock::now();
    if (o->dmap) {
        float T[12];
        lo::se3_to12(pose, T);
        int rc = lo_devmap_update_from_scan(o->dmap, T, o->cfg.max_range * 1.2);
        if (rc == LO_OK && !o->cfg.icp.use_surfel_correspondence)
            rc = lo_devmap_sync_points(o->dmap);         // RebuildKdTree (Estimator.cpp:460-462) on the device
        if (rc != LO_OK) { o->err = lo_devmap_last_error(o->dmap); return rc; }
        ++o->keyframes;
        // the map's error bits (an update that overflowed a capacity aborted; tracking would go on against a stale
        // map): copied back behind the update without a sync, read after the next frame's ICP (lo_odom_process)
        if ((rc = lo_devmap_status_async(o->dmap)) != LO_OK) {
            o->err = lo_devmap_last_error(o->dmap);
            return rc;
        }
        if (info) {
            info->keyframe = 1;
            info->map_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        SE3f edge;
        const bool has_edge = o->fs.on_keyframe(pose, &edge);
        return o->loop_on ? loop_on_keyframe(o, pose, has_edge ? &edge : nullptr) : LO_OK;
    }
    const long long n = lo_filtered_points(o->icp, nullptr, 0);
    if (n < 0) { o->err = lo_last_error(o->icp); return static_cast<int>(n); }
    o->feat.resize(3 * static_cast<size_t>(std::max<long long>(n, 1)));
    lo_filtered_points(o->icp, o->feat.data(), static_cast<size_t>(n));
    o->world.resize(o->feat.size());
    lo::transform_points(pose, o->feat.data(), static_cast<size_t>(n), o->world.data());   // feature_cloud_global
    const double sensor[3] = {pose.t[0], pose.t[1], pose.t[2]};                          // Vector3f -> Vector3d
    int rc = lo_voxelmap_update(o->map, o->world.data(), static_cast<size_t>(n), sensor, o->cfg.max_range * 1.2, 1);
    if (rc == LO_OK) rc = lo_map_sync_voxelmap(o->icp, o->map, nullptr);                 // patch (+ RebuildKdTree)
    if (rc != LO_OK) { o->err = "keyframe map update failed"; return rc; }
    ++o->keyframes;
    if (info) {
        info->keyframe = 1;
        info->map_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    SE3f edge;
    const bool has_edge = o->fs.on_keyframe(pose, &edge);
    return o->loop_on ? loop_on_keyframe(o, pose, has_edge ? &edge : nullptr) : LO_OK;
}

extern "C" {

void lo_odom_config_default_kitti(lo_odom_config* c) {
    std::memset(c, 0, sizeof(*c));
    lo_config_default_kitti(&c->icp);
    c->point_stride = 8;
    c->filter_voxel_size = 0.5f;
    c->max_range = 100.0;
    c->keyframe_distance = 1.0;
    c->keyframe_rotation = 0.3;
    c->planarity_threshold = 0.1f;
}

lo_odometry* lo_odom_create(const lo_odom_config* cfg, int device, int* err) {
    if (!cfg || cfg->point_stride < 1 || !(cfg->filter_voxel_size > 0.0f)) { if (err) *err = LO_ERR_ARG; return nullptr; }
    lo_odometry* o = new (std::nothrow) lo_odometry();
    if (!o) { if (err) *err = LO_ERR_ARG; return nullptr; }
    o->cfg = *cfg;
    o->icp = lo_create(&cfg->icp, device, err);
    if (!o->icp) { delete o; return nullptr; }
    o->map = lo_voxelmap_create(cfg->icp.voxel_size, cfg->icp.hierarchy_factor, cfg->planarity_threshold,
                                cfg->icp.use_surfel_correspondence ? 1 : 0);   // SetComputeSurfels (Estimator.cpp:79)
    if (!o->map) { lo_destroy(o->icp); delete o; if (err) *err = LO_ERR_ARG; return nullptr; }
    if (cfg->icp.use_surfel_correspondence) lo_voxelmap_set_device_fit(o->map, 1);   // refits run in the sync's patch
    const char* hm = std::getenv("LO_HOST_MAP");
    if (!(hm && std::atoi(hm))) {                        // both correspondence modes (KDTree: lo_devmap_sync_points)
        int e = LO_OK;
        size_t max_l0 = size_t(1) << 21;                                   // LO_DEVMAP_MAX_L0: capacity override
        if (const char* cap = std::getenv("LO_DEVMAP_MAX_L0"); cap && std::atoll(cap) > 0) max_l0 = std::atoll(cap);
        o->dmap = lo_devmap_create(o->icp, cfg->icp.voxel_size, cfg->icp.hierarchy_factor, cfg->planarity_threshold,
                                   max_l0, static_cast<size_t>(std::max(cfg->icp.max_points, 16)), &e);
        if (!o->dmap) { lo_voxelmap_destroy(o->map); lo_destroy(o->icp); delete o; if (err) *err = e; return nullptr; }
    }
    if (err) *err = LO_OK;
    return o;
}

void lo_odom_destroy(lo_odometry* o) {
    if (!o) return;
    lo_iris_destroy(o->iris);                            // the three loop-closure handles go before their context
    lo_gmap_destroy(o->gmap);
    lo_pgo_destroy(o->pgo);
    lo_devmap_destroy(o->dmap);
    lo_voxelmap_destroy(o->map);
    lo_destroy(o->icp);
    delete o;
}

const char* lo_odom_last_error(const lo_odometry* o) { return o ? o->err.c_str() : "null odometry"; }

int lo_odom_set_initial_pose(lo_odometry* o, const float T[12]) {
    if (!o || !T) return LO_ERR_ARG;
    o->initial = lo::se3_from12(T);
    return LO_OK;
}

int lo_odom_set_exact(lo_odometry* o, int enable) {
    if (!o) return LO_ERR_ARG;
    return lo_set_exact(o->icp, enable);
}

int lo_odom_process(lo_odometry* o, const float* raw, size_t n, float T_out[12], lo_odom_frame* info) {
    if (!o || !T_out || (n > 0 && !raw)) return LO_ERR_ARG;
    lo_odom_frame local{};
    lo_odom_frame* fi = info ? info : &local;
    std::memset(fi, 0, sizeof(*fi));
    const int stride = o->cfg.point_stride;
    const float voxel = o->cfg.filter_voxel_size;
    if (!o->initialized) {                                                    // initialize_first_frame (:235-269)
        float tmp[12];
        lo::se3_to12(o->initial, tmp);
        const long long nf = lo_voxel_filter_gpu(o->icp, raw, n, voxel, stride, nullptr, 0);
        if (nf < 0) { o->err = lo_last_error(o->icp); return static_cast<int>(nf); }
        fi->n_filtered = static_cast<int>(nf);
        o->last_nf = nf;
        o->fs.init(o->initial);
        lo::se3_to12(o->initial, fi->guess);
        if (nf > 0) {
            const int rc = create_keyframe(o, o->initial, fi);
            if (rc != LO_OK) return rc;
        }
        o->initialized = true;
        std::memcpy(T_out, tmp, sizeof(tmp));
        fi->status = LO_OK;
        return LO_OK;
    }
    if (o->keyframes == 0) {
        // the first frame filtered to nothing: the reference made no keyframe and every later frame returns at
        // "No keyframe available" (Estimator.cpp:140-144) without ICP, pose update or keyframe test
        lo::se3_to12(o->fs.prev_pose(), T_out);
        std::memcpy(fi->guess, T_out, sizeof(fi->guess));
        fi->status = LO_OK;
        return LO_OK;
    }
    // :154: m_previous_frame->get_pose() * m_velocity.  get_pose() is the stored pose only when the previous frame is a
    // keyframe; otherwise it is recomposed from the last keyframe's pose and the frame's relative pose
    // (LidarFrame.cpp:113-128; lo_frame_state.h), which is not the stored pose to the bit
    const SE3f guess = o->fs.guess();
    lo::se3_to12(guess, fi->guess);
    // estimate_motion_dual_frame hands optimize SE3f(guess.R, guess.t), i.e. SO3(R) re-projected (:284), and
    // wraps the result the same way (:308); on failure it returns the guess itself (:304-307)
    SE3f g_in = guess;
    lo::so3_project_svd(guess.R, g_in.R);
    float g12[12], p12[12];
    lo::se3_to12(g_in, g12);
    lo_iter_log logs[LO_MAX_ITERS];
    lo_stats st{};
    int rc = lo_icp_optimize_raw(o->icp, raw, n, stride, voxel, g12, p12, logs, &st);
    if (rc < 0) { o->err = lo_last_error(o->icp); return rc; }
    if (o->dmap) {      // the last keyframe's map update: the ICP's sync has drained it (same stream), so no wait here
        const int mrc = lo_devmap_status_poll(o->dmap);
        if (mrc != LO_OK) { o->err = lo_devmap_last_error(o->dmap); return mrc; }
    }
    fi->status = rc;
    fi->icp_iterations = st.iterations;
    fi->n_corr = st.n_corr;
    fi->device_ms = st.gpu_ms;
    const long long nf = lo_filtered_points(o->icp, nullptr, 0);
    fi->n_filtered = static_cast<int>(nf > 0 ? nf : 0);
    o->last_nf = nf;
    SE3f pose = guess;
    if (rc == LO_OK) {
        const SE3f r = lo::se3_from12(p12);
        pose = r;
        lo::so3_project_svd(r.R, pose.R);
    }
    lo::se3_to12(pose, p12);
    // :177 velocity = m_previous_frame->get_pose().Inverse() * pose (the same recomposed previous pose), :181-191 the
    // frame's stored and relative pose, :198 should_create_keyframe (:349-368)
    if (o->fs.commit(pose, o->cfg.keyframe_distance, o->cfg.keyframe_rotation)) {
        const int krc = create_keyframe(o, pose, fi);       // (a closed loop moves the keyframe, not this frame's pose)
        if (krc != LO_OK) return krc;
    }
    std::memcpy(T_out, p12, sizeof(p12));
    return rc;
}

int lo_odom_flush(lo_odometry* o) {
    if (!o) return LO_ERR_ARG;
    if (!o->dmap) return LO_OK;                          // the host map reports inside lo_voxelmap_update
    const int rc = lo_devmap_status(o->dmap);            // synchronous: the last update's error bits
    if (rc != LO_OK) o->err = lo_devmap_last_error(o->dmap);
    return rc;
}

void lo_loop_config_default(lo_loop_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    lo_iris_config_default(&c->iris);
    c->cooldown_keyframes = 50;
    c->min_inlier_ratio = 0.3f;
    c->odom_trans_noise = 0.5;
    c->odom_rot_noise = 0.5;
    c->loop_trans_noise = 1.0;
    c->loop_rot_noise = 1.0;
    c->max_keyframes = 4096;
    c->max_points = size_t(1) << 22;
}

int lo_odom_enable_loop_closure(lo_odometry* o, const lo_loop_config* cfg) {
    if (!o || !cfg) return LO_ERR_ARG;
    if (cfg->iris.min_keyframe_gap < 1 || cfg->max_keyframes < 1 || cfg->max_points < 1) {
        o->err = "loop closure: min_keyframe_gap, max_keyframes and max_points must be >= 1";
        return LO_ERR_ARG;
    }
    if (o->initialized || o->loop_on) { o->err = "loop closure is enabled once, before the first frame"; return LO_ERR_STATE; }
    int e = LO_OK;
    lo_iris* iris = lo_iris_create(o->icp, cfg->max_keyframes, &e);
    lo_gmap* gmap = iris ? lo_gmap_create(o->icp, cfg->max_points, cfg->max_keyframes, &e) : nullptr;
    lo_pgo* pgo = gmap ? lo_pgo_create() : nullptr;
    if (!pgo) {
        lo_gmap_destroy(gmap);
        lo_iris_destroy(iris);
        o->err = "loop closure: allocation failed";
        return e != LO_OK ? e : LO_ERR_HIP;
    }
    o->iris = iris;
    o->gmap = gmap;
    o->pgo = pgo;
    o->lcfg = *cfg;
    o->ev = lo_loop_event{};
    o->ev.keyframe_id = -1;
    o->ev.candidate_id = -1;
    o->loop_on = true;
    o->fs.keep_kf_poses = true;
    return LO_OK;
}

int lo_odom_last_loop(const lo_odometry* o, lo_loop_event* out) {
    if (!o || !out) return LO_ERR_ARG;
    if (!o->loop_on) return LO_ERR_STATE;
    *out = o->ev;
    return LO_OK;
}

size_t lo_odom_loop_count(const lo_odometry* o) { return o ? o->loops : 0; }

size_t lo_odom_keyframe_poses(const lo_odometry* o, int* ids, float* poses, size_t cap) {
    if (!o) return 0;
    const size_t n = o->fs.kf_poses.size();
    for (size_t k = 0; k < n && k < cap; ++k) {
        if (ids) ids[k] = static_cast<int>(k);
        if (poses) lo::se3_to12(o->fs.kf_poses[k], poses + 12 * k);
    }
    return n;
}

int lo_odom_build_map(lo_odometry* o, float voxel_size, size_t* out_n) {
    if (!o) return LO_ERR_ARG;
    if (!o->loop_on) { o->err = "loop closure is not enabled"; return LO_ERR_STATE; }
    std::vector<float> P(12 * std::max<size_t>(o->fs.kf_poses.size(), 1));
    for (size_t k = 0; k < o->fs.kf_poses.size(); ++k) lo::se3_to12(o->fs.kf_poses[k], P.data() + 12 * k);
    const int rc = lo_gmap_build(o->gmap, P.data(), o->fs.kf_poses.size(), voxel_size, out_n);
    if (rc < 0) o->err = lo_gmap_last_error(o->gmap);
    return rc;
}

long long lo_odom_map_points(lo_odometry* o, float* out, size_t cap) {
    if (!o) return LO_ERR_ARG;
    if (!o->loop_on) { o->err = "loop closure is not enabled"; return LO_ERR_STATE; }
    const long long k = lo_gmap_download(o->gmap, out, cap);
    if (k < 0) o->err = lo_gmap_last_error(o->gmap);
    return k;
}

int lo_odom_save_map_ply(lo_odometry* o, const char* path, float voxel_size) {
    if (!o || !path) return LO_ERR_ARG;
    int rc = lo_odom_build_map(o, voxel_size, nullptr);
    if (rc != LO_OK) return rc;                          // (LO_INSUFFICIENT: nothing stored, nothing written)
    rc = lo_gmap_save_ply(o->gmap, path);
    if (rc < 0) o->err = lo_gmap_last_error(o->gmap);
    return rc;
}

size_t lo_odom_keyframe_count(const lo_odometry* o) { return o ? o->keyframes : 0; }
int lo_odom_kd_reruns(const lo_odometry* o) { return o ? lo_kd_reruns(o->icp) : -1; }
size_t lo_odom_map_surfels(const lo_odometry* o) {
    if (!o) return 0;
    if (o->dmap) {
        size_t c[4] = {0, 0, 0, 0};
        lo_devmap_counts(o->dmap, c);
        return c[2];
    }
    return lo_voxelmap_surfel_count(o->map);
}

}  // extern "C"

// ================================================================================================== B sequences
// lo_odom_batch_*: lo_odom_process for `count` sequences in lockstep (either correspondence mode, no loop closure),
// joined from the batch's pieces: one batched filter, one batched optimize and one batched map update (KDTree mode: and
// one batched grid build) per call, and per job the same
// lo::FrameState bookkeeping on the same values -- so job j's poses, keyframes, iterations and guesses are those of a
// lo_odometry fed sequence j alone.
struct lo_odom_batch {
    lo_odom_config cfg{};
    int count = 0;
    std::vector<lo_ctx*> ctx;
    lo_batch* batch = nullptr;
    std::vector<lo_devmap*> maps;
    std::vector<lo::FrameState> fs;
    std::vector<SE3f> initial, pose;
    std::vector<size_t> keyframes;
    bool initialized = false;
    bool status_due = false;              // keyframes were enqueued whose error bits nobody has read yet
    std::string err;
    std::vector<size_t> nf, counts;
    std::vector<float> guess12, kf12;
    std::vector<lo_batch_rec> recs;
    std::vector<unsigned char> active, early;
};

static thread_local std::string g_odom_batch_create_err;   // why the calling thread's last create failed

// create_keyframe for the jobs flagged in o->active at o->pose: one batched map update, then each job's pose part
static int batch_keyframes(lo_odom_batch* o, lo_odom_frame* info) {
    bool any = false;
    for (int j = 0; j < o->count; ++j) {
        if (!o->active[j]) continue;
        any = true;
        lo::se3_to12(o->pose[j], o->kf12.data() + 12 * j);
    }
    if (!any) return LO_OK;
    const auto t0 = std::chrono::steady_clock::now();
    int rc = lo_batch_update_maps(o->batch, o->maps.data(), o->active.data(), o->kf12.data(), o->cfg.max_range * 1.2);
    if (rc != LO_OK) { o->err = std::string("keyframe map update: ") + lo_batch_last_error(o->batch); return rc; }
    if (!o->cfg.icp.use_surfel_correspondence) {             // RebuildKdTree (Estimator.cpp:460-462) for the same jobs
        rc = lo_batch_sync_points(o->batch, o->maps.data(), o->active.data());
        if (rc != LO_OK) { o->err = std::string("keyframe grid build: ") + lo_batch_last_error(o->batch); return rc; }
    }
    const double ms = ms_since(t0);
    o->status_due = true;
    for (int j = 0; j < o->count; ++j) {
        if (!o->active[j]) continue;
        ++o->keyframes[j];
        if (info) { info[j].keyframe = 1; info[j].map_ms = ms; }
        o->fs[j].on_keyframe(o->pose[j], nullptr);
    }
    return LO_OK;
}

// the error bits of the keyframes enqueued by the previous call(s), all jobs in one copy
static int batch_map_status(lo_odom_batch* o) {
    if (!o->status_due) return LO_OK;
    o->status_due = false;
    const int rc = lo_batch_maps_status(o->batch, o->maps.data(), nullptr);
    if (rc != LO_OK) o->err = std::string("device map: ") + lo_batch_last_error(o->batch);
    return rc;
}

// lo_odom_batch_create (kdtree = false) and lo_odom_batch_create_kdtree (true): one constructor, the config's
// correspondence mode checked against the entry point's
static lo_odom_batch* odom_batch_create(const lo_odom_config* cfg, int count, int device, size_t max_l0, int* err,
                                        bool kdtree) {
    const char* who = kdtree ? "lo_odom_batch_create_kdtree" : "lo_odom_batch_create";
    auto fail = [&](int rc, const std::string& msg, lo_odom_batch* o) -> lo_odom_batch* {
        g_odom_batch_create_err = msg;
        std::fprintf(stderr, "%s: %s\n", who, msg.c_str());
        lo_odom_batch_destroy(o);
        if (err) *err = rc;
        return nullptr;
    };
    if (!cfg || count < 1 || count > 65535 || cfg->point_stride < 1 || !(cfg->filter_voxel_size > 0.0f))
        return fail(LO_ERR_ARG, "need a config, 1..65535 sequences, point_stride >= 1 and filter_voxel_size > 0", nullptr);
    if (!kdtree && !cfg->icp.use_surfel_correspondence)
        return fail(LO_ERR_ARG, "KDTree-mode config: lo_odom_batch_create is surfel mode only (the KDTree frame loop "
                                "is lo_odom_batch_create_kdtree)", nullptr);
    if (kdtree && cfg->icp.use_surfel_correspondence)
        return fail(LO_ERR_ARG, "surfel-mode config: lo_odom_batch_create_kdtree is KDTree mode only "
                                "(use_surfel_correspondence = 0; the surfel frame loop is lo_odom_batch_create)", nullptr);
    lo_odom_batch* o = new (std::nothrow) lo_odom_batch();
    if (!o) return fail(LO_ERR_ARG, "allocation", nullptr);
    o->cfg = *cfg;
    o->count = count;
    for (int j = 0; j < count; ++j) {
        int e = LO_OK;
        lo_ctx* c = lo_create(&cfg->icp, device, &e);
        if (!c) return fail(e, "lo_create failed for sequence " + std::to_string(j), o);
        o->ctx.push_back(c);
        lo_devmap* m = lo_devmap_create(c, cfg->icp.voxel_size, cfg->icp.hierarchy_factor, cfg->planarity_threshold, max_l0,
                                        static_cast<size_t>(std::max(cfg->icp.max_points, 16)), &e);
        if (!m) return fail(e, "lo_devmap_create failed for sequence " + std::to_string(j), o);
        o->maps.push_back(m);
    }
    int e = LO_OK;
    o->batch = lo_batch_create(o->ctx.data(), count, &e);
    if (!o->batch) return fail(e, "lo_batch_create failed", o);
    const size_t B = static_cast<size_t>(count);
    o->fs.resize(B);
    o->initial.resize(B);
    o->pose.resize(B);
    o->keyframes.assign(B, 0);
    o->nf.assign(B, 0);
    o->counts.assign(B, 0);
    o->guess12.assign(12 * B, 0.0f);
    o->kf12.assign(12 * B, 0.0f);
    o->recs.resize(B);
    o->active.assign(B, 0);
    o->early.assign(B, 0);
    if (err) *err = LO_OK;
    return o;
}

extern "C" {

lo_odom_batch* lo_odom_batch_create(const lo_odom_config* cfg, int count, int device, size_t max_l0, int* err) {
    return odom_batch_create(cfg, count, device, max_l0, err, false);
}

lo_odom_batch* lo_odom_batch_create_kdtree(const lo_odom_config* cfg, int count, int device, size_t max_l0, int* err) {
    return odom_batch_create(cfg, count, device, max_l0, err, true);
}

void lo_odom_batch_destroy(lo_odom_batch* o) {
    if (!o) return;
    lo_batch_destroy(o->batch);                          // (waits for the batch stream, where the map updates run)
    for (lo_devmap* m : o->maps) lo_devmap_destroy(m);
    for (lo_ctx* c : o->ctx) lo_destroy(c);
    delete o;
}

const char* lo_odom_batch_last_error(const lo_odom_batch* o) { return o ? o->err.c_str() : g_odom_batch_create_err.c_str(); }

int lo_odom_batch_set_initial_pose(lo_odom_batch* o, int job, const float T[12]) {
    if (!o || !T || job < 0 || job >= o->count) return LO_ERR_ARG;
    o->initial[job] = lo::se3_from12(T);
    return LO_OK;
}

int lo_odom_batch_set_exact(lo_odom_batch* o, int enable) {
    if (!o) return LO_ERR_ARG;
    for (lo_ctx* c : o->ctx) {
        const int rc = lo_set_exact(c, enable);
        if (rc != LO_OK) { o->err = lo_last_error(c); return rc; }
    }
    return LO_OK;
}

int lo_odom_batch_process(lo_odom_batch* o, const float* const* raw, const size_t* n, float* T_out, lo_odom_frame* info) {
    if (!o) return LO_ERR_ARG;
    if (!raw || !n || !T_out) { o->err = "null argument"; return LO_ERR_ARG; }
    const int B = o->count;
    if (info) std::memset(info, 0, sizeof(lo_odom_frame) * B);
    // preprocess_frame for every sequence (an early-return sequence's scan is filtered too: its count is not reported)
    int rc = lo_batch_filter_raw_host(o->batch, raw, n, o->cfg.point_stride, o->cfg.filter_voxel_size, o->nf.data());
    if (rc != LO_OK) { o->err = lo_batch_last_error(o->batch); return rc; }
    if (!o->initialized) {                                                    // initialize_first_frame (:235-269)
        for (int j = 0; j < B; ++j) {
            o->fs[j].init(o->initial[j]);
            o->pose[j] = o->initial[j];
            o->active[j] = o->nf[j] > 0 ? 1 : 0;
            lo::se3_to12(o->initial[j], T_out + 12 * j);
            if (info) {
                info[j].n_filtered = static_cast<int>(o->nf[j]);
                lo::se3_to12(o->initial[j], info[j].guess);
                info[j].status = LO_OK;
            }
        }
        rc = batch_keyframes(o, info);
        if (rc != LO_OK) return rc;
        o->initialized = true;
        return LO_OK;
    }
    std::vector<SE3f>& guess = o->pose;                   // the guesses until the commit, the poses after it
    for (int j = 0; j < B; ++j) {
        o->early[j] = o->keyframes[j] == 0 ? 1 : 0;
        o->counts[j] = 0;
        if (o->early[j]) {                                // "No keyframe available" (Estimator.cpp:140-144)
            lo::se3_to12(o->fs[j].prev_pose(), o->guess12.data() + 12 * j);
            continue;
        }
        guess[j] = o->fs[j].guess();                      // :154
        if (info) lo::se3_to12(guess[j], info[j].guess);
        SE3f g_in = guess[j];
        lo::so3_project_svd(guess[j].R, g_in.R);          // :284
        lo::se3_to12(g_in, o->guess12.data() + 12 * j);
        o->counts[j] = o->nf[j];
    }
    rc = lo_batch_optimize_async(o->batch, nullptr, o->counts.data(), o->guess12.data());
    if (rc != LO_OK) { o->err = lo_batch_last_error(o->batch); return rc; }
    double ms = 0.0;
    rc = lo_batch_result(o->batch, o->recs.data(), &ms);
    if (rc != LO_OK) { o->err = lo_batch_last_error(o->batch); return rc; }
    // the last keyframes' map updates ran before this frame's ICP on the same stream: their error bits, once per call
    if ((rc = batch_map_status(o)) != LO_OK) return rc;
    for (int j = 0; j < B; ++j) {
        o->active[j] = 0;
        float* To = T_out + 12 * j;
        if (o->early[j]) {
            std::memcpy(To, o->guess12.data() + 12 * j, 12 * sizeof(float));
            if (info) { std::memcpy(info[j].guess, To, sizeof(info[j].guess)); info[j].status = LO_OK; }
            continue;
        }
        const lo_batch_rec& R = o->recs[j];
        if (info) {
            info[j].status = R.status;
            info[j].icp_iterations = R.iterations;
            info[j].n_corr = R.n_corr;
            info[j].device_ms = ms;
            info[j].n_filtered = static_cast<int>(o->nf[j]);
        }
        SE3f pose = guess[j];                             // a failed job keeps the guess (:304-307)
        if (R.status == LO_OK) {
            const SE3f r = lo::se3_from12(R.pose);
            pose = r;
            lo::so3_project_svd(r.R, pose.R);             // :308
        }
        lo::se3_to12(pose, To);
        o->pose[j] = pose;
        o->active[j] = o->fs[j].commit(pose, o->cfg.keyframe_distance, o->cfg.keyframe_rotation) ? 1 : 0;
    }
    return batch_keyframes(o, info);
}

int lo_odom_batch_flush(lo_odom_batch* o) {
    if (!o) return LO_ERR_ARG;
    o->status_due = true;                                 // synchronous: the last updates' error bits, read or not
    return batch_map_status(o);
}

size_t lo_odom_batch_keyframe_count(const lo_odom_batch* o, int job) {
    return (o && job >= 0 && job < o->count) ? o->keyframes[job] : 0;
}

int lo_odom_batch_kd_reruns(const lo_odom_batch* o, int job) {
    return (o && job >= 0 && job < o->count) ? lo_kd_reruns(o->ctx[job]) : -1;
}

}  // extern "C"
