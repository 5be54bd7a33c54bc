// lo_frame_state.h — the frame loop's pose bookkeeping, host only (no HIP, no device): what Estimator keeps in
// m_previous_frame, m_last_keyframe, m_last_keyframe_pose, m_velocity and the keyframes' poses, flattened to the few
// values the loop reads.  lo_odometry.cpp holds one lo::FrameState and keeps no pose of its own; tests/test_frame_ref.py
// compiles this header into a host program and compares it with a model of the reference's frame objects.
//
// Why `prev` is not a stored pose.  The reference reads the previous frame through LidarFrame::get_pose()
// (LidarFrame.cpp:113-128), which returns the stored pose only for a keyframe (or a frame without a previous
// keyframe).  For any other frame it RECOMPOSES previous_keyframe->get_pose() * m_relative_pose, where m_relative_pose
// was set to last_keyframe->get_stored_pose().Inverse() * T (Estimator.cpp:186-191).  Inverse and both products
// re-project their rotation through SO3(Matrix3f) (a JacobiSVD, MathUtils.cpp:86-99), so the recomposed pose differs
// from T in the last bits -- and moves with the keyframe when a pose-graph correction moves the keyframe.
#pragma once
#include <cstddef>
#include <vector>

#include "lo_math.h"

namespace lo {

struct FrameState {
    SE3f prev_stored;                 // m_previous_frame->get_stored_pose()
    bool prev_is_kf = false;          // m_previous_frame->is_keyframe()
    bool have_kf = false;             // m_last_keyframe != nullptr
    SE3f kf_pose;                     // m_last_keyframe->get_stored_pose(): its CURRENT pose (a correction moves it)
    SE3f rel;                         // m_previous_frame's m_relative_pose (meaningful when !prev_is_kf && have_kf)
    SE3f velocity;                    // m_velocity
    SE3f last_kf;                     // m_last_keyframe_pose: the keyframe test's copy (:494), never corrected
    bool keep_kf_poses = false;       // loop closure: every keyframe's current pose, keyframe id = index
    std::vector<SE3f> kf_poses;

    // initialize_first_frame (:235-245): the frame takes the initial pose, identity velocity, no previous keyframe
    void init(const SE3f& initial) {
        prev_stored = initial;
        prev_is_kf = false;
        have_kf = false;
        velocity = SE3f();
        rel = SE3f();
    }
    // m_previous_frame->get_pose() (LidarFrame.cpp:113-128)
    SE3f prev_pose() const {
        if (prev_is_kf) return kf_pose;                  // :115-117 (the previous frame IS the last keyframe)
        if (have_kf) return se3_mul(kf_pose, rel);       // :120-124
        return prev_stored;                              // :127
    }
    // T_keyframe_current_guess (Estimator.cpp:154)
    SE3f guess() const { return se3_mul(prev_pose(), velocity); }
    // The tracked frame's pose T (:174-198): velocity (:177), set_pose (:181), set_previous_keyframe / set_relative_pose
    // (:186-191); it becomes the previous frame (:211).  Returns should_create_keyframe(T) (:349-368).
    bool commit(const SE3f& pose, double kf_distance, double kf_rotation) {
        velocity = se3_mul(se3_inv(prev_pose()), pose);
        prev_stored = pose;
        prev_is_kf = false;
        if (have_kf) rel = se3_mul(se3_inv(kf_pose), pose);
        if (!have_kf) return true;                                                    // :351-353
        const float dt[3] = {pose.t[0] - last_kf.t[0], pose.t[1] - last_kf.t[1], pose.t[2] - last_kf.t[2]};
        const float dist = std::sqrt(dot3e(dt[0], dt[1], dt[2], dt[0], dt[1], dt[2]));
        float Rki[3][3], Rkt[3][3], Rrel[3][3], Rrel_p[3][3];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rkt[r][c] = last_kf.R[c][r];
        so3_project_svd(Rkt, Rki);                                                    // SO3::Inverse -> SO3(R^T)
        mul33e(Rki, pose.R, Rrel);
        so3_project_svd(Rrel, Rrel_p);                                                // SO3::operator*
        const double ang = so3_log_norm(Rrel_p);
        return static_cast<double>(dist) > kf_distance || ang > kf_rotation;
    }
    // create_keyframe's pose part (:376-428, :493-494) for the frame just committed (or the first frame) at `pose`,
    // its stored pose.  Returns false for the first keyframe (no edge); otherwise writes the odometry edge the pose
    // graph gets: previous_keyframe->get_pose().Inverse() * pose (:385), its rotation through
    // MathUtils::normalize_rotation_matrix (:388-389, the same U V^T projection) and once more through the
    // SE3f(Matrix3f, Vector3f) constructor (:390, MathUtils.h:116-117).
    bool on_keyframe(const SE3f& pose, SE3f* edge) {
        const bool has_edge = have_kf;
        if (has_edge && edge) {
            const SE3f raw = se3_mul(se3_inv(kf_pose), pose);
            float Rn[3][3];
            so3_project_svd(raw.R, Rn);
            *edge = raw;
            so3_project_svd(Rn, edge->R);
        }
        kf_pose = pose;
        last_kf = pose;
        have_kf = true;
        prev_is_kf = true;
        prev_stored = pose;
        if (keep_kf_poses) kf_poses.push_back(pose);
        return has_edge;
    }
    // apply_pending_pgo_result_if_available's pose part (:1158-1175), applied while the last keyframe is the newest
    // one: every keyframe takes set_pose(optimized).  m_previous_frame, m_velocity and m_last_keyframe_pose are not
    // touched -- but the previous frame's get_pose() goes through the last keyframe's pose, so it moves with it.
    // poses: n = kf_poses.size() current poses in keyframe order.  Returns false (and changes nothing) otherwise.
    bool on_correction(const SE3f* poses, size_t n) {
        if (!keep_kf_poses || n == 0 || n != kf_poses.size()) return false;
        kf_poses.assign(poses, poses + n);
        kf_pose = kf_poses.back();
        if (prev_is_kf) prev_stored = kf_pose;
        return true;
    }
};

}  // namespace lo
