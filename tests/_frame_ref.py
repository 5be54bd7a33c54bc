"""A model of the reference's frame bookkeeping, shaped like its objects (test infrastructure).

`Frame` is database::LidarFrame's pose part, `Estimator` is processing::Estimator's pose part: the model keeps frame
OBJECTS that point at their previous keyframe, as the reference does, where the library (csrc/lo_frame_state.h) and
oracle.odometry keep a few flat variables.  Agreement between the two shapes is what tests/test_frame_ref.py and the
GPU frame-loop tests assert.

Every SE3 / SO3 operation goes through the primitives that tests/test_oracle.py pins on their own
(oracle.se3_compose, se3_inverse, so3_normalize, keyframe_metrics); nothing here restates an SVD.  The ICP is a
callback ``icp(points, guess12) -> (ok, T12)``: the oracle's ICP, the library's ICP on the GPU, or a scripted list.
Poses are row-major 3x4 float32, flattened to 12.  Line numbers cite the reference: E = src/processing/Estimator.cpp,
F = src/database/LidarFrame.cpp, M = src/util/MathUtils.{h,cpp}.
"""
import numpy as np

import oracle

I12 = np.eye(3, 4, dtype=np.float32).reshape(12)


def _p12(T):
    a = np.asarray(T, np.float32)
    return np.ascontiguousarray(a.reshape(12) if a.size == 12 else a[:3, :4].reshape(12)).copy()


def se3_from_rt(T12):
    """SE3f(Matrix3f, Vector3f) (M .h:116-117): the rotation goes through SO3(Matrix3f), the translation is kept."""
    T = _p12(T12).reshape(3, 4)
    T[:, :3] = oracle.so3_normalize(T[:, :3].reshape(9)).reshape(3, 3)
    return T.reshape(12)


def normalize_rotation(T12):
    """MathUtils::normalize_rotation_matrix on the rotation block (M .cpp:363-388): U V^T of the JacobiSVD with the
    determinant fix -- the very arithmetic of SO3(Matrix3f) (M .cpp:86-99), hence the same pinned primitive."""
    return se3_from_rt(T12)


class Frame:
    def __init__(self):
        self.pose = I12.copy()                 # m_pose (F:25)
        self.relative_pose = I12.copy()        # m_relative_pose (F:26)
        self.previous_keyframe = None          # m_previous_keyframe
        self.keyframe_id = -1                  # F:23: not a keyframe

    def is_keyframe(self):
        return self.keyframe_id >= 0

    def get_stored_pose(self):
        return self.pose

    def get_pose(self):
        if self.is_keyframe():                 # F:115-117
            return self.pose
        if self.previous_keyframe is not None:  # F:120-124, the recursion included
            return oracle.se3_compose(self.previous_keyframe.get_pose(), self.relative_pose)
        return self.pose                       # F:127


class Estimator:
    def __init__(self, kf_dist=1.0, kf_rot=0.3, initial=None):
        self.kf_dist, self.kf_rot = float(kf_dist), float(kf_rot)
        self.initial = I12.copy() if initial is None else _p12(initial)
        self.initialized = False
        self.previous_frame = None
        self.last_keyframe = None
        self.last_keyframe_pose = I12.copy()
        self.velocity = I12.copy()
        self.keyframes = []
        self.next_keyframe_id = 0
        # what the tests read
        self.frames = []                       # every Frame, in order
        self.guesses = []                      # per frame: the guess of E:154 (None where the reference forms none)
        self.velocities = []                   # per frame: m_velocity after the frame
        self.odom_edges = []                   # per keyframe: the edge of E:385-390 (None for the first)
        self.prev_was = []                     # per frame: (previous frame's get_pose(), its get_stored_pose(), is_keyframe)

    # ---- E:137-211
    def process(self, points, icp):
        """One frame -> (pose12, is_keyframe, icp_ok)."""
        cur = Frame()
        self.frames.append(cur)
        if not self.initialized:               # E:137-140 -> initialize_first_frame, E:235-269
            self.velocity = I12.copy()         # E:238
            cur.pose = self.initial.copy()     # E:239
            cur.previous_keyframe = None       # E:243
            cur.relative_pose = I12.copy()     # E:244
            self.guesses.append(None)
            self.prev_was.append(None)
            self.initialized = True            # E:250 / E:268
            if len(points) == 0:               # E:248-252: no keyframe, and m_previous_frame stays unset
                self.velocities.append(self.velocity.copy())
                return cur.pose.copy(), False, True
            self.create_keyframe(cur)          # E:263
            self.previous_frame = cur          # E:265
            self.last_keyframe_pose = cur.pose.copy()   # E:266
            self.velocities.append(self.velocity.copy())
            return cur.pose.copy(), True, True
        if self.last_keyframe is None:         # E:146-149: nothing is tracked, nothing changes
            self.guesses.append(None)
            self.prev_was.append(None)
            self.velocities.append(self.velocity.copy())
            return self.initial.copy(), False, True
        prev = self.previous_frame
        self.prev_was.append((prev.get_pose().copy(), prev.get_stored_pose().copy(), prev.is_keyframe()))
        guess = oracle.se3_compose(prev.get_pose(), self.velocity)          # E:154
        self.guesses.append(guess.copy())
        # estimate_motion_dual_frame, E:271-320
        ok, T = icp(points, se3_from_rt(guess))                             # E:288, E:297-302
        pose = se3_from_rt(T) if ok else guess                              # E:310 / E:304-307
        self.velocity = oracle.se3_compose(oracle.se3_inverse(prev.get_pose()), pose)   # E:177
        self.velocities.append(self.velocity.copy())
        cur.pose = _p12(pose)                                               # E:181
        cur.previous_keyframe = self.last_keyframe                          # E:187
        cur.relative_pose = oracle.se3_compose(                             # E:189-190
            oracle.se3_inverse(self.last_keyframe.get_stored_pose()), pose)
        kf = self.should_create_keyframe(pose)                              # E:198
        if kf:
            self.create_keyframe(cur)                                       # E:200
        self.previous_frame = cur                                           # E:211
        return cur.pose.copy(), kf, bool(ok)

    # ---- E:349-368
    def should_create_keyframe(self, pose):
        if not self.keyframes:                 # E:351-353
            return True
        d, a = oracle.keyframe_metrics(self.last_keyframe_pose, pose)       # E:356-360
        return d > self.kf_dist or a > self.kf_rot                          # E:367

    # ---- E:370-428, E:493-494 (the map and the loop detector are the caller's)
    def create_keyframe(self, frame):
        frame.keyframe_id = self.next_keyframe_id                           # E:376: first, so get_pose() below is
        self.next_keyframe_id += 1                                          # the frame's stored pose
        if self.keyframes:
            raw = oracle.se3_compose(oracle.se3_inverse(self.keyframes[-1].get_pose()), frame.get_pose())   # E:381-385
            rel = se3_from_rt(normalize_rotation(raw))                      # E:388-390
            frame.relative_pose = rel                                       # E:392
            self.odom_edges.append(rel.copy())                              # E:401-408
        else:
            frame.relative_pose = I12.copy()                                # E:412
            self.odom_edges.append(None)                                    # E:417-420: the prior instead
        self.keyframes.append(frame)                                        # E:427
        self.last_keyframe = frame                                          # E:493
        self.last_keyframe_pose = frame.get_pose().copy()                   # E:494

    # ---- the pose part of apply_pending_pgo_result_if_available, E:1139-1194, and propagate_poses_after_pgo,
    # E:1196-1225.  Keyframes get set_pose; m_previous_frame, m_velocity and m_last_keyframe_pose are not touched.
    # A non-keyframe's get_pose() goes through its previous keyframe, so it moves with the keyframe all the same.
    def apply_correction(self, new_keyframe_poses):
        """new_keyframe_poses: poses of keyframes 0..n-1 (n <= len(keyframes)); later keyframes are propagated."""
        n = len(new_keyframe_poses)
        assert 1 <= n <= len(self.keyframes)
        for kf, P in zip(self.keyframes[:n], new_keyframe_poses):           # E:1161-1169
            kf.pose = _p12(P)
        acc = self.keyframes[n - 1].get_pose()                              # E:1207
        for kf in self.keyframes[n:]:                                       # E:1215-1218
            acc = oracle.se3_compose(acc, kf.relative_pose)
            kf.pose = acc.copy()

    def keyframe_poses(self):
        return [kf.get_pose().copy() for kf in self.keyframes]


def oracle_icp(vmap, kdtree=False):
    """The callback on the oracle's ICP over `vmap` (an oracle.VoxelMap the caller updates at keyframes)."""
    def icp(points, guess12):
        ok, T, _, _ = oracle.icp_optimize(vmap, points, guess12, kdtree=kdtree)
        return ok, T
    return icp


def run_oracle(raw_scans, initial=None, stride=8, voxel=0.5, map_voxel=0.5, max_range=100.0, kdtree=False):
    """The model driven by the oracle's ICP on the oracle's VoxelMap: the frame loop without loop closure.
    Returns (estimator, poses (n, 12), keyframe flags)."""
    est = Estimator(initial=initial)
    vmap = oracle.VoxelMap(map_voxel, 3, 0.1, not kdtree)                   # SetComputeSurfels (E:79)
    icp = oracle_icp(vmap, kdtree)
    poses, flags = [], []
    for raw in raw_scans:
        pts = oracle.voxel_filter(raw, voxel, stride)
        pose, kf, _ = est.process(pts, icp)
        if kf:                                                              # E:453-457
            vmap.update(oracle.transform_points(pts, pose), pose.reshape(3, 4)[:, 3].astype(np.float64),
                        1.2 * max_range, True)
        poses.append(pose)
        flags.append(kf)
    return est, np.stack(poses), flags


def input_conditions(est):
    """The conditions a sequence must meet to tell the recomposed previous pose from the stored one (asserted on
    the model's run alone).  Returns (frames whose previous frame is a non-keyframe, those among them on which the
    two poses differ in a bit)."""
    non_kf, differ = [], []
    for k, w in enumerate(est.prev_was):
        if w is None:
            continue
        got, stored, is_kf = w
        same = np.array_equal(got.view(np.uint32), stored.view(np.uint32))
        if is_kf:
            assert same, f"frame {k}: a keyframe's get_pose() is its stored pose"
        else:
            non_kf.append(k)
            if not same:
                differ.append(k)
    return non_kf, differ
