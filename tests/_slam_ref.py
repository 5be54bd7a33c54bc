"""The frame loop with loop closure, assembled by hand from the library's public pieces (test infrastructure for
tests/test_gpu_slam.py): lo_icp_optimize_raw, lo_devmap_update_from_scan, IrisLoopDetector, GlobalMapBuilder,
lo_icp_optimize_loop on HOST clouds, PoseGraphOptimizer and lo_devmap_apply_transform, with the bookkeeping of
include/lo_odometry.h kept here in numpy.  The SE3f products (guess, velocity, relative pose, corrected pose,
constraint, correction) and the keyframe test go through the oracle's restatements of the reference's SE3f algebra
(oracle.se3_compose / se3_inverse / so3_normalize / keyframe_metrics), which the odometry parity tests already hold
equal to the library's lo_math.h.

Deliberately different from lo_odom's own path where the library offers a second one: keyframe clouds are host copies
(the detector, the loop ICP and the map builder read them from the host), so the device-resident path is checked
against the host-input one.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

import oracle
from lidar_odometry_amd import (GlobalMapBuilder, ICPConfig, IrisLoopDetector, IterativeClosestPointOptimizer,
                                LoopClosureConfig, _lib)
from lidar_odometry_amd.pgo import PoseGraphOptimizer
from lidar_odometry_amd.voxelmap import DeviceVoxelMap

I12 = np.eye(3, 4, dtype=np.float32).reshape(12)
STRIDE, VOXEL, MAX_RANGE, KF_DIST, KF_ROT = 8, 0.5, 100.0, 1.0, 0.3      # lo_odom_config_default_kitti


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _normalized(T12):
    T = np.asarray(T12, np.float32).reshape(3, 4).copy()
    T[:, :3] = oracle.so3_normalize(T[:, :3].reshape(9)).reshape(3, 3)
    return T.reshape(12)


@dataclass
class Run:
    poses: list = field(default_factory=list)          # per frame, 12 floats
    status: list = field(default_factory=list)
    keyframe: list = field(default_factory=list)
    events: list = field(default_factory=list)         # per keyframe: (id, queried, cand id, distance, bias, inlier, accepted)
    kf_poses: list = field(default_factory=list)       # current (corrected)
    map: np.ndarray | None = None
    loops: int = 0


def run(scans, cfg, map_voxel: float, kdtree: bool = False, max_points: int = 1 << 15) -> Run:
    """cfg: lidar_odometry_amd.odometry.LoopConfig."""
    L = _lib.lib()
    icp = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=not kdtree), max_points=max_points)
    dm = DeviceVoxelMap(icp, 0.5, 3, 0.1, max_l0=1 << 21, max_points=max_points)
    iris_cfg = LoopClosureConfig(cfg.similarity_threshold, cfg.min_keyframe_gap, cfg.max_search_distance)
    iris = IrisLoopDetector(icp, capacity=cfg.max_keyframes, config=iris_cfg)
    gm = GlobalMapBuilder(icp, max_points=cfg.max_points, max_keyframes=cfg.max_keyframes)
    pgo = PoseGraphOptimizer()
    out = Run()
    clouds = []
    prev = vel = last_kf = I12
    last_loop = -1
    try:
        for k, raw in enumerate(scans):
            raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 3)
            status = _lib.LO_OK
            if k == 0:
                pose = I12
                kf = len(icp.voxel_filter(raw, VOXEL, STRIDE)) > 0
            else:
                guess = oracle.se3_compose(prev, vel)
                g_in = _normalized(guess)
                To = np.zeros(12, np.float32)
                st = _lib.LoStats()
                logs = (_lib.LoIterLog * _lib.LO_MAX_ITERS)()
                status = L.lo_icp_optimize_raw(icp.ctx, _fp(raw), len(raw), STRIDE, VOXEL, _fp(g_in), _fp(To), logs,
                                               C.byref(st))
                assert status >= 0, status
                pose = _normalized(To) if status == _lib.LO_OK else guess
                vel = oracle.se3_compose(oracle.se3_inverse(prev), pose)
                d, a = oracle.keyframe_metrics(last_kf, pose)
                kf = d > KF_DIST or a > KF_ROT
            prev = pose
            if kf:
                pose = np.ascontiguousarray(pose, np.float32)
                assert L.lo_devmap_update_from_scan(dm._h, _fp(pose), 1.2 * MAX_RANGE) == _lib.LO_OK
                if kdtree:
                    assert L.lo_devmap_sync_points(dm._h) == _lib.LO_OK
                last_kf = pose
                # ---- the loop bookkeeping of include/lo_odometry.h
                kid = len(out.kf_poses)
                cloud = icp.filtered_points()
                clouds.append(cloud)
                gm.add_keyframe(kid, cloud)
                if kid == 0:
                    pgo.add_first_keyframe(kid, pose)
                else:
                    rel = oracle.se3_compose(oracle.se3_inverse(out.kf_poses[-1]), pose)
                    pgo.add_keyframe_with_odom(kid - 1, kid, pose, rel, cfg.odom_trans_noise, cfg.odom_rot_noise)
                out.kf_poses.append(pose.copy())
                pos = pose.reshape(3, 4)[:, 3].copy()
                queried = kid - last_loop >= cfg.cooldown_keyframes
                cand = iris.detect(kid, pos, cloud) if queried else None
                iris.add_keyframe(kid, pos, cloud)
                ev = [kid, queried, -1, np.float32(0.0), 0, np.float32(0.0), False]
                if cand is not None:
                    mid = cand.match_keyframe_id
                    ev[2:5] = [mid, np.float32(cand.similarity_score), cand.bias]
                    ok, Tr, inl = icp.optimize_loop(cloud, pose, clouds[mid], out.kf_poses[mid])
                    ev[5] = np.float32(inl) if inl is not None else np.float32(0.0)
                    if ok and np.float32(inl) >= np.float32(cfg.min_inlier_ratio):
                        Tr12 = np.ascontiguousarray(np.asarray(Tr, np.float32)[:3, :4].reshape(12))
                        corrected = oracle.se3_compose(pose, Tr12)
                        con = oracle.se3_compose(oracle.se3_inverse(out.kf_poses[mid]), corrected)
                        if pgo.add_loop_and_optimize(mid, kid, con, cfg.loop_trans_noise, cfg.loop_rot_noise):
                            before = out.kf_poses[-1]
                            opt = pgo.get_all_optimized_poses()
                            out.kf_poses = [np.ascontiguousarray(opt[i][:3, :4].reshape(12), np.float32)
                                            for i in range(kid + 1)]
                            corr = oracle.se3_compose(out.kf_poses[-1], oracle.se3_inverse(before))
                            dm.apply_transform(corr)
                            if kdtree:
                                assert L.lo_devmap_sync_points(dm._h) == _lib.LO_OK
                            prev = out.kf_poses[-1]
                            last_loop = kid
                            out.loops += 1
                            ev[6] = True
                out.events.append(tuple(ev))
            out.poses.append(np.asarray(pose, np.float32).reshape(12).copy())
            out.status.append(status)
            out.keyframe.append(bool(kf))
        out.map = gm.build(np.stack(out.kf_poses), map_voxel) if out.kf_poses else np.zeros((0, 3), np.float32)
        return out
    finally:
        gm.close()
        iris.close()
        dm.close()
        pgo.close()
        icp.close()
