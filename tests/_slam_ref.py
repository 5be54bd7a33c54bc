"""The frame loop with loop closure, assembled by hand from the library's public pieces (test infrastructure for
tests/test_gpu_slam.py): lo_icp_optimize_raw, lo_devmap_update_from_scan, IrisLoopDetector, GlobalMapBuilder,
lo_icp_optimize_loop on HOST clouds, PoseGraphOptimizer and lo_devmap_apply_transform.  The pose bookkeeping (previous
frame, guess, velocity, keyframe test, odometry edge, what a correction moves) is the frame-object model of
tests/_frame_ref.py, driven here by the library's ICP; the loop's own SE3f products (corrected pose, constraint,
correction) go through the oracle's restatements of the reference's SE3f algebra (oracle.se3_compose / se3_inverse).

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
from tests import _frame_ref

I12 = np.eye(3, 4, dtype=np.float32).reshape(12)
STRIDE, VOXEL, MAX_RANGE, KF_DIST, KF_ROT = 8, 0.5, 100.0, 1.0, 0.3      # lo_odom_config_default_kitti


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


@dataclass
class Run:
    poses: list = field(default_factory=list)          # per frame, 12 floats
    status: list = field(default_factory=list)
    keyframe: list = field(default_factory=list)
    events: list = field(default_factory=list)         # per keyframe: (id, queried, cand id, distance, bias, inlier, accepted)
    kf_poses: list = field(default_factory=list)       # current (corrected)
    map: np.ndarray | None = None
    loops: int = 0
    guesses: list = field(default_factory=list)        # per frame: the model's guess (None for the first frame)
    odom_edges: list = field(default_factory=list)     # per keyframe: the edge handed to the pose graph (None for the first)


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
    est = _frame_ref.Estimator(KF_DIST, KF_ROT)
    last_loop = -1
    try:
        for k, raw in enumerate(scans):
            raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 3)
            state = {"status": _lib.LO_OK}

            def lib_icp(_points, guess12, raw=raw, state=state):
                To = np.zeros(12, np.float32)
                st = _lib.LoStats()
                logs = (_lib.LoIterLog * _lib.LO_MAX_ITERS)()
                g = np.ascontiguousarray(guess12, np.float32)
                state["status"] = L.lo_icp_optimize_raw(icp.ctx, _fp(raw), len(raw), STRIDE, VOXEL, _fp(g), _fp(To), logs,
                                                        C.byref(st))
                assert state["status"] >= 0, state["status"]
                return state["status"] == _lib.LO_OK, To

            # (the model looks at the points of the first frame only: an empty feature cloud makes no keyframe)
            pose, kf, _ = est.process(icp.voxel_filter(raw, VOXEL, STRIDE) if k == 0 else raw, lib_icp)
            status = state["status"]
            if kf:
                pose = np.ascontiguousarray(pose, np.float32)
                assert L.lo_devmap_update_from_scan(dm._h, _fp(pose), 1.2 * MAX_RANGE) == _lib.LO_OK
                if kdtree:
                    assert L.lo_devmap_sync_points(dm._h) == _lib.LO_OK
                # ---- the loop bookkeeping of include/lo_odometry.h
                kid = len(out.kf_poses)
                cloud = icp.filtered_points()
                clouds.append(cloud)
                gm.add_keyframe(kid, cloud)
                if kid == 0:
                    pgo.add_first_keyframe(kid, pose)
                else:
                    rel = est.odom_edges[-1]
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
                            est.apply_correction(out.kf_poses)
                            last_loop = kid
                            out.loops += 1
                            ev[6] = True
                out.events.append(tuple(ev))
            out.poses.append(np.asarray(pose, np.float32).reshape(12).copy())
            out.status.append(status)
            out.keyframe.append(bool(kf))
        out.guesses = list(est.guesses)
        out.odom_edges = list(est.odom_edges)
        out.map = gm.build(np.stack(out.kf_poses), map_voxel) if out.kf_poses else np.zeros((0, 3), np.float32)
        return out
    finally:
        gm.close()
        iris.close()
        dm.close()
        pgo.close()
        icp.close()
