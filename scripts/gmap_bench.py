#!/usr/bin/env python
"""Global-map builder timings beside the one-core voxel grid on the same input.

    python scripts/gmap_bench.py [--cases e2e,1000] [--leaves 0.2,0.5] [--reps 50]

Cases (seeded, synthetic):
  e2e   bench.py's kitti_e2e run: the 60-frame HDL-64-like sequence from rest through the frame loop (LidarOdometry);
        its keyframes, each with its feature cloud (the device voxel filter of the raw scan at the loop's stride and
        voxel size) at the pose the loop gave it.
  1000  1,000 keyframes 1.2 m apart on the city serpentine (legs 44 m apart, so streets are seen again from the next
        leg), the e2e feature clouds reused in turn (~3.7k points each): the size of a long run's map rebuild after a
        loop closure.
Per case and leaf: the build's device time (lo_gmap_bench_build: HIP events over back-to-back builds after a warm-up
build), its split over the four stages (events around each stage, a second set of builds), points per second, the
transform kernel's bytes per second (12 B in, 20 B out per point) as a share of the 8 TB/s HBM peak, the wall time
of one build() with its download, and lo_gmap_voxelgrid_host on one core over the same transformed points -- whose
result must equal the device's bit for bit.  One JSON line per (case, leaf).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_odometry_amd import GlobalMapBuilder, IterativeClosestPointOptimizer, synth  # noqa: E402
from lidar_odometry_amd.gmap import voxelgrid_host  # noqa: E402
from lidar_odometry_amd.odometry import LidarOdometry  # noqa: E402

HBM_PEAK = 8.0e12
STAGES = ("transform_key", "sort", "heads_gather_scan", "centroids")


def e2e_keyframes(icp):
    """(feature clouds, 3x4 poses) of the keyframes of bench.py's kitti_e2e sequence."""
    n_frames = 60
    seq = synth.KittiLikeSequence(seed=7, n_frames=n_frames, ramp_s=2.0)
    od = LidarOdometry(device=0, initial_pose=seq.poses[0])
    clouds, poses = [], []
    try:
        for k in range(n_frames):
            raw = seq.scan(k, device="cuda")
            T, info = od.process(raw)
            if info.keyframe:
                clouds.append(icp.voxel_filter(raw, 0.5, stride=8))
                poses.append(np.asarray(T, np.float32).reshape(3, 4).copy())
        od.flush()
    finally:
        od.close()
    return clouds, np.stack(poses)


def city_keyframes(clouds, n_kf):
    seq = synth.KittiCitySequence(n_frames=2 * n_kf)
    poses = np.stack([seq.poses[2 * k][:3].astype(np.float32) for k in range(n_kf)])
    return [clouds[k % len(clouds)] for k in range(n_kf)], poses


def run_case(icp, name, clouds, poses, leaves, reps):
    n = int(sum(len(c) for c in clouds))
    gm = GlobalMapBuilder(icp, max_points=n, max_keyframes=len(clouds))
    try:
        for k, c in enumerate(clouds):
            gm.add_keyframe(k, c)
        world = gm.build(poses, 0.0)
        for leaf in leaves:
            got = gm.build(poses, leaf)                      # warm-up of every kernel at this size
            t0 = time.perf_counter()
            got = gm.build(poses, leaf)
            wall = time.perf_counter() - t0
            ms, stages = gm.bench_build(poses, leaf, reps)
            t0 = time.perf_counter()
            host = voxelgrid_host(world, leaf)
            host_s = time.perf_counter() - t0
            same = host.shape == got.shape and bool((host.view(np.uint32) == got.view(np.uint32)).all())
            print(json.dumps({
                "case": name, "keyframes": len(clouds), "points": n, "points_per_keyframe": round(n / len(clouds), 1),
                "leaf": leaf, "voxels": int(len(got)), "build_device_ms": round(ms, 4),
                "stage_ms": {s: round(v, 4) for s, v in zip(STAGES, stages)},
                "points_per_s": round(n / (ms * 1e-3), 0),
                "transform_bytes_per_s": round(32.0 * n / (stages[0] * 1e-3), 0),
                "transform_share_of_hbm_peak": round(32.0 * n / (stages[0] * 1e-3) / HBM_PEAK, 4),
                "build_wall_ms_with_download": round(1e3 * wall, 3),
                "host_one_core_ms": round(1e3 * host_s, 2), "speedup_device_vs_host": round(1e3 * host_s / ms, 1),
                "bit_equal_to_host": same,
            }), flush=True)
            if not same:
                raise SystemExit("device and host voxel grids differ")
    finally:
        gm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="e2e,1000")
    ap.add_argument("--leaves", default="0.2,0.5")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    leaves = [float(v) for v in args.leaves.split(",")]
    import torch
    torch.zeros(1, device="cuda")        # torch's HIP runtime comes up before the library's (the scans are raycast with it)
    icp = IterativeClosestPointOptimizer(max_points=1 << 17)
    try:
        clouds, poses = e2e_keyframes(icp)
        for case in args.cases.split(","):
            if case == "e2e":
                run_case(icp, "kitti_e2e", clouds, poses, leaves, args.reps)
            else:
                c, p = city_keyframes(clouds, int(case))
                run_case(icp, f"city_{case}", c, p, leaves, args.reps)
    finally:
        icp.close()


if __name__ == "__main__":
    main()
