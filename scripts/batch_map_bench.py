#!/usr/bin/env python
"""Keyframe map updates and whole frames for B sequences on one GPU: the batched forms beside one call per context.

    python scripts/batch_map_bench.py [--batches 64,256,1024] [--loop-batches 64] [--ways batched,per_context]
                                      [--passes 9] [--warmup 2] [--parent-json FILE] [--out profiles/batch_map_bench.json]
                                      [--kdtree]

Map updates.  B contexts (max_points 2^14) with one device map each (max_l0 2^15); every pass is one keyframe for all
B maps: frame 2 p of the 40-frame HDL-64-like sequence of the tests (~3.7k feature points at stride 8, voxel 0.5) at
its ground-truth pose, filtered into every context by the batched filter (not timed).  Timed on the host clock:
  batched      one lo_batch_update_maps + lo_batch_maps_status (the batch stream's synchronise);
  per_context  B lo_devmap_update_from_scan calls, then lo_sync on every context.
Each way has its own set of contexts and maps; after --warmup keyframes the ways alternate for --passes keyframes;
median [min, max].  The per-context figure that is quoted beside a batched one comes from a run of this script with
--ways per_context in a checkout of the commit before the batched update, not from the code under test; the
per_context way of the same process is printed as a cross-check.

Frame loop.  lo_odom_batch_process for B sequences beside B lo_odom_process loops over the same raw frames (the
sequence started from rest, --frames frames, the first --warmup frames not counted), per frame, in reference-exact and
in fast mode.  A way's window is its calls for the frame plus its own drain (lo_odom_batch_flush / lo_odom_flush on
every loop), so the keyframe's map update is inside the window of the way that enqueued it; the ways take turns to go
first.  --ways per_context times the solo loops alone: that is the run to make in a checkout of the parent commit,
and --parent-json FILE merges its figures (map updates and frame loop) into this run's output.

--kdtree.  The same two legs for KDTree-mode contexts (use_surfel_correspondence = 0), where every keyframe also
rebuilds the context's correspondence grid: batched is lo_batch_update_maps + lo_batch_sync_points +
lo_batch_maps_status, per_context is B x (lo_devmap_update_from_scan + lo_devmap_sync_points) and lo_sync on every
context; the frame loop is BatchLidarOdometry.kdtree beside B KDTree LidarOdometry loops.  Same windows, same drains;
the default --out becomes profiles/batch_kdtree_loop_bench.json.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lidar_odometry_amd import BatchOptimizer, ICPConfig, IterativeClosestPointOptimizer, lib, synth  # noqa: E402
from lidar_odometry_amd.voxelmap import DeviceVoxelMap  # noqa: E402

STRIDE, VOXEL, RADIUS = 8, 0.5, 120.0
MAXP, MAX_L0 = 1 << 14, 1 << 15


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


class MapSet:
    def __init__(self, B, kdtree=False):
        self.ctxs = [IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=not kdtree), max_points=MAXP)
                     for _ in range(B)]
        self.batch = BatchOptimizer(self.ctxs)
        self.maps = [DeviceVoxelMap(c, VOXEL, 3, 0.1, max_l0=MAX_L0, max_points=MAXP) for c in self.ctxs]

    def close(self):
        self.batch.close()
        for m in self.maps:
            m.close()
        for c in self.ctxs:
            c.close()


def run_maps(B, ways, scans, poses, passes, warmup, kdtree=False):
    L = lib()
    fp = C.POINTER(C.c_float)
    sets = {w: MapSet(B, kdtree) for w in ways}
    try:
        def batched(S, T):
            S.batch.update_maps(S.maps, [1] * B, [T] * B, RADIUS)
            if kdtree:
                S.batch.sync_points(S.maps)
            assert S.batch.maps_status(S.maps) == [0] * B

        def per_context(S, T):
            p = np.ascontiguousarray(T[:3].astype(np.float32).reshape(12))
            for m in S.maps:
                assert L.lo_devmap_update_from_scan(m._h, p.ctypes.data_as(fp), RADIUS) == 0
                if kdtree:
                    assert L.lo_devmap_sync_points(m._h) == 0
            for c in S.ctxs:
                assert L.lo_sync(c.ctx) == 0

        fn = {"batched": batched, "per_context": per_context}
        wall = {w: [] for w in ways}
        for p in range(warmup + passes):
            for w in ways:
                sets[w].batch.filter_raw([scans[p]] * B, STRIDE, VOXEL)
            for w in ways:
                t0 = time.perf_counter()
                fn[w](sets[w], poses[p])
                if p >= warmup:
                    wall[w].append(1e3 * (time.perf_counter() - t0))
        n0 = {w: sets[w].maps[0].counts()[0] for w in ways}
        for w in ways:
            assert all(m.status() == 0 for m in sets[w].maps)
        out = {"B": B, "l0_voxels_at_end": n0, "passes": passes, "warmup": warmup,
               "keyframe_wall_ms": {w: stats(v) for w, v in wall.items()}}
        if len(ways) == 2:
            out["per_context_over_batched"] = round(float(np.median(wall["per_context"]) / np.median(wall["batched"])), 2)
        return out
    finally:
        for S in sets.values():
            S.close()


def run_loop(B, ways, raws, T0, exact, warmup, kdtree=False):
    """Per frame and way: the way's calls for the frame plus its own drain (flush: the keyframe's map update done), so a
    window holds all of its frame's work and nothing of the other way's: both ways are drained before every window, and
    the ways take turns to go first."""
    from lidar_odometry_amd import odometry
    os.environ["LO_DEVMAP_MAX_L0"] = str(MAX_L0)
    solos = [odometry.LidarOdometry(max_points=MAXP, initial_pose=T0, exact=exact, use_surfel_correspondence=not kdtree)
             for _ in range(B)] if "per_context" in ways else []
    make = odometry.BatchLidarOdometry.kdtree if kdtree and "batched" in ways else odometry.BatchLidarOdometry
    bo = make(B, max_points=MAXP, initial_poses=[T0] * B, exact=exact, max_l0=MAX_L0) if "batched" in ways else None
    try:
        res = {}

        def batched(raw):
            res["batched"] = bo.process([raw] * B)
            bo.flush()

        def per_context(raw):
            res["per_context"] = [od.process(raw) for od in solos]
            for od in solos:
                od.flush()

        fn = {"batched": batched, "per_context": per_context}
        wall = {w: [] for w in ways}
        kf = 0
        same = True
        for k, raw in enumerate(raws):
            order = list(ways) if k % 2 == 0 else list(ways)[::-1]
            for w in order:
                t0 = time.perf_counter()
                fn[w](raw)                                   # (ends drained: the next window starts on an idle device)
                if k >= warmup:
                    wall[w].append(1e3 * (time.perf_counter() - t0))
            if len(ways) == 2:
                Tb = res["batched"][0]
                same = same and all(np.array_equal(Tb[j].view(np.uint32), res["per_context"][j][0].view(np.uint32))
                                    for j in range(B))
            if k >= warmup:
                info = res["batched"][1][0] if "batched" in ways else res["per_context"][0][1]
                kf += int(info.keyframe)
        out = {"B": B, "mode": "exact" if exact else "fast", "frames_timed": len(raws) - warmup, "keyframes_timed": kf,
               "frame_wall_ms": {w: stats(v) for w, v in wall.items()},
               "frame_wall_ms_each": {w: [round(x, 3) for x in v] for w, v in wall.items()}}
        if len(ways) == 2:
            out["poses_bit_equal"] = bool(same)
            out["per_context_over_batched"] = round(float(np.median(wall["per_context"]) / np.median(wall["batched"])), 2)
        return out
    finally:
        if bo is not None:
            bo.close()
        for od in solos:
            od.close()


def merge_parent(out, path):
    """The per_context figures of a run of this script in a checkout of the parent commit, beside this run's."""
    with open(path) as f:
        par = json.load(f)
    pm = {r["B"]: r["keyframe_wall_ms"]["per_context"] for r in par.get("map_updates", [])}
    for r in out["map_updates"]:
        if r["B"] in pm and "batched" in r["keyframe_wall_ms"]:
            r["keyframe_wall_ms"]["per_context_parent_commit"] = pm[r["B"]]
            r["parent_per_context_over_batched"] = round(pm[r["B"]]["median"] / r["keyframe_wall_ms"]["batched"]["median"], 2)
    pl = {(r["B"], r["mode"]): r["frame_wall_ms"]["per_context"] for r in par.get("frame_loop", [])}
    for r in out["frame_loop"]:
        if (r["B"], r["mode"]) in pl and "batched" in r["frame_wall_ms"]:
            r["frame_wall_ms"]["per_context_parent_commit"] = pl[(r["B"], r["mode"])]
            r["parent_per_context_over_batched"] = round(pl[(r["B"], r["mode"])]["median"] /
                                                         r["frame_wall_ms"]["batched"]["median"], 2)
    out["note"] = ("per_context_parent_commit: this script with --ways per_context in a checkout of the parent commit "
                   "(--parent-json); per_context: the code under test in this process, a cross-check only")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--loop-batches", default="64")
    ap.add_argument("--ways", default="batched,per_context")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--parent-json", default=None,
                    help="the JSON of a --ways per_context run in a checkout of the parent commit: merged into --out")
    ap.add_argument("--kdtree", action="store_true", help="KDTree-mode contexts: every keyframe also rebuilds the grid")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "batch_kdtree_loop_bench.json" if args.kdtree else "batch_map_bench.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this measurement has no CPU form")
    torch.zeros(1, device="cuda")        # torch's HIP runtime comes up before the library's
    ways = [w for w in args.ways.split(",") if w]
    if "batched" in ways and not hasattr(lib(), "lo_batch_update_maps"):
        raise SystemExit("this library has no lo_batch_update_maps: run with --ways per_context")
    if args.kdtree and "batched" in ways and not hasattr(lib(), "lo_batch_sync_points"):
        raise SystemExit("this library has no lo_batch_sync_points: run with --ways per_context")
    n = args.warmup + args.passes
    seq = synth.KittiLikeSequence(seed=7, n_frames=2 * n + 1)
    scans = [np.ascontiguousarray(seq.scan(2 * p, device="cuda")) for p in range(n)]
    poses = [seq.poses[2 * p] for p in range(n)]
    out = {"device": torch.cuda.get_device_name(0), "stride": STRIDE,
           "voxel_size": VOXEL, "max_l0": MAX_L0, "kdtree": bool(args.kdtree), "map_updates": [], "frame_loop": []}
    for B in (int(v) for v in args.batches.split(",") if v):
        r = run_maps(B, ways, scans, poses, args.passes, args.warmup, args.kdtree)
        print(json.dumps(r), flush=True)
        out["map_updates"].append(r)
    if "batched" not in ways or hasattr(lib(), "lo_odom_batch_process"):
        ramp = synth.KittiLikeSequence(seed=7, n_frames=args.frames, ramp_s=0.5)
        raws = [np.ascontiguousarray(ramp.scan(k, device="cuda")) for k in range(args.frames)]
        for B in (int(v) for v in args.loop_batches.split(",") if v):
            for exact in (True, False):
                r = run_loop(B, ways, raws, ramp.poses[0], exact, args.warmup, args.kdtree)
                print(json.dumps(r), flush=True)
                out["frame_loop"].append(r)
    if args.parent_json:
        merge_parent(out, args.parent_json)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
