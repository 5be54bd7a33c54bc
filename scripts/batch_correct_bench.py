#!/usr/bin/env python
"""The map correction after accepted loops for K sequences on one GPU: one batched call beside K single calls.

    python scripts/batch_correct_bench.py [--batches 1,16,64,256] [--ways batched,solo,solo_enqueued] [--passes 9]
                                          [--warmup 2] [--parent-json FILE] [--out profiles/batch_correct_bench.json]

K contexts (max_points 2^14) with one device map each (max_l0 2^14, so that 256 maps of every way fit), every map built
from the keyframes at frames 0, 2 and 4 of the HDL-64-like sequence of the tests (stride 8, voxel 0.5; ~5.9k L0 voxels,
~2.1k L1 voxels).  Every pass first gives every map of every way one more keyframe through the batched update (not
timed: the maps stay populated and equal across the ways), then times one correction of all K maps on the host clock:
  batched        one lo_batch_apply_transform + lo_batch_maps_status (the batch stream's synchronise);
  solo           K x (lo_devmap_apply_transform, then lo_sync on its context): every call drained before the next;
  solo_enqueued  K lo_devmap_apply_transform calls, then lo_sync on every context (the contexts' streams may overlap).
The correction alternates between se3(rot_z(0.05), [0.4, -0.3, 0.02]) and its inverse, which merges voxels either way
and keeps the maps in place.  Each way has its own contexts and maps; after --warmup passes the ways take turns for
--passes passes; median [min, max].  At the end map 0 of every way is compared bit for bit.

--ways solo,solo_enqueued needs no batched entry: that is the run to make in a checkout of the parent commit, and
--parent-json FILE merges its figures into this run's output as solo_parent_commit / solo_enqueued_parent_commit.
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

from lidar_odometry_amd import BatchOptimizer, IterativeClosestPointOptimizer, lib, synth  # noqa: E402
from lidar_odometry_amd.voxelmap import DeviceVoxelMap  # noqa: E402

STRIDE, VOXEL, RADIUS = 8, 0.5, 120.0
MAXP, MAX_L0 = 1 << 14, 1 << 14
BUILD = (0, 2, 4)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


class MapSet:
    def __init__(self, K):
        self.ctxs = [IterativeClosestPointOptimizer(max_points=MAXP) for _ in range(K)]
        self.batch = BatchOptimizer(self.ctxs)
        self.maps = [DeviceVoxelMap(c, VOXEL, 3, 0.1, max_l0=MAX_L0, max_points=MAXP) for c in self.ctxs]

    def keyframe(self, raw, T):
        K = len(self.maps)
        self.batch.filter_raw([raw] * K, STRIDE, VOXEL)
        self.batch.update_maps(self.maps, [1] * K, [T] * K, RADIUS)
        assert self.batch.maps_status(self.maps) == [0] * K

    def close(self):
        self.batch.close()
        for m in self.maps:
            m.close()
        for c in self.ctxs:
            c.close()


def run(K, ways, scans, poses, passes, warmup):
    L = lib()
    fp = C.POINTER(C.c_float)
    sets = {w: MapSet(K) for w in ways}
    try:
        def p12(T):
            return np.ascontiguousarray(np.asarray(T)[:3].astype(np.float32).reshape(12))

        def batched(S, T):
            S.batch.apply_transform(S.maps, [1] * K, [T] * K)
            assert S.batch.maps_status(S.maps) == [0] * K

        def solo(S, T):
            p = p12(T)
            for m, c in zip(S.maps, S.ctxs):
                assert L.lo_devmap_apply_transform(m._h, p.ctypes.data_as(fp)) == 0
                assert L.lo_sync(c.ctx) == 0

        def solo_enqueued(S, T):
            p = p12(T)
            for m in S.maps:
                assert L.lo_devmap_apply_transform(m._h, p.ctypes.data_as(fp)) == 0
            for c in S.ctxs:
                assert L.lo_sync(c.ctx) == 0

        fn = {"batched": batched, "solo": solo, "solo_enqueued": solo_enqueued}
        for S in sets.values():
            for k in BUILD:
                S.keyframe(scans[k], poses[k])
        built = {w: sets[w].maps[0].counts() for w in ways}
        Cx = synth.se3(synth.rot_z(0.05), [0.4, -0.3, 0.02])
        Ci = np.linalg.inv(Cx)
        moved = np.eye(4)
        wall = {w: [] for w in ways}
        l0 = {w: [] for w in ways}
        for p in range(warmup + passes):
            k = BUILD[-1] + 1 + p
            for S in sets.values():
                S.keyframe(scans[k], moved @ poses[k])
            step = Cx if p % 2 == 0 else Ci
            order = list(ways)[p % len(ways):] + list(ways)[:p % len(ways)]
            for w in order:
                n_before = sets[w].maps[0].counts()[0]         # (drains the context: the window starts idle)
                t0 = time.perf_counter()
                fn[w](sets[w], step)
                if p >= warmup:
                    wall[w].append(1e3 * (time.perf_counter() - t0))
                    l0[w].append([n_before, sets[w].maps[0].counts()[0]])
            moved = step @ moved
        for w in ways:
            assert all(m.status() == 0 for m in sets[w].maps)
        ref = sets[ways[0]].maps[0]
        same = True
        for w in ways[1:]:
            for x, y in zip(ref.l0(), sets[w].maps[0].l0()):
                same = same and x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32))
            a, b = ref.l1(), sets[w].maps[0].l1()
            same = same and all(a[q].shape == b[q].shape and np.array_equal(a[q].view(np.uint8), b[q].view(np.uint8))
                                for q in a)
        out = {"K": K, "passes": passes, "warmup": warmup, "l0_l1_surfels_as_built": built[ways[0]],
               "l0_before_after_each_pass": l0[ways[0]], "maps_bit_equal_across_ways": bool(same),
               "correction_wall_ms": {w: stats(v) for w, v in wall.items()}}
        if "batched" in ways:
            for w in ways:
                if w != "batched":
                    out[w + "_over_batched"] = round(float(np.median(wall[w]) / np.median(wall["batched"])), 2)
        return out
    finally:
        for S in sets.values():
            S.close()


def merge_parent(out, path):
    with open(path) as f:
        par = json.load(f)
    pm = {r["K"]: r["correction_wall_ms"] for r in par.get("corrections", [])}
    for r in out["corrections"]:
        for w, v in pm.get(r["K"], {}).items():
            r["correction_wall_ms"][w + "_parent_commit"] = v
            if "batched" in r["correction_wall_ms"]:
                r[w + "_parent_commit_over_batched"] = round(v["median"] / r["correction_wall_ms"]["batched"]["median"], 2)
    out["note"] = ("*_parent_commit: this script with --ways solo,solo_enqueued in a checkout of the parent commit, run "
                   "directly before this one (--parent-json); solo / solo_enqueued: the code under test in this process")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64,256")
    ap.add_argument("--ways", default="batched,solo,solo_enqueued")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-json", default=None,
                    help="the JSON of a --ways solo,solo_enqueued run in a checkout of the parent commit: merged into --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_correct_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this measurement has no CPU form")
    torch.zeros(1, device="cuda")        # torch's HIP runtime comes up before the library's
    ways = [w for w in args.ways.split(",") if w]
    if "batched" in ways and not hasattr(lib(), "lo_batch_apply_transform"):
        raise SystemExit("this library has no lo_batch_apply_transform: run with --ways solo,solo_enqueued")
    n = BUILD[-1] + 1 + args.warmup + args.passes
    seq = synth.KittiLikeSequence(seed=7, n_frames=n + 1)
    scans = [np.ascontiguousarray(seq.scan(k, device="cuda")) for k in range(n)]
    out = {"device": torch.cuda.get_device_name(0), "stride": STRIDE, "voxel_size": VOXEL, "max_l0": MAX_L0,
           "max_points": MAXP, "corrections": []}
    for K in (int(v) for v in args.batches.split(",") if v):
        r = run(K, ways, scans, seq.poses, args.passes, args.warmup)
        print(json.dumps(r), flush=True)
        out["corrections"].append(r)
    if args.parent_json:
        merge_parent(out, args.parent_json)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
