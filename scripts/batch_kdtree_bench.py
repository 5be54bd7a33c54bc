#!/usr/bin/env python
"""KDTree-mode sequences on one GPU: one batched optimize for B contexts beside one optimize per context.

    python scripts/batch_kdtree_bench.py [--batches 64,256,1024] [--passes 9] [--warmup 2] [--mode exact|fast]
                                         [--ways batch,loop] [--out profiles/batch_kdtree_bench.json]

Input: bench.py's kitti_kdtree workload (the city-grid map after 660 frames as its L0 point cloud, 20 filtered scans
with perturbed initial poses), the scans dealt to the B contexts in turn; every context holds the same map
(lo_map_set_points: the host-built grid with the kd visit order).

Per B, two ways from host scans to poses, each pass timed on the host clock from the first call to the last record on
the host (both end in a device synchronise):
  batch  one lo_batch_optimize for all B (k_knn_b, k_knn_brute_b and k_plane_b per iteration for all jobs);
  loop   B lo_icp_optimize calls, one per context -- the only route for this work before KDTree batches (--ways loop
         runs on a library without them, to time that route there).
After --warmup untimed rounds the ways alternate for --passes rounds; median, min and max are reported.  With both ways
the poses must agree bit for bit (checked once, after the warm-up).  The contexts are created once, for the largest
B; a smaller B uses the first B of them.
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

import bench  # noqa: E402
from lidar_odometry_amd import BatchOptimizer, ICPConfig, IterativeClosestPointOptimizer, lib  # noqa: E402
from lidar_odometry_amd._lib import LoBatchRec  # noqa: E402


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def run(B, ctxs, scans, inits, passes, warmup, ways):
    L = lib()
    ctxs = ctxs[:B]
    sel = [j % len(scans) for j in range(B)]
    T = np.ascontiguousarray(np.stack([inits[i] for i in sel]))
    fp = C.POINTER(C.c_float)
    ns = (C.c_size_t * B)(*[len(scans[i]) for i in sel])
    ptrs = (C.c_void_p * B)(*[scans[i].ctypes.data for i in sel])
    recs = (LoBatchRec * B)()
    poses_l = np.zeros((B, 12), np.float32)
    status_l = np.zeros(B, np.int32)
    batch = BatchOptimizer(ctxs) if "batch" in ways else None
    try:
        def way_batch():
            rc = L.lo_batch_optimize(batch._b, ptrs, ns, T.ctypes.data_as(fp), recs)
            if rc < 0:
                raise SystemExit(f"lo_batch_optimize failed ({rc}): {L.lo_batch_last_error(batch._b).decode()}")

        def way_loop():
            for j, o in enumerate(ctxs):
                s = scans[sel[j]]
                rc = L.lo_icp_optimize(o.ctx, s.ctypes.data_as(fp), len(s), T[j].ctypes.data_as(fp),
                                       poses_l[j].ctypes.data_as(fp), None, None)
                if rc < 0:
                    raise SystemExit(f"lo_icp_optimize failed ({rc})")
                status_l[j] = rc

        fns = [(w, {"batch": way_batch, "loop": way_loop}[w]) for w in ways]
        for _ in range(warmup):
            for _, f in fns:
                f()
        equal = None
        if len(fns) == 2:
            way_batch()
            way_loop()
            pb = np.stack([np.ctypeslib.as_array(r.pose).copy() for r in recs])
            equal = bool((pb.view(np.uint32) == poses_l.view(np.uint32)).all() and
                         all(r.status == s for r, s in zip(recs, status_l)))
        wall = {w: [] for w, _ in fns}
        for _ in range(passes):
            for w, f in fns:
                t0 = time.perf_counter()
                f()
                wall[w].append(1e3 * (time.perf_counter() - t0))
        med = {w: float(np.median(v)) for w, v in wall.items()}
        ok = int(sum(r.status == 0 for r in recs)) if "batch" in ways else int((status_l == 0).sum())
        out = {"B": B, "points_per_scan": int(np.mean([len(scans[i]) for i in sel])), "jobs_converged": ok,
               "poses_bit_equal_across_ways": equal, "passes": passes, "warmup": warmup,
               "wall_ms": {w: stats(v) for w, v in wall.items()},
               "scans_per_s": {w: round(B / (1e-3 * m), 0) for w, m in med.items()}}
        if len(fns) == 2:
            out["speedup_batch_over_loop"] = round(med["loop"] / med["batch"], 2)
        return out
    finally:
        if batch is not None:
            batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--mode", default="exact", choices=["exact", "fast"])
    ap.add_argument("--ways", default="batch,loop")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_kdtree_bench.json"))
    args = ap.parse_args()
    ways = [w for w in args.ways.split(",") if w]
    if not ways or any(w not in ("batch", "loop") for w in ways) or len(set(ways)) != len(ways):
        raise SystemExit("--ways: batch, loop or both")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this measurement has no CPU form")
    torch.zeros(1, device="cuda")        # torch's HIP runtime comes up before the library's
    t0 = time.perf_counter()
    wl = bench.WORKLOADS["kitti_kdtree"](0)
    cloud = np.ascontiguousarray(wl["vm"].l0_cloud(), dtype=np.float32)
    scans = [np.ascontiguousarray(s, dtype=np.float32) for s in wl["scans"]]
    inits = [bench.pose12(T) for T in wl["inits"]]
    print(f"workload: {len(cloud)} map points, {len(scans)} scans of {min(map(len, scans))}..{max(map(len, scans))} "
          f"points, {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    sizes = [int(v) for v in args.batches.split(",")]
    max_points = 1 << 14
    assert all(len(s) <= max_points for s in scans)
    ctxs = []
    try:
        t0 = time.perf_counter()
        for j in range(max(sizes)):
            o = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False), max_points=max_points)
            ctxs.append(o)
            o.set_exact(args.mode == "exact")
            o.set_map_points(cloud)
            if (j + 1) % 64 == 0:
                print(f"contexts: {j + 1} ({time.perf_counter() - t0:.1f} s)", file=sys.stderr, flush=True)
        out = {"device": torch.cuda.get_device_name(0), "workload": wl["name"], "map_points": len(cloud), "mode": args.mode,
               "ways": ways, "results": []}
        for B in sizes:
            r = run(B, ctxs, scans, inits, args.passes, args.warmup, ways)
            print(json.dumps(r), flush=True)
            out["results"].append(r)
    finally:
        for o in ctxs:
            o.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
