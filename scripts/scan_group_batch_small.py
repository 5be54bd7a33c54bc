#!/usr/bin/env python3
"""Wall and device time of one lockstep batch at small B on the kitti workload's scans (ISSUE "scan groups", step 1).

    python scripts/scan_group_batch_small.py [--out profiles/scan_group_batch_small.json] [--reps 200]
    python scripts/scan_group_batch_small.py --only 16 --mode exact --reps 50      (a run for rocprofv3 --kernel-trace)

For B in 2, 4, 8, 16, 32 and both arithmetic modes: B contexts on the bench's map, job j on a private copy of scan
j % 20, lo_batch_optimize_async + lo_batch_result back to back (enqueue + wait, as bench.py's batched leg), the mean of
the call's own device time (its two events) and the wall time per batch.  The PKO workgroup budget (LO_BATCH_PKO_WGS,
read by lo_batch_create) is swept per size.  The single-context queue of the same scans (bench.py's timed step) is
timed in the same process for the ratio the stop condition asks for: with scan groups off (queue_ms_per_step: every
scan down the scan ring, the queue as it was before scan groups) and, where the library has them, at 4, 8, 16 and 32
scans per group (queue_ms_per_step_by_group).  The lockstep batch is the same code before and after scan groups.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", type=int, default=0, help="one batch size only (profiling run)")
    ap.add_argument("--mode", default="both", choices=["both", "exact", "fast"])
    ap.add_argument("--budgets", default="64,128,256,512,1024")
    ap.add_argument("--queue-only", action="store_true",
                    help="only the single-context queue, at scan groups of 1 (off: the ring), 4, 8, 16 and 32")
    args = ap.parse_args()
    import torch

    import bench
    from lidar_odometry_amd import lib
    from lidar_odometry_amd._lib import LoBatchRec
    from lidar_odometry_amd.icp import (AdaptiveMEstimatorConfig, BatchOptimizer, ICPConfig,
                                        IterativeClosestPointOptimizer, MapGeometry)
    L = lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    wl = bench.build_kitti(0)
    max_pts = max(len(s) for s in wl["scans"])
    d_scans = [torch.from_numpy(s).to(dev) for s in wl["scans"]]
    inits = [bench.pose12(T) for T in wl["inits"]]
    nd = len(d_scans)
    fptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731

    def new_ctx(exact):
        o = IterativeClosestPointOptimizer(ICPConfig(), AdaptiveMEstimatorConfig(), MapGeometry(voxel_size=wl["voxel"]),
                                           device=0, max_points=max_pts)
        o.set_exact(exact)
        assert L.lo_map_set_from_voxelmap(o.ctx, wl["vm"].handle) == 0
        return o

    sizes = [args.only] if args.only else [2, 4, 8, 16, 32]
    modes = ["exact", "fast"] if args.mode == "both" else [args.mode]
    budgets = [256] if args.only else [int(x) for x in args.budgets.split(",")]
    res = {"workload": wl["name"], "scans": nd, "avg_points": float(np.mean([len(s) for s in wl["scans"]])),
           "reps": args.reps, "note": "device_ms: mean of lo_batch_result's gpu_ms (events around the batch's uploads, "
           "launches and record copy); wall_ms: enqueue + wait per batch; per_scan_us = device_ms / B", "modes": {}}
    for mode in modes:
        exact = mode == "exact"
        # the single-context queue (the flagship's timed step), same scans
        icp = new_ctx(exact)
        for i in range(nd):
            icp.optimize(None, wl["scans"][i], inits[i])

        def queue(K):
            for k in range(K):
                i = k % nd
                assert L.lo_icp_optimize_async(icp.ctx, C.c_void_p(d_scans[i].data_ptr()), d_scans[i].shape[0],
                                               fptr(inits[i])) == 0
            assert L.lo_sync(icp.ctx) == 0
        def timed_queue():
            queue(100)
            qs = []
            for _ in range(3 if not args.only else 1):
                t0 = time.perf_counter()
                queue(1000)
                qs.append((time.perf_counter() - t0) / 1000 * 1e3)
            return float(np.median(qs))
        # the ring alone (scan groups off) is the queue as it was before scan groups existed
        has_groups = hasattr(L, "lo_set_scan_group")
        if has_groups:
            icp.set_scan_group(1)
        out = {"queue_ms_per_step": timed_queue(), "sizes": []}
        if has_groups:
            out["queue_ms_per_step_by_group"] = {}
            for g in (4, 8, 16, 32):
                icp.set_scan_group(g)
                out["queue_ms_per_step_by_group"][str(g)] = timed_queue()
                print(f"[{mode}] queue, scan group {g}: {out['queue_ms_per_step_by_group'][str(g)] * 1e3:.1f} us/scan",
                      file=sys.stderr, flush=True)
            icp.set_scan_group(0)
        print(f"[{mode}] queue, ring: {out['queue_ms_per_step'] * 1e3:.1f} us/scan", file=sys.stderr, flush=True)
        if args.queue_only:
            res["modes"][mode] = out
            icp.close()
            continue
        pool = []
        for B in sizes:
            while len(pool) < B:
                pool.append(new_ctx(exact))
                pool[-1].optimize(None, wl["scans"][0], inits[0])
            sel = [j % nd for j in range(B)]
            job_scans = [d_scans[i].clone() for i in sel]
            c_ptrs = (C.c_void_p * B)(*[t.data_ptr() for t in job_scans])
            c_cnts = (C.c_size_t * B)(*[t.shape[0] for t in job_scans])
            c_T = np.ascontiguousarray(np.stack([inits[i] for i in sel]))
            recs = (LoBatchRec * B)()
            ms = C.c_double(0.0)
            row = {"B": B, "budgets": []}
            for wg in budgets:
                os.environ["LO_BATCH_PKO_WGS"] = str(wg)
                bo = BatchOptimizer(pool[:B])

                def step():
                    rc = L.lo_batch_optimize_async(bo._b, c_ptrs, c_cnts, fptr(c_T))
                    rc2 = L.lo_batch_result(bo._b, recs, C.byref(ms))
                    assert rc == 0 and rc2 == 0, (rc, rc2)
                    return ms.value
                for _ in range(10):
                    step()
                t0 = time.perf_counter()
                dms = [step() for _ in range(args.reps)]
                wall = (time.perf_counter() - t0) / args.reps * 1e3
                d = float(np.mean(dms))
                row["budgets"].append({"pko_wgs": wg, "pko_wgs_per_job": max(1, min(101, wg // B)), "device_ms": d,
                                       "wall_ms": wall, "per_scan_us": d / B * 1e3,
                                       "ok": int(sum(r.status == 0 for r in recs))})
                print(f"[{mode}] B={B} pko_wgs={wg}: device {d:.3f} ms, wall {wall:.3f} ms, {d / B * 1e3:.1f} us/scan",
                      file=sys.stderr, flush=True)
                bo.close()
            best = min(row["budgets"], key=lambda r: r["device_ms"])
            row["best_pko_wgs"] = best["pko_wgs"]
            row["default_256"] = next((r for r in row["budgets"] if r["pko_wgs"] == 256), None)
            out["sizes"].append(row)
        os.environ.pop("LO_BATCH_PKO_WGS", None)
        r16 = next((r for r in out["sizes"] if r["B"] == 16), None)
        if r16 and r16["default_256"]:
            out["per_scan_us_B16"] = r16["default_256"]["per_scan_us"]
            out["stop_condition"] = {"rule": "device time per scan at B = 16 below half of the queue's ms_per_step",
                                     "per_scan_ms_B16": r16["default_256"]["per_scan_us"] / 1e3,
                                     "half_queue_ms_per_step": out["queue_ms_per_step"] / 2,
                                     "go": r16["default_256"]["per_scan_us"] / 1e3 < out["queue_ms_per_step"] / 2}
        res["modes"][mode] = out
        for o in pool:
            o.close()
        icp.close()
    line = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
