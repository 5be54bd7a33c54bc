#!/usr/bin/env python
"""Raw scans in, poses out for B sequences on one GPU: the batched filter + batched optimize beside one raw optimize
per context.

    python scripts/batch_raw_bench.py [--batches 64,1024] [--passes 9] [--warmup 2] [--out profiles/batch_raw_bench.json]

Input (seeded, synthetic): eight scans of the 40-frame HDL-64-like sequence of the tests (frames 21..28, ~113k raw
points each, stride 8 -> ~14k samples -> ~3.7k feature points at voxel 0.5), dealt to the B contexts in turn; one
surfel map (keyframes 0, 2, ..., 20 at their ground-truth poses) uploaded to every context; initial poses perturbed
as in the tests.  Every context is in the library's default, reference-exact mode.

Per B, three ways from raw scans to poses, each pass timed on the host clock from the first call to the last record
on the host (every way ends in a device synchronise):
  a_host_pinned  lo_batch_optimize_raw on the scans in pinned host memory (the filter reads the samples in place);
  a_device       lo_batch_filter_raw + lo_batch_optimize_async + lo_batch_result on the scans in device memory;
  b_device       what the library offered before the batched filter: lo_icp_optimize_raw_async on each of the B
                 contexts (the same device scans), then lo_icp_result on each.
The batched filter alone (its five launches, HIP events on the batch stream: lo_batch_filter_ms) is read after every
a_* pass.  After --warmup untimed rounds the three ways alternate for --passes rounds; median, min and max are
reported.  The poses of the three ways must agree bit for bit (checked once, after the warm-up).
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

import oracle  # noqa: E402
from lidar_odometry_amd import BatchOptimizer, IterativeClosestPointOptimizer, lib, pinned_empty, synth  # noqa: E402
from lidar_odometry_amd._lib import LoBatchRec  # noqa: E402

STRIDE, VOXEL = 8, 0.5
FRAMES = tuple(range(21, 29))


def prepare():
    """(surfels, raw scans, initial poses (12 floats each)) of the benchmark; host only."""
    seq = synth.KittiLikeSequence(seed=7, n_frames=40)
    vm = oracle.VoxelMap(VOXEL, 3, 0.1, True)
    for k in range(0, 21, 2):
        T = seq.poses[k]
        vm.update(synth.transform(T, oracle.voxel_filter(seq.scan(k), VOXEL, STRIDE)), T[:3, 3], 120.0, True)
    k, n, c, _ = vm.surfels()
    raws = [np.ascontiguousarray(seq.scan(f), dtype=np.float32) for f in FRAMES]
    inits = [np.ascontiguousarray(synth.perturb(seq.poses[f], np.random.default_rng(42 + f), 0.05, 0.01)[:3]
                                  .astype(np.float32).reshape(12)) for f in FRAMES]
    return (k, n, c), raws, inits


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def run(B, surfels, raws, inits, passes, warmup):
    import torch
    L = lib()
    d_raw = [torch.from_numpy(r).cuda() for r in raws]
    p_raw = []
    for r in raws:
        p = pinned_empty(r.shape)
        p[:] = r
        p_raw.append(p)
    max_points = 1 << 14
    assert all((len(r) + STRIDE - 1) // STRIDE <= max_points for r in raws)
    ctxs = [IterativeClosestPointOptimizer(max_points=max_points) for _ in range(B)]
    batch = None
    try:
        for o in ctxs:
            o.set_surfels(*surfels)
        batch = BatchOptimizer(ctxs)
        sel = [j % len(raws) for j in range(B)]
        T = np.ascontiguousarray(np.stack([inits[i] for i in sel]))
        fp = C.POINTER(C.c_float)
        ns = (C.c_size_t * B)(*[len(raws[i]) for i in sel])
        host_ptrs = (C.c_void_p * B)(*[p_raw[i].ctypes.data for i in sel])
        dev_ptrs = (C.c_void_p * B)(*[d_raw[i].data_ptr() for i in sel])
        counts = (C.c_size_t * B)()
        recs = (LoBatchRec * B)()
        poses_b = np.zeros((B, 12), np.float32)

        def check(rc, what):
            if rc < 0:
                raise SystemExit(f"{what} failed ({rc}): {L.lo_batch_last_error(batch._b).decode()}")

        def a_host():
            check(L.lo_batch_optimize_raw(batch._b, host_ptrs, ns, STRIDE, VOXEL, T.ctypes.data_as(fp), recs, counts),
                  "lo_batch_optimize_raw")

        def a_dev():
            check(L.lo_batch_filter_raw(batch._b, dev_ptrs, ns, STRIDE, VOXEL, counts), "lo_batch_filter_raw")
            check(L.lo_batch_optimize_async(batch._b, None, counts, T.ctypes.data_as(fp)), "lo_batch_optimize_async")
            check(L.lo_batch_result(batch._b, recs, None), "lo_batch_result")

        def b_dev():
            for j, o in enumerate(ctxs):
                rc = L.lo_icp_optimize_raw_async(o.ctx, C.c_void_p(d_raw[sel[j]].data_ptr()), len(raws[sel[j]]), STRIDE,
                                                 C.c_float(VOXEL), T[j].ctypes.data_as(fp))
                if rc != 0:
                    raise SystemExit(f"lo_icp_optimize_raw_async failed ({rc})")
            for j, o in enumerate(ctxs):
                rc = L.lo_icp_result(o.ctx, poses_b[j].ctypes.data_as(fp), None, None)
                if rc < 0:
                    raise SystemExit(f"lo_icp_result failed ({rc})")

        def batch_poses():
            return np.stack([np.ctypeslib.as_array(r.pose).copy() for r in recs])

        ways = (("a_host_pinned", a_host), ("a_device", a_dev), ("b_device", b_dev))
        for _ in range(warmup):
            for _, f in ways:
                f()
        a_host()
        pa = batch_poses()
        ok = int(sum(r.status == 0 for r in recs))
        a_dev()
        pd = batch_poses()
        b_dev()
        equal = bool((pa.view(np.uint32) == pd.view(np.uint32)).all() and
                     (pa.view(np.uint32) == poses_b.view(np.uint32)).all())
        wall = {name: [] for name, _ in ways}
        filt = {"a_host_pinned": [], "a_device": []}
        for _ in range(passes):
            for name, f in ways:
                t0 = time.perf_counter()
                f()
                wall[name].append(1e3 * (time.perf_counter() - t0))
                if name in filt:
                    filt[name].append(float(L.lo_batch_filter_ms(batch._b)))
        med = {name: float(np.median(v)) for name, v in wall.items()}
        return {
            "B": B, "raw_points_per_scan": int(np.mean([len(r) for r in raws])),
            "filtered_points_per_scan": int(np.mean([int(n) for n in counts])), "jobs_converged": ok,
            "poses_bit_equal_across_ways": equal, "passes": passes, "warmup": warmup,
            "raw_to_poses_wall_ms": {name: stats(v) for name, v in wall.items()},
            "batched_filter_device_ms": {name: stats(v) for name, v in filt.items()},
            "scans_per_s": {name: round(B / (1e-3 * m), 0) for name, m in med.items()},
            "speedup_a_device_over_b_device": round(med["b_device"] / med["a_device"], 2),
            "speedup_a_host_pinned_over_b_device": round(med["b_device"] / med["a_host_pinned"], 2),
        }
    finally:
        if batch is not None:
            batch.close()
        for o in ctxs:
            o.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="64,1024")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_raw_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this measurement has no CPU form")
    torch.zeros(1, device="cuda")        # torch's HIP runtime comes up before the library's
    surfels, raws, inits = prepare()
    out = {"device": torch.cuda.get_device_name(0), "stride": STRIDE, "voxel_size": VOXEL, "mode": "reference-exact",
           "results": []}
    for B in (int(v) for v in args.batches.split(",")):
        r = run(B, surfels, raws, inits, args.passes, args.warmup)
        print(json.dumps(r), flush=True)
        out["results"].append(r)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
