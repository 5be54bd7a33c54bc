#!/usr/bin/env python
"""Batched loop-closure ICP beside one solo call per context: K loop candidates verified at once.

    python scripts/loop_batch_bench.py [--jobs 8,64,256] [--passes 9] [--warmup 2] [--out profiles/loop_batch_bench.json]

K loop pairs drawn from the 40-frame HDL-64-like sequence of the tests: keyframe fb re-observes keyframe fa (fb - fa in
3 .. 5), both feature clouds after stride 8 / 0.5 m voxels (~3.7k points, the all-pairs form), the current pose
perturbed as tests/_data.loop_case does (sigma 0.3 m / 0.03 rad), a different seed per pair.  K contexts
(max_points 2^13) in one batch; the clouds are device-resident before the clock starts.  Timed on the host clock, in
reference-exact and in fast mode:
  batched  one lo_batch_optimize_loop_dev over the K jobs;
  solo     K lo_icp_optimize_loop_dev calls, one per context (the entry this change leaves as it was).
After --warmup rounds the two ways alternate for --passes rounds; median [min, max] in ms.  Every batched record is
checked against its solo record (status, iterations, T_rel bits) in the first round.
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
from lidar_odometry_amd import BatchOptimizer, IterativeClosestPointOptimizer, _lib, lib, synth  # noqa: E402

STRIDE, VOXEL, MAXP, FRAMES = 8, 0.5, 1 << 13, 40
FP = C.POINTER(C.c_float)


def stats(v):
    v = np.asarray(v, np.float64)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def pose12(T):
    return np.ascontiguousarray(np.asarray(T, np.float64)[:3, :].astype(np.float32).reshape(12))


def pairs(K):
    seq = synth.KittiLikeSequence(seed=7, n_frames=FRAMES)
    feats = {}

    def feat(i):
        if i not in feats:
            feats[i] = np.ascontiguousarray(oracle.voxel_filter(seq.scan(i), VOXEL, STRIDE), np.float32)
        return feats[i]
    out = []
    for k in range(K):
        fa = (2 * k) % (FRAMES - 6)
        fb = fa + 3 + k % 3
        rng = np.random.default_rng(k)
        Tb0 = synth.perturb(seq.poses[fb], rng, 0.3, 0.03)
        out.append((feat(fb), pose12(Tb0), feat(fa), pose12(seq.poses[fa])))
    return out


def run(K, passes, warmup):
    import torch
    L = lib()
    ctxs = [IterativeClosestPointOptimizer(max_points=MAXP) for _ in range(K)]
    b = BatchOptimizer(ctxs)
    res = {}
    try:
        cases = pairs(K)
        dev = {}
        for c in cases:
            for a in (c[0], c[2]):
                if id(a) not in dev:
                    dev[id(a)] = torch.from_numpy(a).cuda()
        torch.cuda.synchronize()
        arr = (_lib.LoLoopJob * K)()
        for i, (cur, Tc, mat, Tm) in enumerate(cases):
            arr[i].job, arr[i].d_curr, arr[i].n_curr = i, dev[id(cur)].data_ptr(), len(cur)
            arr[i].d_matched, arr[i].n_matched = dev[id(mat)].data_ptr(), len(mat)
            arr[i].T_curr[:] = Tc.tolist()
            arr[i].T_matched[:] = Tm.tolist()
        recs = (_lib.LoLoopRec * K)()
        ms = C.c_double(0.0)
        Tr = np.zeros((K, 12), np.float32)
        inl = np.zeros(K, np.float32)
        sts = (_lib.LoStats * K)()
        solo_args = [(ctxs[i].ctx, arr[i].d_curr, arr[i].n_curr, arr[i].T_curr, arr[i].d_matched, arr[i].n_matched,
                      arr[i].T_matched, Tr[i].ctypes.data_as(FP), inl[i:].ctypes.data_as(FP), None, C.byref(sts[i]))
                     for i in range(K)]               # (built before the clock starts)

        def batched():
            t0 = time.perf_counter()
            rc = L.lo_batch_optimize_loop_dev(b._b, arr, K, recs, None, C.byref(ms))
            t1 = time.perf_counter()
            assert rc == _lib.LO_OK, L.lo_batch_last_error(b._b).decode()
            return 1e3 * (t1 - t0)

        def solo():
            t0 = time.perf_counter()
            for args in solo_args:
                L.lo_icp_optimize_loop_dev(*args)
            return 1e3 * (time.perf_counter() - t0)

        for exact in (True, False):
            for o in ctxs:
                o.set_exact(exact)
            tb, ts, dev_ms = [], [], []
            for r in range(warmup + passes):
                x, y = batched(), solo()
                if r == 0:
                    for i in range(K):
                        assert (recs[i].status, recs[i].iterations) == (sts[i].status, sts[i].iterations), i
                        if recs[i].converged:
                            assert np.array_equal(np.array(recs[i].T_rel[:], np.float32).view(np.uint32), Tr[i].view(np.uint32)), i
                if r >= warmup:
                    tb.append(x)
                    ts.append(y)
                    dev_ms.append(ms.value)
            its = [recs[i].iterations for i in range(K)]
            res["exact" if exact else "fast"] = {
                "batched_ms": stats(tb), "solo_ms": stats(ts), "batched_device_ms": stats(dev_ms),
                "speedup_median": round(float(np.median(ts) / np.median(tb)), 3),
                "iterations": {"min": int(min(its)), "max": int(max(its))},
                "ok_jobs": int(sum(recs[i].status == _lib.LO_OK for i in range(K)))}
            print(f"K={K} {'exact' if exact else 'fast'}: batched {res['exact' if exact else 'fast']['batched_ms']} "
                  f"solo {res['exact' if exact else 'fast']['solo_ms']}", flush=True)
    finally:
        b.close()
        for o in ctxs:
            o.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", default="8,64,256")
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loop_batch_bench.json"))
    a = ap.parse_args()
    import torch
    torch.zeros(1, device="cuda")                        # torch's HIP runtime first (tests/conftest.py)
    out = {"what": "lo_batch_optimize_loop_dev vs K lo_icp_optimize_loop_dev calls, host clock, ms",
           "points": {"stride": STRIDE, "voxel": VOXEL}, "passes": a.passes, "warmup": a.warmup, "jobs": {}}
    for K in [int(x) for x in a.jobs.split(",")]:
        out["jobs"][str(K)] = run(K, a.passes, a.warmup)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
