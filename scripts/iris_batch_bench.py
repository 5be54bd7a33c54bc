#!/usr/bin/env python
"""One frame's loop-closure work for B sequences: the batched detector against B solo detectors.

    python scripts/iris_batch_bench.py [--batches 16,64] [--sizes 64,1024] [--points 4000] [--out profiles/iris_batch_bench.json]

For B contexts whose databases hold N entries each, and one KITTI-size query cloud per job (host memory):
  batched  one lo_iris_batch_detect + one lo_iris_batch_add over all B jobs (BatchIrisDetector)
  solo     B x (lo_iris_detect + lo_iris_add_keyframe) on B solo detectors (IrisLoopDetector), one job after another
Both ways see the same clouds, ids and positions, and their candidates are compared (outside the timed window).  The
host clock runs from the first call to the last result; every call is synchronous, so the window ends with the device
idle.  2 warm-up rounds, then 9 timed rounds, the two ways alternating inside each round; median and [min, max].

Two eligibility settings per (B, N), each on freshly filled databases of exactly N entries:
  sparse  one entry in 20 lies within max_search_distance of the query (about 5 %), the rest 1 km away
  all     max_search_distance is huge: every one of the N entries is eligible (what is left is the launch saving)
The keyframes added during the rounds carry the previous queries' ids, so the keyframe-gap test gates them out for
both ways' candidates; the solo way still matches them, as it matches every entry.
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

from lidar_odometry_amd import (BatchIrisDetector, BatchOptimizer, IrisLoopDetector,  # noqa: E402
                                IterativeClosestPointOptimizer, LoopClosureConfig)
from tests import _iris_ref as ref  # noqa: E402

WARMUP, ROUNDS = 2, 9
FAR = 1000.0


def spread(xs):
    xs = [1e3 * x for x in xs]
    return {"median_ms": round(float(np.median(xs)), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def entry_position(i):
    return [0.0 if i % 20 == 0 else FAR, 0.0, 0.0]


def run_point(ctxs, n_entries, mode, variants):
    B = len(ctxs)
    cap = n_entries + WARMUP + ROUNDS
    batch = BatchOptimizer(ctxs)
    ib = BatchIrisDetector(batch, cap)
    solo = [IrisLoopDetector(c, cap) for c in ctxs]
    cfg = LoopClosureConfig(0.3, 50, 10.0 if mode == "sparse" else 1e9)
    jobs = list(range(B))
    try:
        for i in range(n_entries):
            cl = [variants[(i + j) % len(variants)] for j in jobs]
            pos = [entry_position(i)] * B
            assert ib.add(jobs, [i] * B, pos, cl) == [0] * B
            for j in jobs:
                solo[j].add_keyframe(i, pos[j], cl[j])
        t_b, t_s, equal, found = [], [], True, 0
        for r in range(WARMUP + ROUNDS):
            kid = n_entries + 100 + r
            cl = [variants[(r + 3 * j + 1) % len(variants)] for j in jobs]
            ids, pos, far = [kid] * B, [[0.0, 0.0, 0.0]] * B, [[FAR, 0.0, 0.0]] * B

            def batched():
                t0 = time.perf_counter()
                c = ib.detect(jobs, ids, pos, cl, cfg)
                ib.add(jobs, ids, far, cl)
                return time.perf_counter() - t0, c

            def one_by_one():
                t0 = time.perf_counter()
                c = []
                for j in jobs:
                    c.append(solo[j].detect(kid, pos[j], cl[j], cfg))
                    solo[j].add_keyframe(kid, far[j], cl[j])
                return time.perf_counter() - t0, c

            first, second = (batched, one_by_one) if r % 2 == 0 else (one_by_one, batched)
            (ta, ca), (tb, cb) = first(), second()
            equal = equal and ca == cb
            if r >= WARMUP:
                (t_b if first is batched else t_s).append(ta)
                (t_s if first is batched else t_b).append(tb)
                found += sum(c is not None for c in ca)
        eligible = sum(1 for i in range(n_entries) if mode == "all" or i % 20 == 0)
        b, s = spread(t_b), spread(t_s)
        return {"B": B, "N": n_entries, "mode": mode, "eligible_per_job": eligible, "points": int(len(variants[0])),
                "batched": b, "solo": s, "solo_over_batched": round(s["median_ms"] / b["median_ms"], 2),
                "candidates_equal": bool(equal), "candidates_per_round": found / ROUNDS}
    finally:
        for d in solo:
            d.close()
        ib.close()
        batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--sizes", default="64,1024")
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iris_batch_bench.json"))
    args = ap.parse_args()
    batches = [int(x) for x in args.batches.split(",")]
    sizes = [int(x) for x in args.sizes.split(",")]

    bases = [ref.scene(s, n_ground=args.points * 5 // 8, per_wall=args.points // 32) for s in range(4)]
    variants = [ref.yawed(b, 37.0 * k, (0.1 * k, 0.0, 0.0), 0.02, k) for k in range(4) for b in bases]
    ctxs = [IterativeClosestPointOptimizer(max_points=8192) for _ in range(max(batches))]
    rows = []
    try:
        for B in batches:
            for n in sizes:
                for mode in ("sparse", "all"):
                    row = run_point(ctxs[:B], n, mode, variants)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    finally:
        for c in ctxs:
            c.close()
    out = {"what": "one lo_iris_batch_detect + one lo_iris_batch_add over B jobs against B x (lo_iris_detect + "
                   "lo_iris_add_keyframe); host clock, first call to last result, ms",
           "warmup_rounds": WARMUP, "timed_rounds": ROUNDS, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
