#!/usr/bin/env python
"""Loop-closure detector timings against database size, beside a numpy run of the same definition.

    python scripts/iris_bench.py [--sizes 64,1024,4096] [--points 4000] [--reps 20]

Per size: wall time of one add_keyframe (points -> image -> packed descriptor in the database), wall time of one
query (compare_all: image, encode, match against every entry at all 360 shifts, records back on the host), the
match kernel's own device time (HIP events over back-to-back launches), and what that time means in database bytes
streamed and 32-bit popcounts per second.  The numpy figure is tests/_iris_ref.py's hamming_all_shifts + best_shift on
already-encoded descriptors (no image / encode time), measured on a few entries and scaled to the database size.
One JSON line per size.
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

from lidar_odometry_amd import IrisLoopDetector, IterativeClosestPointOptimizer  # noqa: E402
from tests import _iris_ref as ref  # noqa: E402

DESC_BYTES = 43200                      # packed descriptor
POPC32_PER_SHIFT = 360 * 15 * 2         # 32-bit popcounts per (entry, shift): valid, Re and Im words of every column


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--numpy-entries", type=int, default=4)
    args = ap.parse_args()
    sizes = [int(s) for s in args.sizes.split(",")]

    rng = np.random.default_rng(0)
    bases = [ref.scene(s, n_ground=args.points * 5 // 8, per_wall=args.points // 32) for s in range(8)]
    query = ref.yawed(bases[0], 41, (0.3, 0.1, 0.0), 0.02, 1)

    icp = IterativeClosestPointOptimizer(max_points=1 << 17)
    det = IrisLoopDetector(icp, capacity=max(sizes))
    try:
        q_desc = det.encode(det.image(query))
        np_entries = [det.encode(det.image(b)) for b in bases[:args.numpy_entries]]
        t0 = time.perf_counter()
        for e in np_entries:
            ref.best_shift(*ref.hamming_all_shifts(q_desc[0], q_desc[1], e[0], e[1]))
        numpy_per_entry = (time.perf_counter() - t0) / len(np_entries)

        det.add_keyframe(0, [0, 0, 0], bases[0])            # warm-up (staging buffer, code load)
        det.compare_all(query)
        det.clear()
        for size in sizes:
            add_s, n_added = 0.0, 0
            while len(det) < size:
                k = len(det)
                cloud = ref.yawed(bases[k % len(bases)], float(rng.integers(0, 360)), (0.0, 0.0, 0.0))
                t0 = time.perf_counter()
                det.add_keyframe(k, [0, 0, 0], cloud)
                add_s += time.perf_counter() - t0
                n_added += 1
            walls = []
            for _ in range(5):
                t0 = time.perf_counter()
                dist, bias, _, _ = det.compare_all(query)
                walls.append(time.perf_counter() - t0)
            match_ms = det.bench_match(args.reps)
            pairs = size * 360
            print(json.dumps({
                "db_size": size, "points": len(query),
                "add_keyframe_ms": round(1e3 * add_s / max(n_added, 1), 4),
                "query_wall_ms": round(1e3 * float(np.median(walls)), 4),
                "match_kernel_ms": round(match_ms, 4),
                "numpy_match_ms": round(1e3 * numpy_per_entry * size, 1),
                "db_bytes_per_s": round(size * DESC_BYTES / (match_ms * 1e-3), 0),
                "operand_bytes_per_s": round(2.0 * pairs * DESC_BYTES / (match_ms * 1e-3), 0),
                "popc32_per_s": round(pairs * POPC32_PER_SHIFT / (match_ms * 1e-3), 0),
                "best": [float(np.nanmin(dist)), int(bias[int(np.nanargmin(dist))])],
            }), flush=True)
    finally:
        det.close()
        icp.close()


if __name__ == "__main__":
    main()
