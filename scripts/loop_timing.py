"""Wall time vs device-timeline time of the loop-closure ICP (lo_icp_optimize_loop) on the bench's keyframe pairs:
the difference is host work (matched-cloud grid + kd visit order, uploads, per-chunk syncs).  A second leg times
lo_icp_optimize_loop_dev (both clouds already on the device) against it on the same pairs: wall time per call, median
over repeated rounds after warm-up rounds, the two entries interleaved pair by pair so both see the same clocks."""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402,F401

from tests import _data  # noqa: E402
from lidar_odometry_amd import IterativeClosestPointOptimizer  # noqa: E402

torch.zeros(1, device="cuda")
icp = IterativeClosestPointOptimizer(max_points=1 << 17)
pairs = [_data.loop_case(fa, fa + 3 + (fa % 2), seed=fa) for fa in range(2, 26, 2)]
for rep in range(2):
    wall, dev, iters = [], [], []
    for cur, Tc, mat, Tm, _ in pairs:
        t0 = time.perf_counter()
        icp.optimize_loop(cur, Tc, mat, Tm)
        wall.append(time.perf_counter() - t0)
        st = icp.get_last_stats()
        dev.append(st.optimization_time_ms * 1e-3)
        iters.append(st.num_iterations)
    print(f"rep {rep}: wall {1e3 * np.mean(wall):.3f} ms, device timeline {1e3 * np.mean(dev):.3f} ms, "
          f"GN iterations {np.mean(iters):.2f}")

# ---- device entry against host entry, same pairs (results are bit-identical: tests/test_gpu_loop_dev.py)
dev_pairs = [(torch.from_numpy(cur).cuda(), Tc, torch.from_numpy(mat).cuda(), Tm) for cur, Tc, mat, Tm, _ in pairs]
torch.cuda.synchronize()
WARM, ROUNDS = 3, 20
host_ms, dev_ms = [], []
for rnd in range(WARM + ROUNDS):
    th = td = 0.0
    for (cur, Tc, mat, Tm, _), (dcur, _, dmat, _) in zip(pairs, dev_pairs):
        t0 = time.perf_counter()
        icp.optimize_loop(cur, Tc, mat, Tm)
        t1 = time.perf_counter()
        icp.optimize_loop_dev(dcur, Tc, dmat, Tm)
        t2 = time.perf_counter()
        th += t1 - t0
        td += t2 - t1
    if rnd >= WARM:
        host_ms.append(1e3 * th / len(pairs))
        dev_ms.append(1e3 * td / len(pairs))
h, d = np.asarray(host_ms), np.asarray(dev_ms)
print(f"per call over {len(pairs)} pairs, {ROUNDS} rounds after {WARM} warm-up: host entry median {np.median(h):.3f} ms "
      f"(min {h.min():.3f}, max {h.max():.3f}); device entry median {np.median(d):.3f} ms "
      f"(min {d.min():.3f}, max {d.max():.3f}); ratio {np.median(h) / np.median(d):.3f}")

# ---- the grid path: a matched cloud beyond kKnnAllMax (the 11.6k points of tests/test_gpu_loop_dev.py::
# test_grid_path_equals_host_entry), whose cell grid the device entry builds on the device with the occupancy rule
import oracle  # noqa: E402

cur, Tc, _, Tm, _ = _data.loop_case(4, 7, 3)
mat = oracle.voxel_filter(_data.kitti_scan(4, 40), 0.3, 1)
dcur, dmat = torch.from_numpy(cur).cuda(), torch.from_numpy(mat).cuda()
torch.cuda.synchronize()
host_ms, dev_ms = [], []
for rnd in range(WARM + ROUNDS):
    t0 = time.perf_counter()
    icp.optimize_loop(cur, Tc, mat, Tm)
    t1 = time.perf_counter()
    icp.optimize_loop_dev(dcur, Tc, dmat, Tm)
    t2 = time.perf_counter()
    if rnd >= WARM:
        host_ms.append(1e3 * (t1 - t0))
        dev_ms.append(1e3 * (t2 - t1))
h, d = np.asarray(host_ms), np.asarray(dev_ms)
print(f"grid path, {len(mat)} matched points, {ROUNDS} rounds after {WARM} warm-up: host entry median {np.median(h):.3f} ms "
      f"(min {h.min():.3f}, max {h.max():.3f}); device entry median {np.median(d):.3f} ms "
      f"(min {d.min():.3f}, max {d.max():.3f})")
icp.close()
