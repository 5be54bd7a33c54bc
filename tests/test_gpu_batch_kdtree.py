"""GPU tests of KDTree-mode batches (lo_batch_* over use_surfel_correspondence = false contexts): the lockstep 5-NN
search (k_knn_b), the unresolved pass (k_knn_brute_b) and the plane fit (k_plane_b) for all jobs in one launch each.

Bar: the project's own single-context KDTree path, which tests/test_gpu_kdtree.py pins to the oracle and to nanoflann's
goldens.  Every job's batch record equals ``optimizers[j].optimize`` on the same input bit for bit: success, iterations,
n_corr, pose (as uint32), initial / final cost and alpha.  No tolerance anywhere.
"""
import numpy as np
import pytest

import oracle
from lidar_odometry_amd._lib import LO_ERR_CAPACITY
from tests import _data

pytestmark = pytest.mark.gpu

I12 = np.eye(3, 4, dtype=np.float32).reshape(12)


def _kd(max_points=1 << 14, voxel=0.5, exact=True):
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer, MapGeometry
    o = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False), geometry=MapGeometry(voxel_size=voxel),
                                       max_points=max_points)
    o.set_exact(exact)
    return o


def _bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(12)).view(np.uint32)


def _record(ok, To, st):
    """A single optimize's result in the fields of a batch record."""
    return dict(success=bool(ok), pose=_bits32(To), iterations=st.num_iterations, n_corr=st.num_correspondences,
                initial_cost=np.float32(st.initial_cost).view(np.uint32), final_cost=np.float32(st.final_cost).view(np.uint32),
                alpha=np.float64(st.iterations[-1]["alpha"]).view(np.uint64) if st.iterations else None)


def _single(o, pts, Ti):
    ok, To = o.optimize(None, pts, Ti)
    return _record(ok, To, o.get_last_stats())


def _of_batch(r):
    return dict(success=bool(r.success), pose=_bits32(r.pose), iterations=r.iterations, n_corr=r.n_corr,
                initial_cost=np.float32(r.initial_cost).view(np.uint32), final_cost=np.float32(r.final_cost).view(np.uint32),
                alpha=np.float64(r.alpha).view(np.uint64))


def _assert_same(got, want, msg):
    """got: a batch record (BatchResult or _of_batch's dict); want: a single's or another batch's record."""
    g = got if isinstance(got, dict) else _of_batch(got)
    for k in ("success", "iterations", "n_corr", "initial_cost", "final_cost"):
        assert g[k] == want[k], f"{msg}: {k} {g[k]} vs {want[k]}"
    np.testing.assert_array_equal(g["pose"], want["pose"], err_msg=f"{msg}: pose")
    if want["alpha"] is not None:            # a single that ran no iteration has no alpha on record
        assert g["alpha"] == want["alpha"], f"{msg}: alpha"


# ---------------------------------------------------------------- inputs (CPU; built once, never modified)
def _lattice_job():
    """The map and queries of test_kdtree_exact_ties_lattice: equal distances everywhere (on-device ranking by the kd
    visit order), and 100 queries 9 m away that the grid shells cannot certify (the unresolved pass)."""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    m = oracle.VoxelMap(0.25, 3, 0.1, False)
    m.update((g * 0.5).astype(np.float32), np.zeros(3), 1e3, True)
    rng = np.random.default_rng(5)
    q = (rng.integers(0, 22, size=(600, 3)) * 0.25).astype(np.float32)
    q[500:] += np.float32(9.0)
    return m.l0_cloud(), 0.25, q, I12


def _jobs():
    """(map cloud, voxel size, scan, T_init) of the heterogeneous batch."""
    jobs = []
    for f in (11, 21):
        m, pts, Ti, _ = _data.kitti_case(f)
        jobs.append((m.l0_cloud(), 0.5, pts, Ti))
    jobs.append(_lattice_job())
    rng = np.random.default_rng(3)
    jobs.append((rng.normal(size=(4, 3)).astype(np.float32), 0.5, rng.normal(size=(300, 3)).astype(np.float32), I12))
    m, pts, Ti, _ = _data.kitti_case(11)
    jobs.append((m.l0_cloud(), 0.5, pts[:0], Ti))                       # n = 0: skipped
    return jobs


class _Set:
    """The heterogeneous jobs' contexts (maps uploaded) and, per arithmetic mode, their single-optimize records."""

    def __init__(self):
        self.jobs = _jobs()
        self.ctxs = [_kd(voxel=v) for (_, v, _, _) in self.jobs]
        for o, (cloud, _, _, _) in zip(self.ctxs, self.jobs):
            o.set_map_points(cloud)
        self._singles = {}

    def set_exact(self, exact):
        for o in self.ctxs:
            o.set_exact(exact)

    def singles(self, exact):
        if exact not in self._singles:
            self.set_exact(exact)
            self._singles[exact] = [_single(o, p, T) for o, (_, _, p, T) in zip(self.ctxs, self.jobs)]
        return self._singles[exact]

    def close(self):
        for o in self.ctxs:
            o.close()


@pytest.fixture(scope="module")
def hset():
    s = _Set()
    yield s
    s.close()


def _run(ctxs, jobs):
    from lidar_odometry_amd import BatchOptimizer
    b = BatchOptimizer(ctxs)
    try:
        return b.optimize(None, [j[2] for j in jobs], [j[3] for j in jobs])
    finally:
        b.close()


# ---------------------------------------------------------------- 1. construction
def test_construction_one_mode_per_batch():
    from lidar_odometry_amd import BatchOptimizer, IterativeClosestPointOptimizer
    kd, kd2 = _kd(1024), _kd(1024)
    surfel = IterativeClosestPointOptimizer(max_points=1024)
    try:
        b = BatchOptimizer([kd, kd2])                   # refused before KDTree batches existed
        assert len(b) == 2
        b.close()
        with pytest.raises(RuntimeError):
            BatchOptimizer([surfel, kd])
        with pytest.raises(RuntimeError):
            BatchOptimizer([kd, surfel])
    finally:
        for o in (kd, kd2, surfel):
            o.close()


# ---------------------------------------------------------------- 2. heterogeneous lockstep batch
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_heterogeneous_batch_bitwise_vs_single(hset, exact):
    singles = hset.singles(exact)
    hset.set_exact(exact)
    res = _run(hset.ctxs, hset.jobs)
    for j, (r, s) in enumerate(zip(res, singles)):
        _assert_same(r, s, f"job {j}")
    # not on failures alone: a scan-to-map job converged on most of its points
    assert any(r.success and r.n_corr > len(j[2]) // 2 for r, j in zip(res, hset.jobs))
    for j in (3, 4):                                    # fewer than five map points / no scan: the initial pose
        assert not res[j].success
        np.testing.assert_array_equal(_bits32(res[j].pose), _bits32(hset.jobs[j][3]))


# ---------------------------------------------------------------- 3. repeat and job order
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_repeat_and_rotated_job_order(hset, exact):
    from lidar_odometry_amd import BatchOptimizer
    hset.set_exact(exact)
    scans, Ts = [j[2] for j in hset.jobs], [j[3] for j in hset.jobs]
    b = BatchOptimizer(hset.ctxs)
    try:
        first = [_of_batch(r) for r in b.optimize(None, scans, Ts)]
        again = b.optimize(None, scans, Ts)             # the cached device parameters; the unresolved list's atomics
        for j, (r, f) in enumerate(zip(again, first)):
            _assert_same(r, f, f"repeat job {j}")
    finally:
        b.close()
    rot = [2, 3, 4, 0, 1]
    res = _run([hset.ctxs[k] for k in rot], [hset.jobs[k] for k in rot])
    for slot, k in enumerate(rot):
        _assert_same(res[slot], first[k], f"rotated: job {k} in slot {slot}")


# ---------------------------------------------------------------- 4. a map replaced between batches
def test_map_replaced_between_batches():
    from lidar_odometry_amd import BatchOptimizer
    cases = [_data.kitti_case(f) for f in (11, 13, 17)]
    cloud = cases[0][0].l0_cloud()
    ctxs = [_kd() for _ in cases]
    try:
        for o in ctxs:
            o.set_map_points(cloud)
        scans, Ts = [c[1] for c in cases], [c[2] for c in cases]
        b = BatchOptimizer(ctxs)
        try:
            before = [_of_batch(r) for r in b.optimize(None, scans, Ts)]
            for j, r in enumerate(b.optimize(None, scans, Ts)):     # the device parameters are now cached
                _assert_same(r, before[j], f"cached job {j}")
            thinned = np.ascontiguousarray(cloud[::2])              # another map for job 1 (half the points)
            ctxs[1].set_map_points(thinned)
            after = b.optimize(None, scans, Ts)
            want = _single(ctxs[1], scans[1], Ts[1])
            _assert_same(after[1], want, "job 1 on its new map")
            assert not np.array_equal(_of_batch(after[1])["pose"], before[1]["pose"])   # the map did change the result
            for j in (0, 2):
                _assert_same(after[j], before[j], f"untouched job {j}")
        finally:
            b.close()
    finally:
        for o in ctxs:
            o.close()


# ---------------------------------------------------------------- 5. a device-built grid meets distance ties
def test_device_grid_ties_rerun_inside_the_batch():
    """The lattice and scan of test_device_grid_tie_reruns_with_kd_order: the device-built grid has no kd visit order, so
    its job is run again through its context by lo_batch_result; the host-built grid ranks the ties on the device."""
    from lidar_odometry_amd import BatchOptimizer, lib
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap, VoxelMap
    g = np.arange(-12, 12) * 0.5 + 0.25
    A2, B2 = np.meshgrid(g, g)
    a, b2 = A2.ravel(), B2.ravel()
    c = np.full(a.size, 0.25)
    world = np.ascontiguousarray(np.concatenate([np.stack([a, b2, c - 3.0], 1), np.stack([c + 3.0, a, b2], 1),
                                                 np.stack([a, c + 3.0, b2], 1)]), dtype=np.float32)
    rng = np.random.default_rng(3)
    scan = world[rng.choice(len(world), 600, replace=False)] + np.float32(0.25) * np.array([1, 0, 0], np.float32)
    scan = np.ascontiguousarray(scan, dtype=np.float32)
    T0 = np.eye(3, 4, dtype=np.float32)
    T0[:, 3] = [0.02, -0.01, 0.01]
    dev, host = _kd(4096), _kd(4096)
    dm = DeviceVoxelMap(dev, 0.5, 3, 0.1, max_l0=1 << 14, max_points=1 << 14)
    try:
        dm.update(world, np.zeros(3), 1000.0, True)
        L = lib()
        assert L.lo_devmap_sync_points(dm._h) == 0
        hv = VoxelMap(0.5, 3, 0.1, False)
        hv.update(world, np.zeros(3), 1000.0, True)
        host.set_map_points(hv.l0_cloud())
        r0 = L.lo_kd_reruns(dev.ctx)
        bt = BatchOptimizer([dev, host])
        try:
            res = bt.optimize(None, [scan, scan], [T0, T0])
        finally:
            bt.close()
        _assert_same(res[0], _of_batch(res[1]), "device grid vs host grid")
        assert L.lo_kd_reruns(dev.ctx) >= r0 + 1
        assert L.lo_kd_reruns(host.ctx) == 0
        _assert_same(res[1], _single(host, scan, T0), "host grid vs its single optimize")
    finally:
        dm.close()
        dev.close()
        host.close()


# ---------------------------------------------------------------- 6. raw scans in
def test_optimize_raw_bitwise_vs_single():
    from lidar_odometry_amd import BatchOptimizer
    frames = (11, 17)
    cases = [_data.kitti_case(f) for f in frames]
    raws = [_data.kitti_scan(f) for f in frames]
    ctxs = [_kd(1 << 16) for _ in frames]
    try:
        for o, cse in zip(ctxs, cases):
            o.set_map_points(cse[0].l0_cloud())
        singles = []
        for o, raw, cse in zip(ctxs, raws, cases):
            ok, To = o.optimize_raw(None, raw, cse[2], stride=8, voxel_size=0.5)
            singles.append(_record(ok, To, o.get_last_stats()))
        b = BatchOptimizer(ctxs)
        try:
            res = b.optimize_raw(None, raws, [cse[2] for cse in cases], stride=8, voxel_size=0.5)
            assert b.last_counts == [len(cse[1]) for cse in cases]
        finally:
            b.close()
        for j, (r, s) in enumerate(zip(res, singles)):
            _assert_same(r, s, f"raw job {j}")
        assert all(r.success for r in res)
    finally:
        for o in ctxs:
            o.close()


# ---------------------------------------------------------------- 7. in-flight state checks
def test_state_and_capacity_checks():
    from lidar_odometry_amd import BatchOptimizer
    kd = _kd(1024)
    try:
        b = BatchOptimizer([kd])
        try:
            with pytest.raises(RuntimeError):
                b.result()                              # nothing in flight
            with pytest.raises(RuntimeError) as e:
                b.optimize(None, [np.zeros((2048, 3), np.float32)], [I12])      # beyond max_points
            assert int(str(e.value).split("error")[1].split(":")[0]) == LO_ERR_CAPACITY
            res = b.optimize(None, [np.zeros((100, 3), np.float32)], [I12])     # still usable; empty map
            assert not res[0].success
        finally:
            b.close()
    finally:
        kd.close()
