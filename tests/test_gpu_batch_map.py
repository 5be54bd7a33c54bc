"""Batched keyframe map updates (lo_batch_update_maps / lo_batch_maps_status; csrc/lo_devmap.hip k_dm_*_b): the update
pipeline of lo_devmap_update_from_scan, one launch per phase for all active jobs of a batch.

Bar: after every step each job's device map equals its host VoxelMap (the specification, as in
tests/test_gpu_devmap.py): L0 order and centroids, the counts, the surfels in L1 order, and the context table the map
patches answers lookups like a full upload of the host map.  Where a batched update is compared with the single call,
both device maps' L0 and L1 containers are compared whole.  Every equality is on bits (.view(np.uint32)).

The host map is fed what the device computes from: the context's own device-filtered scan, moved to the world frame
with util::transform_point_cloud's fp32 expression order (k_dm_world).
"""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import synth
from lidar_odometry_amd._lib import LO_ERR_ARG, LO_ERR_CAPACITY, LO_OK
from tests.test_gpu_devmap import _same_lookups, _same_maps

pytestmark = pytest.mark.gpu

MAXP = 1 << 15
RADIUS = 120.0


def world(T, p):
    """((T0 x + T1 y) + T2 z) + T3, every step rounded to fp32 (lo_math.h transform_points, k_dm_world)."""
    T = np.asarray(T, np.float32).reshape(-1)[:12].reshape(3, 4)
    p = np.asarray(p, np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    one = np.float32(1.0)
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] * one for r in range(3)], axis=1)


def pose12(T):
    return np.ascontiguousarray(np.asarray(T, np.float32)[:3, :4].reshape(12))


def same_device_maps(a, b):
    """Two device maps: L0 and L1 containers whole, in order."""
    for x, y in zip(a.l0(), b.l0()):
        assert x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
    la, lb = a.l1(), b.l1()
    for k in la:
        assert la[k].shape == lb[k].shape, k
        np.testing.assert_array_equal(la[k].view(np.uint8), lb[k].view(np.uint8), err_msg=k)


class Jobs:
    """B contexts, their batch, one device map and one host map per job."""

    def __init__(self, max_l0s, kdtree=False, max_points=MAXP):
        from lidar_odometry_amd import BatchOptimizer, ICPConfig, IterativeClosestPointOptimizer
        from lidar_odometry_amd.voxelmap import DeviceVoxelMap, VoxelMap
        self.ctxs = [IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=not kdtree), max_points=max_points)
                     for _ in max_l0s]
        self.b = BatchOptimizer(self.ctxs)
        self.dms = [DeviceVoxelMap(c, 0.5, 3, 0.1, max_l0=m, max_points=max_points) for c, m in zip(self.ctxs, max_l0s)]
        self.vms = [VoxelMap(0.5, 3, 0.1, not kdtree) for _ in max_l0s]
        self.clouds = [np.zeros((0, 3), np.float32) for _ in max_l0s]
        self.ref = None                                      # a context for full uploads of the host maps (check_lookups)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self.ref is not None:
            self.ref.close()
        self.b.close()
        for d in self.dms:
            d.close()
        for c in self.ctxs:
            c.close()

    def filter(self, raws, stride=8, voxel=0.5):
        counts = self.b.filter_raw(raws, stride, voxel)
        self.clouds = [c.filtered_points() if n else np.zeros((0, 3), np.float32) for c, n in zip(self.ctxs, counts)]
        return counts

    def host_update(self, j, T, radius=RADIUS):
        T = np.asarray(T, np.float32)
        self.vms[j].update(world(T, self.clouds[j]), T[:3, 3].astype(np.float64), radius, True)

    def batched(self, active, poses, radius=RADIUS, host=True, wait=True):
        """One batched update over the active jobs (and the host maps' updates); returns maps_status."""
        if host:
            for j, a in enumerate(active):
                if a:
                    self.host_update(j, poses[j], radius)
        self.b.update_maps(self.dms, active, poses, radius)
        return self.b.maps_status(self.dms) if wait else None     # (maps_status waits for the batch stream)

    def single(self, j, T, radius=RADIUS):
        from lidar_odometry_amd import lib
        self.host_update(j, T, radius)
        p = pose12(T)
        assert lib().lo_devmap_update_from_scan(self.dms[j]._h, p.ctypes.data_as(C.POINTER(C.c_float)), radius) == LO_OK

    def check(self, jobs=None):
        for j in (range(len(self.dms)) if jobs is None else jobs):
            _same_maps(self.vms[j], self.dms[j])            # (counts() waits for the context stream)

    def check_lookups(self, j, scan, poses):
        from lidar_odometry_amd import IterativeClosestPointOptimizer, lib
        if self.ref is None:
            self.ref = IterativeClosestPointOptimizer(max_points=MAXP)
        assert lib().lo_map_set_from_voxelmap(self.ref.ctx, self.vms[j].handle) == 0
        _same_lookups(self.ctxs[j], self.ref, scan, [pose12(T) for T in poses])


class _Seq(synth.KittiLikeSequence):
    def scan(self, i, device="cuda"):                     # raycast on the GPU: these are GPU tests, and it saves seconds
        return super().scan(i, device=device)


def _seqs(seeds, n):
    return [_Seq(seed=s, n_frames=n) for s in seeds]


def _snapshot(dm):
    return [a.copy() for a in dm.l0()] + [dm.l1()[k].copy() for k in ("keys", "has_surfel", "normals", "children")]


def test_subsets_of_a_batch_with_different_capacities():
    """B = 3 maps of different max_l0 on three sequences over 6 keyframes; active = {0, 2}, {1}, all, none in turn:
    after every step every job's map is its host map and its patched table answers lookups like a full upload of the
    host map (the step's own filtered scan at the step's pose; an inactive job's table included), and inactive jobs'
    maps do not change."""
    from lidar_odometry_amd.voxelmap import voxel_filter
    seqs = _seqs((7, 9, 11), 13)
    patterns = [(1, 0, 1), (0, 1, 0), (1, 1, 1), (0, 0, 0), (1, 0, 1), (1, 1, 1)]
    with Jobs([1 << 16, 1 << 17, 1 << 15]) as J:
        for step, act in enumerate(patterns):
            k = 2 * step
            J.filter([s.scan(k) for s in seqs])
            idle = {j: _snapshot(J.dms[j]) for j in range(3) if not act[j]}
            st = J.batched(act, [s.poses[k] for s in seqs])
            assert st == [LO_OK] * 3
            J.check()
            for j, s in enumerate(seqs):
                if step > 0 or act[j]:                      # (a job without a keyframe yet has an empty table)
                    J.check_lookups(j, J.clouds[j], [s.poses[k]])
            for j, before in idle.items():
                for x, y in zip(before, _snapshot(J.dms[j])):
                    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
        assert min(v.surfel_count() for v in J.vms) > 50 and min(v.l0_count() for v in J.vms) > 1000
        for j, s in enumerate(seqs):
            scan = voxel_filter(s.scan(11), 0.5, 8)
            rng = np.random.default_rng(j)
            J.check_lookups(j, scan, [s.poses[11], synth.perturb(s.poses[11], rng, 0.3, 0.03)])


def test_batch_of_one_equals_the_single_call():
    from lidar_odometry_amd import IterativeClosestPointOptimizer, lib
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap
    seq = _seqs((7,), 9)[0]
    S = IterativeClosestPointOptimizer(max_points=MAXP)
    sm = DeviceVoxelMap(S, 0.5, 3, 0.1, max_l0=1 << 16, max_points=MAXP)
    try:
        with Jobs([1 << 16]) as J:
            for k in range(0, 9, 2):
                raw = seq.scan(k)
                J.filter([raw])
                S.voxel_filter(raw, 0.5, 8)
                assert J.batched([1], [seq.poses[k]]) == [LO_OK]
                p = pose12(seq.poses[k])
                assert lib().lo_devmap_update_from_scan(sm._h, p.ctypes.data_as(C.POINTER(C.c_float)), RADIUS) == LO_OK
                same_device_maps(J.dms[0], sm)
            J.check()
    finally:
        sm.close()
        S.close()


def test_batched_and_single_updates_alternate_with_transform_and_table_reupload():
    """Batched and single updates on the same maps in turn, one ApplyTransformAndRehash in between, and an unrelated
    upload into job 0's table between two batched updates (the table's generation changes: the map refills it and the
    batch re-uploads that job's descriptor)."""
    from lidar_odometry_amd.voxelmap import voxel_filter
    seqs = _seqs((7, 9), 15)
    Cx = synth.se3(synth.rot_z(0.05), [0.4, -0.3, 0.02])
    with Jobs([1 << 16, 1 << 16]) as J:
        moved = np.eye(4)
        for step, k in enumerate(range(0, 14, 2)):
            J.filter([s.scan(k) for s in seqs])
            poses = [moved @ s.poses[k] for s in seqs]
            if step in (1, 4):                              # the single call, job by job (contexts idle: check() waited)
                for j in range(2):
                    J.single(j, poses[j])
            else:
                assert J.batched([1, 1], poses) == [LO_OK, LO_OK]
            J.check()
            if step == 2:
                for j in range(2):
                    J.vms[j].apply_transform(Cx[:3].astype(np.float32))
                    J.dms[j].apply_transform(Cx[:3].astype(np.float32))
                moved = Cx
                J.check()
            if step == 5:
                J.ctxs[0].set_surfels(np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
        for j, s in enumerate(seqs):
            J.check_lookups(j, voxel_filter(s.scan(14), 0.5, 8), [Cx @ s.poses[14]])


def test_churn_in_one_job_beside_a_plain_sequence():
    """Job 0: the churn scene of test_devmap_planarity_erase_and_churn (noisy clutter, a sensor jumping between two
    places with a small radius: erase batches, whole regions pruned, tombstones renewing the indices); job 1: a plain
    sequence.  The radius is the batch's, so the plain job is pruned at 35 m too."""
    seq = _seqs((7,), 15)[0]
    sc = synth.patch_scene(n_patches=60, seed=3, extent=25.0)
    rng = np.random.default_rng(4)
    sizes = []
    with Jobs([1 << 16, 1 << 16]) as J:
        for k in range(14):
            off = np.array([0.0 if k % 3 else 300.0, 40.0 * (k % 2), 0.0], np.float32)
            local = synth.sample_patches(sc, 20000, 50 + k, outlier_frac=0.3)
            local = local[rng.permutation(len(local))]
            # every point of job 0 in 0.1 m cells (keeps the clutter dense); job 1's scan thinned beforehand
            J.b.filter_raw([local, np.ascontiguousarray(seq.scan(k)[::8])], 1, 0.1)
            J.clouds = [c.filtered_points() for c in J.ctxs]
            T0 = np.eye(4)
            T0[:3, 3] = off
            assert J.batched([1, 1], [T0, seq.poses[k]], 35.0) == [LO_OK, LO_OK]
            J.check()
            sizes.append(J.vms[0].l0_count())
        assert any(b < a for a, b in zip(sizes, sizes[1:])), sizes      # the prune emptied whole regions
        assert J.vms[0].surfel_count() > 0


def test_empty_scan_and_overflow_stay_in_their_own_jobs():
    """Job 0's scan filters to nothing (counts unchanged, UpdateVoxelMap returns before the prune), job 1's map
    (max_l0 = 64) overflows: maps_status reports LO_ERR_CAPACITY for job 1 only and jobs 0 and 2 are still exact."""
    seqs = _seqs((7, 9, 11), 5)
    with Jobs([1 << 16, 64, 1 << 16]) as J:
        J.filter([seqs[0].scan(0), np.zeros((0, 3), np.float32), seqs[2].scan(0)])
        assert J.batched([1, 0, 1], [s.poses[0] for s in seqs]) == [LO_OK] * 3
        J.check([0, 2])
        before = J.dms[0].counts()
        assert before[0] > 1000
        counts = J.filter([np.full((64, 3), np.nan, np.float32), seqs[1].scan(2), seqs[2].scan(2)])
        assert counts[0] == 0 and counts[1] > 64
        # job 0 far away with a small radius: a non-empty scan there would prune the whole map
        far = np.eye(4)
        far[:3, 3] = [500.0, 0.0, 0.0]
        st = J.batched([1, 1, 1], [far, seqs[1].poses[2], seqs[2].poses[2]], host=False)
        J.host_update(2, seqs[2].poses[2])
        assert st == [LO_OK, LO_ERR_CAPACITY, LO_OK]
        assert J.dms[0].counts() == before
        assert J.dms[1].status() == LO_ERR_CAPACITY
        J.check([0, 2])
        assert J.b.maps_status([J.dms[0], None, J.dms[2]]) == [LO_OK] * 3      # a job without a map reports LO_OK
        assert J.b.maps_status(J.dms) == [LO_OK, LO_ERR_CAPACITY, LO_OK]
        # a map of another context in a job's place is refused
        with pytest.raises(RuntimeError, match=str(LO_ERR_ARG)):
            J.b.update_maps([J.dms[2], J.dms[1], J.dms[0]], [1, 1, 1], [s.poses[2] for s in seqs], RADIUS)


def test_back_to_back_updates_across_a_table_replacement():
    """Two batched updates with nothing waiting for the batch stream in between (the second inserts the same filtered
    scans again, at the next frame's poses) and job 0's table replaced between them by an unrelated upload: the
    emptying and the refill on the context stream are ordered behind the first update and before the second."""
    from lidar_odometry_amd.voxelmap import voxel_filter
    seqs = _seqs((7, 9), 6)
    with Jobs([1 << 16, 1 << 16]) as J:
        J.filter([s.scan(0) for s in seqs])
        assert J.batched([1, 1], [s.poses[0] for s in seqs]) == [LO_OK, LO_OK]
        J.filter([s.scan(2) for s in seqs])
        assert J.batched([1, 1], [s.poses[2] for s in seqs], wait=False) is None
        J.ctxs[0].set_surfels(np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
        assert J.batched([1, 1], [s.poses[3] for s in seqs]) == [LO_OK, LO_OK]
        J.check()
        for j, s in enumerate(seqs):
            J.check_lookups(j, voxel_filter(s.scan(5), 0.5, 8), [s.poses[5]])


def test_kdtree_mode_batch_updates_the_l0_containers():
    """A KDTree-mode batch of 2 (compute_surfels = False: no surfel decisions, no planarity erases): every map equals the
    host map (L0 order and centroids, counts, no surfels), and job 0's whole containers -- L0 keys and point counts, L1
    keys, child counts and children -- equal a KDTree-mode map updated by the single call."""
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer, lib
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap
    seqs = _seqs((7, 9), 9)
    S = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False), max_points=MAXP)
    sm = DeviceVoxelMap(S, 0.5, 3, 0.1, max_l0=1 << 16, max_points=MAXP)
    try:
        with Jobs([1 << 16, 1 << 16], kdtree=True) as J:
            for k in range(0, 9, 2):
                raws = [s.scan(k) for s in seqs]
                J.filter(raws)
                S.voxel_filter(raws[0], 0.5, 8)
                assert J.batched([1, k != 4], [s.poses[k] for s in seqs]) == [LO_OK, LO_OK]
                p = pose12(seqs[0].poses[k])
                assert lib().lo_devmap_update_from_scan(sm._h, p.ctypes.data_as(C.POINTER(C.c_float)), RADIUS) == LO_OK
                J.check()
                assert all(vm.surfel_count() == 0 for vm in J.vms)
                same_device_maps(J.dms[0], sm)
            assert J.dms[0].counts()[0] > 1000
    finally:
        sm.close()
        S.close()
