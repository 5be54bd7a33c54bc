"""Batched map correction (lo_batch_apply_transform; csrc/lo_devmap.hip k_dm_at_*_b, k_dm_recompute_b, k_dm_flag_b):
ApplyTransformAndRehash + RecomputeAllSurfels for the active jobs of a batch in the single call's nine launches.

Bar: after every call each job's device map equals its host VoxelMap (corrected with apply_transform only where the job
was active): L0 order and centroids, the counts, the surfels in L1 order, and the context table answers lookups like a
full upload of the host map.  Against the single call (lo_devmap_apply_transform on a twin) the L0 and L1 containers
are compared whole, children included.  Every equality is on bits.

Inputs: KittiLikeSequence seeds 7, 9, 11; keyframes at frames 0, 2, 4 (job 2: frames 0 and 2 only) through the
0.5 m / stride 8 filter into maps of 0.5, 3, 0.1; job j's correction is se3(rot_z(0.05 + 0.01 seed), [0.4, -0.3, 0.02]),
which merges about a fifth of each map's L0 voxels.  The raw scans are raycast once per session and never modified.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from lidar_odometry_amd import synth
from lidar_odometry_amd._lib import LO_ERR_ARG, LO_ERR_CAPACITY, LO_ERR_STATE, LO_OK
from tests.test_gpu_batch_map import MAXP, RADIUS, Jobs, _seqs, _snapshot, pose12, same_device_maps
from tests.test_gpu_devmap import _same_lookups

pytestmark = pytest.mark.gpu

SEEDS = (7, 9, 11)
FRAMES = (0, 2, 4, 5, 6)
KEYFRAMES = ((0, (1, 1, 1)), (2, (1, 1, 1)), (4, (1, 1, 0)))
CAPS = [1 << 16, 1 << 17, 1 << 15]


@functools.lru_cache(maxsize=None)
def _inputs():
    """(sequences, {frame: [raw scan per job]}), built once."""
    seqs = _seqs(SEEDS, 7)
    raws = {k: [np.ascontiguousarray(s.scan(k), dtype=np.float32) for s in seqs] for k in FRAMES}
    for v in raws.values():
        for a in v:
            a.setflags(write=False)
    return seqs, raws


def _corr(seed):
    return synth.se3(synth.rot_z(0.05 + 0.01 * seed), [0.4, -0.3, 0.02])


CORR = [_corr(s) for s in SEEDS]


def _c34(Cx):
    return np.ascontiguousarray(np.asarray(Cx)[:3], dtype=np.float32)


def _build(J, jobs=(0, 1, 2)):
    """The keyframes of KEYFRAMES into the device and the host maps of J (whose job i is sequence jobs[i])."""
    seqs, raws = _inputs()
    for k, act in KEYFRAMES:
        J.filter([raws[k][j] for j in jobs])
        st = J.batched([act[j] for j in jobs], [seqs[j].poses[k] for j in jobs])
        assert st == [LO_OK] * len(jobs)


def _correct(J, active, corr, wait=True):
    """One batched correction over the active jobs, and the host maps' apply_transform; returns maps_status."""
    for j, a in enumerate(active):
        if a:
            J.vms[j].apply_transform(_c34(corr[j]))
    J.b.apply_transform(J.dms, active, [_c34(c) for c in corr])
    return J.b.maps_status(J.dms) if wait else None


def _rec(r):
    """A batch record's fields as bits."""
    f32 = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    return (bool(r.success), np.asarray(r.pose, np.float32).reshape(12).view(np.uint32).tolist(), r.iterations,
            r.n_corr, f32(r.initial_cost), f32(r.final_cost), int(np.float64(r.alpha).view(np.uint64)))


def _counts(J):
    return [(v.l0_count(), v.l1_count(), v.surfel_count()) for v in J.vms]


def test_subsets_capacities_and_distinct_transforms():
    seqs, raws = _inputs()
    with Jobs(CAPS) as J:
        _build(J)
        J.check()
        before = _counts(J)
        moved = [np.eye(4)] * 3
        for act in ((1, 0, 1), (0, 1, 0)):
            idle = {j: _snapshot(J.dms[j]) for j in range(3) if not act[j]}
            assert _correct(J, act, CORR) == [LO_OK] * 3
            moved = [CORR[j] if act[j] else moved[j] for j in range(3)]
            J.check()
            for j in range(3):
                if act[j]:
                    J.check_lookups(j, J.clouds[j], [CORR[j] @ seqs[j].poses[4]])   # (frame 4 was filtered for all)
            for j, was in idle.items():
                for x, y in zip(was, _snapshot(J.dms[j])):
                    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
        after = _counts(J)
        for j in range(3):                                   # the correction merged voxels and kept surfels
            assert after[j][0] < before[j][0], (j, before[j], after[j])
            assert after[j][2] > 50, (j, after[j])
        J.filter(raws[6])
        assert J.batched([1, 1, 1], [moved[j] @ seqs[j].poses[6] for j in range(3)]) == [LO_OK] * 3
        J.check()


def test_batch_of_one_equals_the_single_call():
    from lidar_odometry_amd import IterativeClosestPointOptimizer, lib
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap, voxel_filter
    seqs, raws = _inputs()
    seq = seqs[0]
    S = IterativeClosestPointOptimizer(max_points=MAXP)
    sm = DeviceVoxelMap(S, 0.5, 3, 0.1, max_l0=1 << 16, max_points=MAXP)

    def both(k, T):
        J.filter([raws[k][0]])
        S.voxel_filter(raws[k][0], 0.5, 8)
        assert J.batched([1], [T]) == [LO_OK]
        p = pose12(T)
        assert lib().lo_devmap_update_from_scan(sm._h, p.ctypes.data_as(C.POINTER(C.c_float)), RADIUS) == LO_OK

    try:
        with Jobs([1 << 16]) as J:
            for k in (0, 2, 4):
                both(k, seq.poses[k])
            n0 = sm.counts()[0]
            assert _correct(J, [1], CORR[:1]) == [LO_OK]
            sm.apply_transform(_c34(CORR[0]))
            same_device_maps(J.dms[0], sm)
            assert sm.counts()[0] < n0 and sm.counts()[2] > 50
            J.check()
            scan = voxel_filter(raws[5][0], 0.5, 8)
            _same_lookups(J.ctxs[0], S, scan, [pose12(CORR[0] @ seq.poses[5])])
            both(6, CORR[0] @ seq.poses[6])
            same_device_maps(J.dms[0], sm)
            J.check()
    finally:
        sm.close()
        S.close()


def test_errors_stay_in_their_job():
    seqs, raws = _inputs()
    with Jobs(CAPS) as J:
        # empty maps, active (their contexts have not filtered a scan either): nothing changes
        assert _correct(J, [1, 1, 1], CORR) == [LO_OK] * 3
        assert [d.counts() for d in J.dms] == [(0, 0, 0)] * 3
        _build(J)
        # between optimize_async and result: refused, and the maps are as they were
        was = [_snapshot(d) for d in J.dms]
        counts = J.filter(raws[5])
        J.b.optimize_async([0] * 3, counts, [pose12(s.poses[5]) for s in seqs])
        with pytest.raises(RuntimeError, match=str(LO_ERR_STATE)):
            J.b.apply_transform(J.dms, [1, 1, 1], [_c34(c) for c in CORR])
        J.b.result()
        # a map of another context in a job's place
        with pytest.raises(RuntimeError, match=str(LO_ERR_ARG)):
            J.b.apply_transform([J.dms[2], J.dms[1], J.dms[0]], [1, 1, 1], [_c34(c) for c in CORR])
        assert J.b.maps_status(J.dms) == [LO_OK] * 3
        for a, d in zip(was, J.dms):
            for x, y in zip(a, _snapshot(d)):
                np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))
        # job 1 thrown 1e6 m away: its keys pass 2^20 at 0.5 m
        far = np.eye(4)
        far[:3, 3] = [1e6, 0.0, 0.0]
        for j in (0, 2):
            J.vms[j].apply_transform(_c34(CORR[j]))
        J.b.apply_transform(J.dms, [1, 1, 1], [_c34(CORR[0]), _c34(far), _c34(CORR[2])])
        assert J.b.maps_status(J.dms) == [LO_OK, LO_ERR_CAPACITY, LO_OK]
        assert J.dms[1].status() == LO_ERR_CAPACITY
        J.check([0, 2])
        for j in (0, 2):
            J.check_lookups(j, J.clouds[j], [CORR[j] @ seqs[j].poses[5]])


def test_back_to_back_and_across_a_table_replacement():
    seqs, raws = _inputs()
    with Jobs(CAPS) as J:
        _build(J)
        # update, correction, update with nothing waiting in between (the second update inserts the same filtered
        # scans again, at the next frame's corrected poses)
        J.filter(raws[5])
        assert J.batched([1, 1, 1], [s.poses[5] for s in seqs], wait=False) is None
        assert _correct(J, [1, 1, 1], CORR, wait=False) is None
        assert J.batched([1, 1, 1], [CORR[j] @ seqs[j].poses[6] for j in range(3)], wait=False) is None
        assert J.b.maps_status(J.dms) == [LO_OK] * 3
        J.check()
        # job 0's table replaced by an unrelated upload: the correction refills it first
        J.ctxs[0].set_surfels(np.zeros((1, 3), np.int32), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32))
        assert _correct(J, [1, 1, 1], CORR) == [LO_OK] * 3
        J.check()
        J.check_lookups(0, J.clouds[0], [CORR[0] @ CORR[0] @ seqs[0].poses[5]])
        # the single call on job 1 (the batch stream is idle: maps_status waited), the batched one on job 0
        J.vms[1].apply_transform(_c34(CORR[1]))
        J.dms[1].apply_transform(_c34(CORR[1]))
        assert _correct(J, [1, 0, 0], CORR) == [LO_OK] * 3
        J.check()
        for j in (0, 1):
            J.check_lookups(j, J.clouds[j], [CORR[j] @ CORR[j] @ CORR[j] @ seqs[j].poses[5]])
        assert min(c[2] for c in _counts(J)) > 50


def test_kdtree_batch_correction_then_sync_points():
    """A KDTree batch of 2: the batched correction followed by the batched grid build, against twins corrected and
    rebuilt by the single calls; the same batched optimize of frame 5 on both gives the same records."""
    from lidar_odometry_amd import lib
    from lidar_odometry_amd.voxelmap import voxel_filter
    seqs, raws = _inputs()
    L = lib()
    with Jobs(CAPS[:2], kdtree=True) as J, Jobs(CAPS[:2], kdtree=True) as W:
        for X in (J, W):
            _build(X, jobs=(0, 1))
            X.b.sync_points(X.dms)
            assert X.b.maps_status(X.dms) == [LO_OK] * 2
        assert _correct(J, [1, 1], CORR[:2], wait=False) is None
        J.b.sync_points(J.dms, [1, 1])
        assert J.b.maps_status(J.dms) == [LO_OK] * 2
        for j in range(2):
            W.vms[j].apply_transform(_c34(CORR[j]))
            W.dms[j].apply_transform(_c34(CORR[j]))
            W.dms[j].sync_points()
            same_device_maps(J.dms[j], W.dms[j])
            # what a KDTree context reads: the L0 centroids in order, against the host map.  (The surfels are left
            # out: the host map refits none at a correction when compute_surfels is off, the device map -- solo and
            # batched alike -- refits them all, as RecomputeAllSurfels does.)
            h0 = J.vms[j].l0_cloud()
            assert len(h0) > 1000
            np.testing.assert_array_equal(J.dms[j].l0()[1].view(np.uint32), h0.view(np.uint32))
        scans = [voxel_filter(raws[5][j], 0.5, 8) for j in range(2)]
        Ts = [pose12(CORR[j] @ seqs[j].poses[5]) for j in range(2)]
        got = J.b.optimize(None, scans, Ts)
        want = W.b.optimize(None, scans, Ts)
        for j in range(2):
            assert got[j].success and got[j].n_corr > 100
            assert _rec(got[j]) == _rec(want[j]), j
            assert L.lo_kd_reruns(J.ctxs[j].ctx) == L.lo_kd_reruns(W.ctxs[j].ctx)
