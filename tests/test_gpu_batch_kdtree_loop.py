"""The grids of a KDTree batch built together (lo_batch_sync_points; csrc/lo_grid.hip k_grid_*_b) and the frame loop for B
KDTree-mode sequences on top of it (lo_odom_batch_create_kdtree, BatchLidarOdometry.kdtree).

Bar: the single call.  After lo_batch_sync_points a context's grid (lo_debug_grid: cell edge, origin, dimensions, point
count, every cell start, every point) equals, as uint32 words, the grid lo_devmap_sync_points builds on a twin context
whose twin map received the same updates; the frame loop's poses, guesses, keyframe flags, iteration counts, filtered
counts, statuses and lo_kd_reruns equal a solo KDTree LidarOdometry's.  No tolerance anywhere.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from lidar_odometry_amd._lib import LO_ERR_ARG, LO_ERR_CAPACITY, LO_ERR_STATE, LO_OK
from tests.test_gpu_batch_kdtree import _assert_same, _kd, _of_batch
from tests.test_gpu_batch_map import MAXP, RADIUS, Jobs, _seqs, pose12
from tests.test_gpu_batch_odometry import MAX_L0, N_FRAMES, bits, sequences
from tests.test_gpu_batch_odometry import MAXP as ODOM_MAXP

pytestmark = pytest.mark.gpu


def grid(opt):
    """lo_debug_grid of an optimizer's context: every field as uint32 / int32 words."""
    from lidar_odometry_amd import lib
    L = lib()
    h, m = C.c_float(0), C.c_int(0)
    org, dim = (C.c_int * 3)(), (C.c_int * 3)()
    assert L.lo_debug_grid(opt.ctx, C.byref(h), org, dim, C.byref(m), None, 0, None, 0) == LO_OK
    ncell = dim[0] * dim[1] * dim[2]
    start = np.zeros(ncell + 1, np.uint32)
    pts = np.zeros((max(m.value, 1), 4), np.float32)
    assert L.lo_debug_grid(opt.ctx, C.byref(h), org, dim, C.byref(m), start.ctypes.data_as(C.POINTER(C.c_uint32)),
                           len(start), pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts)) == LO_OK
    return dict(h=np.float32(h.value).view(np.uint32), org=tuple(org), dim=tuple(dim), m=m.value, start=start,
                pts=pts[:m.value].view(np.uint32))


def same_grid(a, b, msg):
    assert (a["h"], a["org"], a["dim"], a["m"]) == (b["h"], b["org"], b["dim"], b["m"]), msg
    np.testing.assert_array_equal(a["start"], b["start"], err_msg=msg + ": start")
    np.testing.assert_array_equal(a["pts"], b["pts"], err_msg=msg + ": pts")


def sorted_by_cell(g):
    """The layout itself: start ends at m, and inside every cell the point indices ascend."""
    assert g["start"][0] == 0 and g["start"][-1] == g["m"] and np.all(np.diff(g["start"].astype(np.int64)) >= 0)
    idx = g["pts"][:, 3].astype(np.int64)
    assert sorted(idx.tolist()) == list(range(g["m"]))
    cell = np.searchsorted(g["start"], np.arange(g["m"]), side="right") - 1
    same = cell[1:] == cell[:-1]
    assert np.all(idx[1:][same] > idx[:-1][same])


class Twins:
    """One KDTree context + device map per job, fed through the single calls."""

    def __init__(self, max_l0s, max_points=MAXP):
        from lidar_odometry_amd.voxelmap import DeviceVoxelMap
        self.ctxs = [_kd(max_points) for _ in max_l0s]
        self.dms = [DeviceVoxelMap(c, 0.5, 3, 0.1, max_l0=m, max_points=max_points) for c, m in zip(self.ctxs, max_l0s)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for d in self.dms:
            d.close()
        for c in self.ctxs:
            c.close()

    def keyframe(self, j, raw, T):
        from lidar_odometry_amd import lib
        self.ctxs[j].voxel_filter(raw, 0.5, 8)
        p = pose12(T)
        assert lib().lo_devmap_update_from_scan(self.dms[j]._h, p.ctypes.data_as(C.POINTER(C.c_float)), RADIUS) == LO_OK


# ---------------------------------------------------------------- 1. grids equal the single call's
def test_grids_of_a_subset_and_of_all_jobs_equal_the_single_call():
    seqs = _seqs((7, 9, 11), 7)
    caps = [1 << 16] * 3
    with Jobs(caps, kdtree=True) as J, Twins(caps) as W:
        def keyframe(k):
            raws = [s.scan(k) for s in seqs]
            J.filter(raws)
            assert J.batched([1, 1, 1], [s.poses[k] for s in seqs], host=False) == [LO_OK] * 3
            for j, s in enumerate(seqs):
                W.keyframe(j, raws[j], s.poses[k])

        keyframe(0)
        J.dms[1].sync_points()                              # job 1 gets a grid of its own first (the single call)
        before = grid(J.ctxs[1])
        assert before["m"] > 1000
        keyframe(2)
        J.b.sync_points(J.dms, [1, 0, 1])
        for d in W.dms:
            d.sync_points()
        want = [grid(c) for c in W.ctxs]
        got = [grid(c) for c in J.ctxs]
        for j in (0, 2):
            same_grid(got[j], want[j], f"job {j}")
            sorted_by_cell(got[j])
            assert got[j]["m"] > 1000 and len(got[j]["start"]) > 1024
        same_grid(got[1], before, "inactive job 1")
        assert got[1]["m"] != want[1]["m"]                  # (its map did move on: the grid was not rebuilt)
        keyframe(4)
        J.b.sync_points(J.dms)                              # active = None: every job
        for j, d in enumerate(W.dms):
            d.sync_points()
            same_grid(grid(J.ctxs[j]), grid(W.ctxs[j]), f"all jobs: job {j}")


# ---------------------------------------------------------------- 2. / 3. edges, and the search on a batched grid
def _edge_clouds():
    rng = np.random.default_rng(12)
    three = np.array([[0.25, 0.25, 0.25], [3.25, -1.75, 0.75], [-2.25, 0.75, 5.25]], np.float32)
    # (c) ~3000 L0 voxels: more than one 1024-thread pass, no multiple of 256
    dense = (rng.integers(0, [80, 80, 10], size=(3200, 3)) * 0.5 + 0.25).astype(np.float32)
    # (d) 300 voxel centres over a 500 m cube (500^3 cells of 1 m exceed 2^26: the edge doubles to 2 m), and a block of
    # 4 x 4 x 3 adjacent voxels inside one 2 m cell
    far = (rng.integers(-500, 500, size=(300, 3)) * 0.5 + 0.25).astype(np.float32)
    far[0], far[1] = [-249.75, -249.75, -249.75], [249.75, 249.75, 249.75]
    blk = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    cluster = (blk * 0.5 + np.array([100.25, 100.25, 100.25])).astype(np.float32)
    spread = np.ascontiguousarray(np.concatenate([far[:150], cluster[::-1], far[150:]]))
    return [None, three, dense, spread]


def test_edge_maps_and_the_search_on_a_batched_grid():
    clouds = _edge_clouds()
    caps = [1 << 14] * 4
    with Jobs(caps, kdtree=True, max_points=1 << 14) as J, Twins(caps, 1 << 14) as W:
        for j, cl in enumerate(clouds):
            if cl is None:
                continue
            for d in (J.dms[j], W.dms[j]):
                d.update(cl, np.zeros(3), 1e4, True)
        counts = [d.counts()[0] for d in J.dms]             # (waits for every context stream: the batch may read the maps)
        assert counts[0] == 0 and counts[1] == 3
        assert 2500 <= counts[2] <= 4000 and counts[2] % 256 != 0 and counts[2] > 1024
        J.b.sync_points(J.dms, [1, 1, 1, 1])
        for d in W.dms:
            d.sync_points()
        got = [grid(c) for c in J.ctxs]
        for j in range(4):
            same_grid(got[j], grid(W.ctxs[j]), f"edge job {j}")
            sorted_by_cell(got[j])
        assert got[0]["m"] == 0 and got[0]["dim"] == (1, 1, 1) and got[0]["start"].tolist() == [0, 0]
        assert got[1]["m"] == 3
        one = np.float32(1.0).view(np.uint32)
        assert got[2]["h"] == one
        assert got[3]["h"] == np.float32(2.0).view(np.uint32)                   # doubled once
        assert np.diff(got[3]["start"].astype(np.int64)).max() >= 40            # ranks far beyond 8 in one cell
        # 3. the same answers from both grids
        rng = np.random.default_rng(5)
        q = (rng.uniform([0, 0, 0], [40, 40, 5], size=(500, 3))).astype(np.float32)
        ia, da, fa = J.ctxs[2].nearest_k_search(q)
        ib, db, fb = W.ctxs[2].nearest_k_search(q)
        np.testing.assert_array_equal(ia, ib)
        np.testing.assert_array_equal(da.view(np.uint32), db.view(np.uint32))
        assert fa.sum() > 0 and np.array_equal(fa, fb)


# ---------------------------------------------------------------- 4. ties on a batched grid
def test_ties_rerun_on_a_batched_grid_and_the_next_build_replaces_the_ordered_grid():
    """The lattice world and scan of test_device_grid_ties_rerun_inside_the_batch, the device context's grid built by
    lo_batch_sync_points: its job is run again with the host-built order (which leaves an ordered grid in the context);
    the next batched build replaces that grid, and the same optimize ties, re-runs and agrees again."""
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
    L = lib()
    try:
        dm.update(world, np.zeros(3), 1000.0, True)
        assert dm.status() == LO_OK                         # (waits for the context stream)
        hv = VoxelMap(0.5, 3, 0.1, False)
        hv.update(world, np.zeros(3), 1000.0, True)
        host.set_map_points(hv.l0_cloud())
        bt = BatchOptimizer([dev, host])
        try:
            first = None
            for rnd in range(2):
                r0 = L.lo_kd_reruns(dev.ctx)
                bt.sync_points([dm, None], [1, 0])
                res = bt.optimize(None, [scan, scan], [T0, T0])
                _assert_same(res[0], _of_batch(res[1]), f"round {rnd}: batched device grid vs host grid")
                assert L.lo_kd_reruns(dev.ctx) >= r0 + 1, rnd
                if first is None:
                    first = _of_batch(res[0])
                _assert_same(res[0], first, f"round {rnd}")
            assert L.lo_kd_reruns(host.ctx) == 0
        finally:
            bt.close()
    finally:
        dm.close()
        dev.close()
        host.close()


# ---------------------------------------------------------------- 5. the frame loop
@functools.lru_cache(maxsize=None)
def solo(j, exact, n=N_FRAMES, first_empty=False):
    """Sequence j through a solo KDTree LidarOdometry: ([(pose, info)], lo_kd_reruns).  Run once per case."""
    from lidar_odometry_amd.odometry import LidarOdometry
    raws, T0 = sequences()[j]
    feed = [np.full((16, 3), np.nan, np.float32) if (first_empty and k == 0) else raws[k] for k in range(n)]
    os.environ["LO_DEVMAP_MAX_L0"] = str(MAX_L0)
    try:
        od = LidarOdometry(max_points=ODOM_MAXP, initial_pose=T0, exact=exact, use_surfel_correspondence=False)
    finally:
        del os.environ["LO_DEVMAP_MAX_L0"]
    try:
        out = [od.process(r) for r in feed]
        od.flush()
        return out, od.kd_reruns
    finally:
        od.close()


def same_frames(got, j, ref, msg):
    for k, (T, info) in enumerate(ref):
        Tb, ib = got[k][0][j], got[k][1][j]
        m = f"{msg} sequence {j} frame {k}"
        np.testing.assert_array_equal(bits(Tb), bits(T), err_msg=m)
        np.testing.assert_array_equal(bits(ib.guess), bits(info.guess), err_msg=m)
        assert (ib.keyframe, ib.icp_iterations, ib.n_filtered, ib.status) == \
               (info.keyframe, info.icp_iterations, info.n_filtered, info.status), m


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_every_kdtree_sequence_equals_its_solo_frame_loop(exact):
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    seqs = sequences()
    bo = BatchLidarOdometry.kdtree(len(seqs), max_points=ODOM_MAXP, initial_poses=[T0 for _, T0 in seqs], exact=exact,
                                   max_l0=MAX_L0)
    try:
        got = [bo.process([raws[k] for raws, _ in seqs]) for k in range(N_FRAMES)]
        bo.flush()
        kfs = [bo.keyframes(j) for j in range(len(seqs))]
        reruns = [bo.kd_reruns(j) for j in range(len(seqs))]
    finally:
        bo.close()
    for j in range(len(seqs)):
        ref, ref_reruns = solo(j, exact)
        flags = [i.keyframe for _, i in ref]
        assert sum(flags) >= 3 and not all(flags[1:]), flags            # several keyframes, some frames without
        assert kfs[j] == sum(flags)
        assert reruns[j] == ref_reruns
        same_frames(got, j, ref, "exact" if exact else "fast")
        assert any(i.status == LO_OK and i.icp_iterations > 0 for _, i in ref[1:])


def test_empty_first_scan_beside_a_tracking_kdtree_sequence():
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    (raws_a, Ta), (raws_b, Tb), _ = sequences()
    empty = np.full((16, 3), np.nan, np.float32)
    n = 5
    feed = [[raws_a[k], empty if k == 0 else raws_b[k]] for k in range(n)]
    bo = BatchLidarOdometry.kdtree(2, max_points=ODOM_MAXP, initial_poses=[Ta, Tb], max_l0=MAX_L0)
    try:
        got = [bo.process(f) for f in feed]
        assert bo.keyframes(1) == 0 and bo.keyframes(0) >= 1
    finally:
        bo.close()
    same_frames(got, 0, solo(0, True)[0][:n], "tracking")
    same_frames(got, 1, solo(1, True, n, True)[0], "empty first scan")
    assert all(not got[k][1][1].keyframe and got[k][1][1].icp_iterations == 0 for k in range(n))


# ---------------------------------------------------------------- 6. refusals
def test_refusals():
    from lidar_odometry_amd import lib, odometry
    from lidar_odometry_amd._lib import LoOdomConfig
    L = lib()
    act = (C.c_uint8 * 2)(1, 1)
    with Jobs([1 << 12, 1 << 12], max_points=4096) as S:    # a surfel-mode batch
        assert L.lo_batch_sync_points(S.b._b, S.b._map_handles(S.dms), act) == LO_ERR_STATE
        with pytest.raises(RuntimeError, match=str(LO_ERR_STATE)):
            S.b.sync_points(S.dms)
        h, m = C.c_float(0), C.c_int(0)
        assert L.lo_debug_grid(S.ctxs[0].ctx, C.byref(h), None, None, C.byref(m), None, 0, None, 0) == LO_ERR_STATE
    with Jobs([1 << 12, 1 << 12], kdtree=True, max_points=4096) as K:
        swapped = [K.dms[1], K.dms[0]]
        assert L.lo_batch_sync_points(K.b._b, K.b._map_handles(swapped), act) == LO_ERR_ARG
        before = grid(K.ctxs[0])
        assert L.lo_batch_sync_points(K.b._b, K.b._map_handles([None, K.dms[1]]), (C.c_uint8 * 2)(0, 1)) == LO_OK
        same_grid(grid(K.ctxs[0]), before, "inactive job without a map")
        K.b.optimize_async([0, 0], [0, 0], [np.eye(3, 4, dtype=np.float32)] * 2)
        assert L.lo_batch_sync_points(K.b._b, K.b._map_handles(K.dms), act) == LO_ERR_STATE     # optimize pending
        K.b.result()
        # lo_debug_grid's caps
        K.dms[0].update(np.array([[0.25, 0.25, 0.25], [5.25, 0.25, 0.25]], np.float32), np.zeros(3), 1e3, True)
        assert K.dms[0].status() == LO_OK
        K.b.sync_points(K.dms, [1, 0])
        h, m = C.c_float(0), C.c_int(0)
        st = np.zeros(1, np.uint32)
        assert L.lo_debug_grid(K.ctxs[0].ctx, C.byref(h), None, None, C.byref(m), st.ctypes.data_as(C.POINTER(C.c_uint32)),
                               1, None, 0) == LO_ERR_CAPACITY
        assert m.value == 2
    # the KDTree constructor on a surfel config: in C, and through the class the classmethod returns
    cfg = LoOdomConfig()
    L.lo_odom_config_default_kitti(C.byref(cfg))
    assert cfg.icp.use_surfel_correspondence == 1
    err = C.c_int(0)
    assert not L.lo_odom_batch_create_kdtree(C.byref(cfg), 2, 0, 1 << 12, C.byref(err))
    assert err.value == LO_ERR_ARG
    with pytest.raises(ValueError, match="KDTree mode only.*-1"):
        odometry._KdtreeBatchLidarOdometry(2, max_points=4096, use_surfel_correspondence=True)
    with pytest.raises(TypeError):
        odometry.BatchLidarOdometry.kdtree(2, use_surfel_correspondence=True)


# ---------------------------------------------------------------- 7. overflow
def test_overflowing_maps_in_the_kdtree_loop_and_in_the_batched_build():
    """max_l0 = 64: the first keyframes overflow every map and abort.  The loop's first call returns what the solo
    loop's does and flush() reports -3; lo_batch_sync_points on such a map returns what lo_devmap_sync_points returns on
    a twin and builds the same (clamped) grid, and the job beside it is exact."""
    from lidar_odometry_amd import lib
    from lidar_odometry_amd.odometry import BatchLidarOdometry, LidarOdometry
    (raws_a, Ta), (raws_b, Tb), _ = sequences()
    os.environ["LO_DEVMAP_MAX_L0"] = "64"
    try:
        od = LidarOdometry(max_points=ODOM_MAXP, initial_pose=Ta, use_surfel_correspondence=False)
    finally:
        del os.environ["LO_DEVMAP_MAX_L0"]
    try:
        od.process(raws_a[0])                               # the single calls accept the aborted map's grid build
        with pytest.raises(RuntimeError, match="-3"):
            od.flush()
    finally:
        od.close()
    bo = BatchLidarOdometry.kdtree(2, max_points=ODOM_MAXP, initial_poses=[Ta, Tb], max_l0=64)
    try:
        bo.process([raws_a[0], raws_b[0]])
        with pytest.raises(RuntimeError, match="-3"):
            bo.flush()
    finally:
        bo.close()
    L = lib()
    seqs = _seqs((7, 9), 1)
    caps = [1 << 16, 64]
    with Jobs(caps, kdtree=True) as J, Twins(caps) as W:
        raws = [s.scan(0) for s in seqs]
        J.filter(raws)
        assert J.batched([1, 1], [s.poses[0] for s in seqs], host=False) == [LO_OK, LO_ERR_CAPACITY]
        for j, s in enumerate(seqs):
            W.keyframe(j, raws[j], s.poses[0])
        want_rc = [L.lo_devmap_sync_points(d._h) for d in W.dms]
        assert want_rc[0] == LO_OK
        rc = L.lo_batch_sync_points(J.b._b, J.b._map_handles(J.dms), (C.c_uint8 * 2)(1, 1))
        assert rc == want_rc[1]
        for j in range(2):
            same_grid(grid(J.ctxs[j]), grid(W.ctxs[j]), f"job {j}")
        assert grid(J.ctxs[1])["m"] <= 64
