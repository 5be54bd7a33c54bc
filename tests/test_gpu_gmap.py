"""GPU global-map builder (include/lo_gmap.h, csrc/lo_gmap.hip) against the numpy fp32 restatement of
Estimator::save_map_to_ply's arithmetic (tests/_gmap_ref.py): transform_point_cloud, VoxelGrid::filter's sequential
running average per voxel in input order, std::map key order.  Every comparison is bit for bit and every count exact;
no tolerance is involved."""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import _lib, synth
from tests import _data
from tests import _gmap_ref as ref

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def icp():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 17)
    yield o
    o.close()


@pytest.fixture()
def gm(icp):
    from lidar_odometry_amd import GlobalMapBuilder
    g = GlobalMapBuilder(icp, max_points=1 << 15, max_keyframes=16)
    yield g
    g.close()


def _pose(w, t):
    return synth.se3(synth.exp_so3(w), t)[:3].astype(np.float32)


POSES_A = np.stack([_pose([0.3, -0.2, 0.9], [1.5, -2.25, 0.4]), _pose([-0.6, 0.1, -1.4], [-3.1, 0.7, -0.9]),
                    _pose([0.05, 0.8, 2.6], [-0.8, -1.9, 1.3]), _pose([-1.1, -0.4, 0.2], [2.7, 3.3, -0.35]),
                    _pose([0.7, 0.5, -2.2], [-1.2, 2.4, 0.6])])
POSES_B = np.stack([_pose([0.1, 0.2, -0.5], [0.3, 0.9, -0.2]), _pose([0.9, -0.7, 0.4], [2.2, -1.7, 0.8]),
                    _pose([-0.3, 0.3, 1.1], [-2.6, 0.2, 0.1]), _pose([0.2, -0.9, -0.8], [1.1, 1.6, -1.4]),
                    _pose([-0.8, 0.6, 3.0], [-0.4, -2.8, 0.5])])
SIZES = (0, 1, 700, 2049, 513)        # empty, one point, < one 1,024-point chunk, two chunks + 1, two 256-lane rounds + 1


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(21)
    return [(rng.uniform(-1.0, 1.0, (n, 3)) * [4.0, 4.0, 1.0]).astype(np.float32) for n in SIZES]


@pytest.fixture(scope="module")
def want_a(clouds):
    """The restatement of the main case, computed once."""
    world = ref.world_cloud(clouds, POSES_A)
    out, order = ref.voxel_grid(world, 0.5)
    return world, out, order


def _fill(g, clouds):
    for k, c in enumerate(clouds):
        g.add_keyframe(10 + k, c)
    return g


def _one_voxel_run():
    """World points: 300 in voxel (3, -2, 0) of leaf 0.5 split over three keyframes, among 400 one-point voxels."""
    rng = np.random.default_rng(0)
    run = (np.array([1.5, -1.0, 0.0]) + rng.uniform(0.01, 0.49, (300, 3))).astype(np.float32)
    cells = rng.permutation(40 * 40)[:400]
    lone = np.stack([cells // 40 - 20, cells % 40 - 20, np.full(400, 3)], 1)
    lone = ((lone + rng.uniform(0.1, 0.9, (400, 3))) * 0.5).astype(np.float32)
    parts = [np.concatenate([run[:120], lone[:150]]), np.concatenate([lone[150:300], run[120:130]]),
             np.concatenate([run[130:], lone[300:]])]
    return run, parts


IDENT = np.tile(np.eye(4, dtype=np.float32)[:3].reshape(1, 12), (3, 1))


# ---------------------------------------------------------------------------------------------------- parity
def test_main_case_equals_the_restatement(gm, clouds, want_a):
    _fill(gm, clouds)
    assert len(gm) == 5 and gm.points == sum(SIZES)
    world, want, order = want_a
    assert len(world) == sum(SIZES) and 300 < len(want) < len(world)
    got = gm.build(POSES_A, 0.5)
    ref.assert_bits_equal(got, want)
    ptr, n = gm.device_points()
    assert ptr != 0 and n == len(want)


def test_long_run_across_keyframes_and_one_point_voxels(gm):
    run, parts = _one_voxel_run()
    for k, p in enumerate(parts):
        gm.add_keyframe(k, p)
    world = ref.world_cloud(parts, IDENT)
    want, order = ref.voxel_grid(world, 0.5)
    assert len(want) == 401 and order.count((3, -2, 0)) == 1
    got = gm.build(IDENT, 0.5)
    ref.assert_bits_equal(got, want)
    # the long run's centroid is the sequential average of its 300 points in insertion order, and no other order's
    i = order.index((3, -2, 0))
    seq, _ = ref.voxel_grid(run, 0.5)
    rev, _ = ref.voxel_grid(run[::-1], 0.5)
    ref.assert_bits_equal(got[i:i + 1], seq)
    assert (ref.bits(rev) != ref.bits(seq)).any()


def test_signed_key_order(gm):
    k = np.array([-3, -1, 0, 2])
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(3)
    pts = ((g + 0.5) * 0.5).astype(np.float32)[rng.permutation(len(g))]
    gm.add_keyframe(0, pts[:40])
    gm.add_keyframe(1, pts[40:])
    want, order = ref.voxel_grid(ref.world_cloud([pts[:40], pts[40:]], IDENT), 0.5)
    assert order == sorted(map(tuple, g.tolist())) and order[0] == (-3, -3, -3) and order[-1] == (2, 2, 2)
    got = gm.build(IDENT[:2], 0.5)
    ref.assert_bits_equal(got, want)
    assert [tuple(r) for r in ref.keys(got, 0.5).tolist()] == order


def test_voxel_size_zero_is_the_transformed_concatenation(gm, clouds, want_a):
    _fill(gm, clouds)
    for leaf in (0.0, -1.0):
        ref.assert_bits_equal(gm.build(POSES_A, leaf), want_a[0])


def test_rebuild_with_other_poses(icp, gm, clouds, want_a):
    from lidar_odometry_amd import GlobalMapBuilder
    _fill(gm, clouds)
    first = gm.build(POSES_A, 0.5)
    second = gm.build(POSES_B, 0.5)
    fresh = GlobalMapBuilder(icp, max_points=1 << 12, max_keyframes=5)
    try:
        ref.assert_bits_equal(second, _fill(fresh, clouds).build(POSES_B, 0.5))
    finally:
        fresh.close()
    ref.assert_bits_equal(second, ref.voxel_grid(ref.world_cloud(clouds, POSES_B), 0.5)[0])
    assert second.shape != first.shape or (ref.bits(second) != ref.bits(first)).any()
    ref.assert_bits_equal(gm.build(POSES_A, 0.5), first)
    ref.assert_bits_equal(first, want_a[1])


def test_leaf_sizes(gm, clouds):
    _fill(gm, clouds)
    world = ref.world_cloud(clouds, POSES_B)
    for leaf in (0.2, 0.4):
        ref.assert_bits_equal(gm.build(POSES_B, leaf), ref.voxel_grid(world, leaf)[0])


# ---------------------------------------------------------------------------------------------------- inputs
def test_device_tensor_input_equals_host(icp, gm, clouds, want_a):
    import torch
    for k, c in enumerate(clouds):
        gm.add_keyframe(k, torch.from_numpy(c).cuda())
    ref.assert_bits_equal(gm.build(POSES_A, 0.5), want_a[1])


def test_add_from_scan_equals_the_host_copy(icp, gm):
    rng = np.random.default_rng(8)
    raw = (rng.uniform(-1.0, 1.0, (20000, 3)) * [25.0, 25.0, 2.0]).astype(np.float32)
    first = icp.voxel_filter(raw, 0.5, stride=2)
    assert 1000 < len(first) < 10000
    gm.add_from_scan(0)
    second = icp.voxel_filter(raw[::-1].copy(), 0.5, stride=3)
    gm.add_from_scan(1)
    ref.assert_bits_equal(icp.filtered_points(), second)
    gm.add_keyframe(2, first)                              # the host copy of keyframe 0
    assert gm.points == 2 * len(first) + len(second)
    poses = POSES_A[:3]
    ref.assert_bits_equal(gm.build(poses, 0.0), ref.world_cloud([first, second, first], poses))
    ref.assert_bits_equal(gm.build(poses, 0.5), ref.voxel_grid(ref.world_cloud([first, second, first], poses), 0.5)[0])


# ---------------------------------------------------------------------------------------------------- return codes
def test_capacity_limits_leave_the_builder_unchanged(icp):
    from lidar_odometry_amd import GlobalMapBuilder
    L = _lib.lib()
    rng = np.random.default_rng(4)
    a, b = (rng.uniform(-3.0, 3.0, (n, 3)).astype(np.float32) for n in (600, 100))
    g = GlobalMapBuilder(icp, max_points=1000, max_keyframes=2)
    try:
        g.add_keyframe(0, a)
        assert L.lo_gmap_add_keyframe(g._h, 1, a.ctypes.data, len(a), 0) == _lib.LO_ERR_CAPACITY     # 1,200 points
        assert (len(g), g.points) == (1, 600)
        with pytest.raises(RuntimeError):
            g.add_keyframe(1, a)
        g.add_keyframe(1, b)
        assert L.lo_gmap_add_keyframe(g._h, 2, b.ctypes.data, 1, 0) == _lib.LO_ERR_CAPACITY          # a third keyframe
        assert L.lo_gmap_add_keyframe(g._h, 2, b.ctypes.data, 0, 0) == _lib.LO_ERR_CAPACITY
        assert (len(g), g.points) == (2, 700)
        ref.assert_bits_equal(g.build(POSES_A[:2], 0.5), ref.voxel_grid(ref.world_cloud([a, b], POSES_A[:2]), 0.5)[0])
        g.clear()
        assert (len(g), g.points) == (0, 0)
        g.add_keyframe(5, b)
        ref.assert_bits_equal(g.build(POSES_B[:1], 0.5), ref.voxel_grid(ref.world_cloud([b], POSES_B[:1]), 0.5)[0])
    finally:
        g.close()


def test_wrong_pose_count_and_empty_builder(gm, clouds):
    L = _lib.lib()
    n = C.c_size_t(7)
    P = np.ascontiguousarray(POSES_A.reshape(-1, 12))
    assert L.lo_gmap_build(gm._h, P.ctypes.data_as(FP), 0, 0.5, C.byref(n)) == _lib.LO_INSUFFICIENT   # no keyframe
    assert n.value == 0 and len(gm.build(np.zeros((0, 12)), 0.5)) == 0
    gm.add_keyframe(0, clouds[0])                                      # a keyframe without points
    assert L.lo_gmap_build(gm._h, P.ctypes.data_as(FP), 1, 0.5, C.byref(n)) == _lib.LO_INSUFFICIENT
    assert L.lo_gmap_download(gm._h, None, 0) == _lib.LO_ERR_STATE
    gm.add_keyframe(1, clouds[2])
    for bad in (1, 3):
        assert L.lo_gmap_build(gm._h, P.ctypes.data_as(FP), bad, 0.5, C.byref(n)) == _lib.LO_ERR_ARG
    with pytest.raises(RuntimeError):
        gm.build(POSES_A[:3], 0.5)
    assert L.lo_gmap_build(gm._h, P.ctypes.data_as(FP), 2, 0.5, C.byref(n)) == _lib.LO_OK
    assert n.value == L.lo_gmap_download(gm._h, None, 0) > 0


@pytest.mark.parametrize("bad, count", [(3e6, 1), (np.nan, 2)])
def test_points_outside_the_key_range_are_refused(gm, clouds, bad, count):
    L = _lib.lib()
    c = clouds[2].copy()
    c[5, 1] = bad
    if count == 2:
        c[699, 2] = np.inf
    gm.add_keyframe(0, clouds[4])
    gm.add_keyframe(1, c)
    P = np.ascontiguousarray(IDENT[:2])
    n = C.c_size_t(7)
    assert L.lo_gmap_build(gm._h, P.ctypes.data_as(FP), 2, 0.5, C.byref(n)) == _lib.LO_ERR_ARG
    assert n.value == 0
    text = L.lo_gmap_last_error(gm._h).decode()
    assert text.startswith(f"{count} of {len(c) + len(clouds[4])} ")
    assert L.lo_gmap_download(gm._h, None, 0) == _lib.LO_ERR_STATE     # no result
    if count == 1:                                                     # the limit is on the key: 3e6 / 4 < 2^20
        ref.assert_bits_equal(gm.build(P, 4.0), ref.voxel_grid(ref.world_cloud([clouds[4], c], P), 4.0)[0])


def test_add_from_scan_without_a_scan_is_a_state_error():
    from lidar_odometry_amd import GlobalMapBuilder, IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=4096)
    g = GlobalMapBuilder(o, max_points=4096, max_keyframes=2)
    try:
        assert _lib.lib().lo_gmap_add_from_scan(g._h, 0) == _lib.LO_ERR_STATE
        assert len(g) == 0
    finally:
        g.close()
        o.close()


# ---------------------------------------------------------------------------------------------------- PLY
def test_save_ply_round_trip(gm, clouds, want_a, tmp_path):
    _fill(gm, clouds)
    got = gm.build(POSES_A, 0.5)
    path = tmp_path / "maps" / "map.ply"
    gm.save_ply(path)
    L = _lib.lib()
    n = L.lo_load_ply(str(path).encode(), None, 0)
    assert n == len(got)
    back = np.zeros((n, 3), np.float32)
    assert L.lo_load_ply(str(path).encode(), back.ctypes.data_as(FP), n) == n
    ref.assert_bits_equal(back, got)
    ref.assert_bits_equal(back, want_a[1])


# ---------------------------------------------------------------------------------------------------- end to end
def test_sequence_end_to_end(icp):
    """Six scans of the synthetic street through the device filter + ICP; their feature clouds, taken on the device,
    at their ICP poses make the map the restatement makes from the host copies."""
    from lidar_odometry_amd import GlobalMapBuilder
    frames = (11, 13, 15, 17, 19, 21)
    g = GlobalMapBuilder(icp, max_points=1 << 16, max_keyframes=len(frames))
    try:
        feats, poses = [], []
        for f in frames:
            m, _, Ti, _ = _data.kitti_case(f)
            if not feats:
                icp.set_surfels(*_data.surfels(m))
            ok, T = icp.optimize_raw(None, _data.kitti_scan(f), Ti, stride=8, voxel_size=0.5)
            assert ok
            g.add_from_scan(f)
            feats.append(icp.filtered_points())
            poses.append(np.asarray(T, np.float32).reshape(3, 4))
        assert g.points == sum(len(c) for c in feats) > 6000
        world = ref.world_cloud(feats, poses)
        want, _ = ref.voxel_grid(world, 0.5)
        assert len(want) < 0.8 * len(world)                    # the scans overlap: voxels hold several keyframes' points
        ref.assert_bits_equal(g.build(np.stack(poses), 0.5), want)
    finally:
        g.close()
