"""Every handle gives back the device and pinned memory it took (lo_debug_live_bytes, csrc/lo_buf.h).

Each cycle makes handles, drives them through the smallest shapes that reach every buffer grow path, and destroys
them; the library's count of live bytes must then be what it was before the cycle.  The count covers this process's
own buffers only, so other jobs on a shared GPU cannot move it.  Each cycle runs twice (the second pass would show a
leak that a first-use allocation hides), and while the handles live the count must be above the baseline.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _live():
    from lidar_odometry_amd import lib
    return int(lib().lo_debug_live_bytes())


def _lattice():
    """The 1,728-point three-plane lattice of test_device_grid_tie_reruns_with_kd_order and its 600-point scan."""
    g = np.arange(-12, 12) * 0.5 + 0.25
    A2, B2 = np.meshgrid(g, g)
    a, b = A2.ravel(), B2.ravel()
    c = np.full(a.size, 0.25)
    world = np.ascontiguousarray(np.concatenate([np.stack([a, b, c - 3.0], 1), np.stack([c + 3.0, a, b], 1),
                                                 np.stack([a, c + 3.0, b], 1)]), dtype=np.float32)
    rng = np.random.default_rng(3)
    scan = world[rng.choice(len(world), 600, replace=False)] + np.float32(0.25) * np.array([1, 0, 0], np.float32)
    T0 = np.eye(3, 4, dtype=np.float32)
    T0[:, 3] = [0.02, -0.01, 0.01]
    return world, np.ascontiguousarray(scan, dtype=np.float32), T0


@pytest.fixture(scope="module")
def surfel_scene():
    """A small planar-patch scene: its surfels (keys, normals, centroids) and a sampler of scans in it."""
    import oracle
    from lidar_odometry_amd import synth
    sc = synth.patch_scene(n_patches=40, seed=5, extent=12.0)
    vm = oracle.VoxelMap(0.5, 3, 0.1, True)
    vm.update(synth.sample_patches(sc, 30000, 4, outlier_frac=0.0), np.zeros(3), 1e3, True)
    k, n, c, _ = vm.surfels()
    T = synth.se3(synth.rot_z(0.05), [0.2, -0.1, 0.05])
    Ti = np.ascontiguousarray(T[:3], dtype=np.float32)

    def scan(count, seed):
        return np.ascontiguousarray(synth.transform(np.linalg.inv(T), synth.sample_patches(sc, count, seed)), np.float32)
    return (k, n, c), Ti, scan


def _twice(cycle):
    for _ in range(2):
        base = _live()
        cycle(base)
        assert _live() == base


def test_kdtree_context_with_device_map_returns_its_memory():
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer, lib
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap
    world, scan, T0 = _lattice()
    assert len(world) == 1728 and len(scan) == 600

    def cycle(base):
        icp = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False), max_points=4096)
        dm = DeviceVoxelMap(icp, 0.5, 3, 0.1, max_l0=1 << 14, max_points=1 << 14)
        try:
            dm.update(world, np.zeros(3), 1000.0, True)
            assert lib().lo_devmap_sync_points(dm._h) == 0      # the device-built grid and its scratch
            icp.optimize(None, scan, T0)
            assert _live() > base
        finally:
            dm.close()
            icp.close()
    _twice(cycle)


def test_surfel_context_returns_its_memory(surfel_scene):
    from lidar_odometry_amd import IterativeClosestPointOptimizer, lib
    (k, n, c), Ti, scan = surfel_scene
    raw, big, small = scan(4000, 11), scan(17000, 12), scan(1500, 13)

    def cycle(base):
        icp = IterativeClosestPointOptimizer(max_points=1 << 15)
        try:
            icp.set_surfels(k, n, c)
            after_create = _live()
            assert after_create > base
            icp.optimize_raw(None, raw, Ti, stride=2, voxel_size=0.5)      # raw staging + the filter's buffers
            icp.optimize(None, big, Ti)              # > 16384 points: column-sum records, residual sort scratch
            icp.find_correspondences(small, Ti)      # the parity hooks' residual buffers
            assert lib().lo_set_stage_timing(icp.ctx, 1) == 0             # the span stamps
            icp.optimize(None, small, Ti)
            assert _live() > after_create
        finally:
            icp.close()
    _twice(cycle)


def test_batch_iris_and_gmap_return_their_memory(surfel_scene):
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    from lidar_odometry_amd.gmap import GlobalMapBuilder
    from lidar_odometry_amd.icp import BatchOptimizer
    from lidar_odometry_amd.iris import IrisLoopDetector
    (k, n, c), Ti, scan = surfel_scene
    kf = [scan(500, 21), scan(500, 22)]
    poses = np.stack([np.eye(3, 4, dtype=np.float32)] * 2)

    def cycle(base):
        ctxs = [IterativeClosestPointOptimizer(max_points=4096) for _ in range(2)]
        handles = []
        try:
            for o in ctxs:
                o.set_surfels(k, n, c)
            with_ctxs = _live()
            b = BatchOptimizer(ctxs)
            handles.append(b)
            assert _live() > with_ctxs
            b.optimize(None, kf, [Ti, Ti])
            before_iris = _live()
            d = IrisLoopDetector(ctxs[0], capacity=8)
            handles.append(d)
            d.add_keyframe(0, np.zeros(3), kf[0])
            assert _live() > before_iris
            before_gmap = _live()
            g = GlobalMapBuilder(ctxs[1], max_points=1 << 12, max_keyframes=4)
            handles.append(g)
            g.add_keyframe(0, kf[0])
            g.add_keyframe(1, kf[1])
            assert len(g.build(poses, 0.5)) > 0
            assert _live() > before_gmap
        finally:
            for h in reversed(handles):
                h.close()
            for o in ctxs:
                o.close()
    _twice(cycle)
