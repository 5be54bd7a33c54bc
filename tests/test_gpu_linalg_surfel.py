"""The device's three surfel-fit call sites against fp64 eigh (tests/_linalg_ref.py): lo_math.h surfel_fit /
jacobi_svd3 as compiled for the GPU in (a) DeviceVoxelMap.update (lo_devmap.hip dm_touched_one), (b)
DeviceVoxelMap.apply_transform's RecomputeAllSurfels (dm_recompute_one) and (c) k_surfel_fit, reached through a host
VoxelMap with set_device_fit and lo_map_sync_voxelmap.  tests/test_gpu_devmap.py pins these to the host's build of
the same header bit for bit; here each voxel's centroid, normal and planarity are held to derived fp32 bounds around
the fp64 mean, covariance and eigenvectors of the same points.  tests/test_linalg_ref.py is the CPU twin (it also
asserts the conditioning of the inputs).

Path (b) fits voxels with at least five children, as the reference's RecomputeAllSurfels does
(MIN_OCCUPIED_CHILDREN = 5) and as the host map and the oracle do: voxels inserted with three and four children have
no surfel before the transform and none after it.
"""
import ctypes as C

import numpy as np
import pytest

from tests import _linalg_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 14)
    yield o
    o.close()


def _devmap(icp, thr=2.0):
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap
    return DeviceVoxelMap(icp, L.VOXEL, L.FACTOR, thr, max_l0=1 << 15, max_points=1 << 14)


@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_devmap_update_fit(icp, family):
    ref = L.surfel_ref(family)
    dm = _devmap(icp)
    try:
        dm.update(ref.case.points, np.zeros(3), 1e6, True)
        assert dm.status() == 0
        got = dm.surfels()
    finally:
        dm.close()
    rows = L.check_surfels(ref, got, label=f"devmap update {family}")
    if family == "isotropic":
        L.check_threshold_side(ref, rows, got[3], label=family)


@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_devmap_recompute_fit(icp, family):
    case = L.surfel_case(family, True)
    assert len(case.small) == 8 and set(case.m[case.small]) == {3, 4}
    moved = case.moved(L.SHIFT)
    dm = _devmap(icp)
    try:
        dm.update(case.points, np.zeros(3), 1e6, True)
        before = dm.surfels()
        dm.apply_transform(L.shift_pose())
        assert dm.status() == 0
        after = dm.surfels()
        _, c0, pc = dm.l0()
    finally:
        dm.close()
    # the transform and the rehash were exact: the children are the translated points, one per cell
    assert np.all(pc == 1)
    np.testing.assert_array_equal(np.sort(c0.view(np.uint32).view("u4,u4,u4").ravel()),
                                  np.sort(moved.points.view(np.uint32).view("u4,u4,u4").ravel()))
    # check_surfels rejects a surfel on any voxel outside the reference's fitted set (the 3- and 4-child voxels)
    L.check_surfels(L.surfel_ref(family, True), before, label=f"devmap before {family}")
    L.check_surfels(L.surfel_ref(family, True, L.SHIFT), after, label=f"devmap recompute {family}")


def _sync(icp, vm):
    from lidar_odometry_amd import lib
    patched = C.c_int(0)
    rc = lib().lo_map_sync_voxelmap(icp.ctx, vm.handle, C.byref(patched))
    assert rc == 0, rc
    return patched.value


def _seed_cloud():
    """512 exactly planar five-point voxels away from every family's: the first sync uploads them whole, which sizes
    the context's table (four slots per surfel) with room for the families' 400 in-place patches."""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), -1).reshape(-1, 3)
    keys = 40 + 2 * g
    star = 0.75 + 0.375 * np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]])
    return keys, (keys[:, None, :] * L.L1 + star[None, :, :]).reshape(-1, 3).astype(np.float32)


def _fit_on_device(icp, points, thr):
    """A host map whose refits run in k_surfel_fit: the context mirrors the map after a first (full) sync, then the
    family's update records its fits as jobs and the next sync runs them on the device."""
    from lidar_odometry_amd.voxelmap import VoxelMap
    seed_keys, seed = _seed_cloud()
    vm = VoxelMap(L.VOXEL, L.FACTOR, thr, True)
    try:
        vm.update(seed, np.zeros(3), 1e6, True)
        assert vm.surfel_count() == len(seed_keys)
        assert _sync(icp, vm) == -1                                   # a full upload: the context now mirrors vm
        vm.set_device_fit(True)
        vm.update(points, np.zeros(3), 1e6, True)
        patched = _sync(icp, vm)
        k, n, c, pl = vm.surfels()
    finally:
        vm.close()
    own = ~np.all((k >= 40) & (k < 56), axis=1)
    assert (~own).sum() == len(seed_keys)
    return patched, (k[own], n[own], c[own], pl[own])


@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_surfel_fit_kernel(icp, family):
    ref = L.surfel_ref(family)
    patched, got = _fit_on_device(icp, ref.case.points, 2.0)
    assert patched >= len(ref.keys), patched                          # every voxel's fit went to the device
    rows = L.check_surfels(ref, got, label=f"k_surfel_fit {family}")
    if family == "isotropic":
        L.check_threshold_side(ref, rows, got[3], label=family)


@pytest.mark.parametrize("site", ["update", "kernel"])
def test_production_threshold_survivors(icp, site):
    """The near-isotropic family at the production threshold 0.1: the voxels that keep a surfel are the fp64
    set, apart from the voxels whose fp64 planarity is within the planarity bound of 0.1."""
    ref = L.surfel_ref("isotropic")
    if site == "update":
        dm = _devmap(icp, 0.1)
        try:
            dm.update(ref.case.points, np.zeros(3), 1e6, True)
            got = dm.surfels()
        finally:
            dm.close()
    else:
        _, got = _fit_on_device(icp, ref.case.points, 0.1)
    L.check_survivors(ref, got[0], label=site)
    L.check_surfels(ref, got, expect_all=False, label=f"{site} survivors")
