"""CPU twin of tests/test_gpu_linalg_*.py: the Eigen restatements against fp64 numpy (tests/_linalg_ref.py) through
the host entry points of the same source -- the host VoxelMap (lo_math.h surfel_fit / jacobi_svd3), the oracle's
KDTree correspondence (its smallest_eigvec3d, the twin of lo_kdtree.hip's) and the oracle's LDLT / SO3::Exp / SE3
product (the twins of lo_exact.h).  A failure here is the algorithm's; a failure of the GPU files alone points at the
device build.  The shares of well-conditioned inputs that the checks rely on are asserted here from fp64 alone, so a
generator change cannot quietly empty a check.
"""
import numpy as np
import pytest

import oracle
from lidar_odometry_amd.voxelmap import VoxelMap
from tests import _linalg_ref as L


# ---------------------------------------------------------------------------------------------- A. surfel fit
@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_surfel_input_conditions(family):
    L.surfel_input_conditions(family)


def _host_map(points, thr=2.0, defer=False):
    vm = VoxelMap(L.VOXEL, L.FACTOR, thr, True)
    if defer:
        vm.set_device_fit(True)
    vm.update(points, np.zeros(3), 1e6, True)
    return vm


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_host_surfel_fit_update(family, defer):
    """UpdateVoxelMap's fit (defer: recorded as jobs and fitted when the map is read, with no context to run them)."""
    ref = L.surfel_ref(family)
    vm = _host_map(ref.case.points, defer=defer)
    got = vm.surfels()
    rows = L.check_surfels(ref, got, label=f"host update {family}")
    if family == "isotropic":
        L.check_threshold_side(ref, rows, got[3], label=family)


@pytest.mark.parametrize("family", L.SURFEL_FAMILIES)
def test_host_surfel_fit_recompute(family):
    """RecomputeAllSurfels after an exact translation; voxels with three and four children never get a surfel (the
    reference's MIN_OCCUPIED_CHILDREN = 5 holds on this path too)."""
    case = L.surfel_case(family, True)
    assert len(case.small) == 8 and set(case.m[case.small]) == {3, 4}
    vm = _host_map(case.points)
    L.check_surfels(L.surfel_ref(family, True), vm.surfels(), label=f"host before {family}")
    vm.apply_transform(L.shift_pose())
    L.check_surfels(L.surfel_ref(family, True, L.SHIFT), vm.surfels(), label=f"host recompute {family}")


def test_host_production_threshold_survivors():
    ref = L.surfel_ref("isotropic")
    vm = _host_map(ref.case.points, thr=0.1)
    got = vm.surfels()
    L.check_survivors(ref, got[0], label="host")
    L.check_surfels(ref, got, expect_all=False, label="host survivors")


# ---------------------------------------------------------------------------------------------- B. plane fit
def _oracle_kd_map(cloud):
    m = oracle.VoxelMap(L.KD_VOXEL, 3, 0.1, False)
    m.update(cloud, np.zeros(3), 1e9, True)
    np.testing.assert_array_equal(m.l0_cloud(), cloud)              # GetPointCloud is the cloud, in its order
    return m


@pytest.mark.parametrize("which", ["identity", "perturbed"])
@pytest.mark.parametrize("family", L.PLANE_FAMILIES)
def test_oracle_plane_fit(family, which):
    L.plane_input_conditions(family, which)
    ref = L.plane_ref(family, which)
    m = _oracle_kd_map(ref.case.cloud)
    idx, _, found = oracle.kdtree_knn5(ref.case.cloud, L.transform_f32(ref.pose, ref.case.queries))
    assert np.all(found == 5)
    n, valid, res = oracle.find_correspondences(m, ref.case.queries, ref.pose, max_corr=L.MAX_CORR, kdtree=True)
    assert n == valid.sum()
    *_, note = L.check_planes(ref, valid, res, idx, label=f"oracle {family} {which}")
    print(note)


def test_kitti_like_map_conditioning():
    """The conditioning the project's own KITTI-like test map produces stays far inside the regime where the
    A^T A route is bounded at 1e-6 m (the figure quoted in tests/test_gpu_linalg_plane.py)."""
    kappa, term1, n = L.kitti_like_kappa()
    assert n > 1000 and term1 < 1e-6, (kappa, term1, n)


# ---------------------------------------------------------------------------------------------- C. exact GN step
@pytest.fixture(scope="module")
def families():
    return L.solve_families()


@pytest.mark.parametrize("name", ["realistic", "pivoting", "graded", "edge"])
def test_oracle_exact_step(families, name):
    tot, pose, expect_all, max_skipped = families[name]
    fin = np.isfinite(tot).all(1)
    out = np.zeros((len(tot), 19), np.uint32)
    out[fin] = L.oracle_steps(tot[fin], pose[fin])
    sel = L.check_solve(tot, pose, out, label=f"oracle {name}", max_skipped=max_skipped, expect_all=expect_all)
    if name == "pivoting":
        assert (~sel.spd).sum() > 0.5 * len(tot)                    # the sign flips: indefinite systems are covered
    if name == "graded":
        assert sel.nondegenerate.mean() > 0.95 and not sel.spd.any()
    if name == "edge":
        assert sel.nondegenerate.sum() >= 80
