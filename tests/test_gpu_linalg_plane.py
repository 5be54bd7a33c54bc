"""The KDTree variant's 5-point plane fit on the device (lo_kdtree.hip plane_body / smallest_eigvec3d) against the
operation the reference performs: JacobiSVD of the centred 5x3 neighbour matrix, taken here with np.linalg.svd in
fp64 (tests/_linalg_ref.py PlaneRef).  The device does not take that SVD: it runs a cyclic Jacobi eigen-solve of the
3x3 scatter matrix A^T A, which squares the condition number.  tests/test_gpu_kdtree.py compares it with the oracle's
copy of the same sweep; this file measures it against the SVD route:

  * the 5-NN equal the fp64 brute force (no query has a tie among its six nearest: checked in fp64);
  * the valid set is the reference's, outside a relative 1e-9 of max_correspondence_distance and outside 1 % of the
    0.5 collinearity gate;
  * |dist - dist_ref| <= 64 eps64 kappa |q' - mean| + 64 eps64 (|q'| + |mean|), kappa = sigma1^2 / (sigma2^2 - sigma3^2),
    wherever the first term is below 1e-6 m.

Families: noisy planes, exactly coplanar dyadic patches, thin slabs, maps offset by 5000 m, stretched cells around
the collinearity gate, and strips -- tight triangles strung along a line, so that the first three neighbours pass the
gate while the five are nearly a line (sigma2 / sigma1 down to 1e-3).

Where the A^T A route is worst -- the strips, on an MI355X
(python -m pytest tests/test_gpu_linalg_plane.py -m gpu -k strips -s; tests/test_linalg_ref.py prints the same
figures for the oracle's twin of the sweep):
    identity pose:  worst |dist - dist_ref| 1.525e-11 m at kappa 8.666e+05; worst kappa 1.432e+06
    perturbed pose: worst |dist - dist_ref| 4.169e-11 m at kappa 1.093e+06; worst kappa 2.492e+06
(0.013 and 0.021 of the bound).  At kappa ~ 1e6 the eigen-solve of A^T A sits five orders of magnitude under 1e-6 m
from the reference's SVD route.  The KITTI-like map of tests/_data.py (kitti_case(11): 2668 valid correspondences)
has a worst kappa of 203 and a worst first term of the bound of 7.3e-13 m
(python -c "from tests import _linalg_ref as L; print(L.kitti_like_kappa())"): there is no finding to write up.
"""
import numpy as np
import pytest

from tests import _linalg_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kd_icp():
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False, max_correspondence_distance=L.MAX_CORR),
                                       max_points=1 << 14)
    yield o
    o.close()


@pytest.mark.parametrize("which", ["identity", "perturbed"])
@pytest.mark.parametrize("family", L.PLANE_FAMILIES)
def test_plane_fit_against_svd(kd_icp, family, which):
    ref = L.plane_ref(family, which)
    assert len(ref.case.cloud) <= 10000 and len(ref.q) <= 4000
    kd_icp.set_map_points(ref.case.cloud)
    idx, _, found = kd_icp.nearest_k_search(L.transform_f32(ref.pose, ref.case.queries))
    assert np.all(found == 5)
    n, valid, res = kd_icp.find_correspondences(ref.case.queries, ref.pose)
    assert n == valid.sum()
    err, kappa, kmax, note = L.check_planes(ref, valid, res, idx, label=f"device {family} {which}")
    print(note)
    if family == "strips":
        # the number nobody had: the A^T A route against the SVD route where it is worst
        assert kmax > 1e5, note
        assert err <= 1e-6, note
