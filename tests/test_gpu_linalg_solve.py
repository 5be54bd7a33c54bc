"""The exact GN step on the device (lo_exact.h: fp32 pivoted LDLT, SO3::Exp with the restated sinf / cosf, the SVD
re-projection and the SE3 product; one-lane and wave forms through lo_exact_solve_both) against fp64 numpy
(tests/_linalg_ref.py): for EVERY finite, non-degenerate system the residual of the solve (backward stability, with
the factor growth of an fp64 replay of the same pivot order folded in for indefinite systems), the new rotation
against polar(R_old) Exp64(delta_w), the new translation and the convergence flag.  tests/test_gpu_solve_wave.py pins
the two forms to each other and to the oracle bit for bit; tests/test_linalg_ref.py is the CPU twin.

The edge family's Exp angle sweep (1e-11 .. 3.1 rad, both sides of the 1e-10 and 1e-6 branch points) is the only
place the device build of the sinf / cosf restatement meets an independent reference.  The graded family is there for
the pivot rule: on the pivoting family the diagonal dominates, so any pivot order is stable.
"""
import numpy as np
import pytest

from tests import _linalg_ref as L
from tests.test_gpu_solve_wave import _solve_both

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 12)
    yield o
    o.close()


@pytest.fixture(scope="module")
def families():
    return L.solve_families()


@pytest.mark.parametrize("name", ["realistic", "pivoting", "graded", "edge"])
def test_exact_step_against_fp64(ctx, families, name):
    tot, pose, expect_all, max_skipped = families[name]
    assert len(tot) <= 6000
    a, b = _solve_both(ctx, tot, pose)
    for form, out in (("one-lane", a), ("wave", b)):
        sel = L.check_solve(tot, pose, out, label=f"{form} {name}", max_skipped=max_skipped, expect_all=expect_all)
    if name == "edge":
        names = [c[0] for c in L.edge_cases(np.random.default_rng(13))]
        theta = np.asarray([nm.startswith("theta") for nm in names])
        assert theta.sum() == 76 and sel.nondegenerate[theta].all()     # the whole angle sweep was checked
