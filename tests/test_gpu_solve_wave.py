"""The wave-cooperative reference-exact GN solve (lo_exact.h exact_solve_step_wave, run by wave 0 of every exact PKO
candidate workgroup) against the one-lane exact_solve_step, bit for bit: the new pose, delta and the convergence flag
of lo_exact_solve_both's two forms on the same 43 totals and pose.  The one-lane form is pinned to the oracle by
tests/test_gpu_exact.py; a subset here is also compared with the oracle's own LDLT / SO3::Exp / SE3 product."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import _linalg_ref
from tests._linalg_ref import (edge_cases as _edge_cases, oracle_step as _oracle_step, pivot_replay as _pivot_replay,
                               pivoting_systems as _pivoting_systems, poses as _poses, realistic as _realistic,
                               totals as _totals)

pytestmark = pytest.mark.gpu

TOL = _linalg_ref.TOL


@pytest.fixture(scope="module")
def ctx():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 12)
    yield o
    o.close()


def _solve_both(o, tot, pose, tol_t=TOL, tol_r=TOL):
    from lidar_odometry_amd import lib
    tot = np.ascontiguousarray(tot, np.float32).reshape(-1, 43)
    pose = np.ascontiguousarray(pose, np.float32).reshape(-1, 12)
    n = len(tot)
    assert len(pose) == n
    a = np.full((n, 19), 0xdeadbeef, np.uint32)
    b = np.full((n, 19), 0xfeedf00d, np.uint32)
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    rc = lib().lo_exact_solve_both(o.ctx, tot.ctypes.data_as(fp), pose.ctypes.data_as(fp), n, tol_t, tol_r,
                                   a.ctypes.data_as(up), b.ctypes.data_as(up))
    assert rc == 0, rc
    return a, b


def _assert_same(a, b):
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), bad[:8], a[bad[:2]], b[bad[:2]])


def test_realistic_systems_bitwise(ctx):
    rng = np.random.default_rng(11)
    n = 4096
    tot, pose = _realistic(rng, n), _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    _assert_same(a, b)
    # the hook ran, and every system's step is the fp64 one within the fp32 bounds (tests/_linalg_ref.py)
    _linalg_ref.check_solve(tot, pose, a, tol_t=TOL, tol_r=TOL, label="realistic", expect_all=True)
    for i in range(0, n, 32):                                        # ... and both equal the oracle's own step
        pn_o, d_o = _oracle_step(tot[i], pose[i])
        np.testing.assert_array_equal(b[i, :12], pn_o.view(np.uint32), err_msg=f"system {i} pose")
        np.testing.assert_array_equal(b[i, 12:18], d_o.view(np.uint32), err_msg=f"system {i} delta")


def test_pivoting_bitwise(ctx):
    rng = np.random.default_rng(12)
    Hs, _ = _pivoting_systems(rng)
    n = len(Hs)
    count = np.zeros((5, 6), int)
    ties = negs = 0
    for H in Hs:
        tr, tie, neg = _pivot_replay(H)
        for k, q in enumerate(tr):
            count[k, q] += 1
        ties += tie
        negs += neg
    for k in range(5):
        for q in range(k, 6):
            assert count[k, q] > 0, ("pivot choice never taken", k, q)
    assert ties > 0 and negs > 0, (ties, negs)
    g = rng.normal(0, 1.0, (n, 6))
    tot = _totals(Hs, g, rng.uniform(0, 1, n))
    pose = _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    _assert_same(a, b)
    for i in range(0, n, 16):
        d_o = oracle.ldlt6_solve(tot[i, :36], -tot[i, 36:42])
        np.testing.assert_array_equal(b[i, 12:18], d_o.view(np.uint32), err_msg=f"system {i} delta")


def test_edge_paths_bitwise(ctx):
    rng = np.random.default_rng(13)
    cases = _edge_cases(rng)
    n = len(cases)
    tot = _totals([c[1] for c in cases], [c[2] for c in cases], rng.uniform(0, 1, n))
    tot[-1, 42] = np.nan
    pose = _poses(rng, n)
    a, b = _solve_both(ctx, tot, pose)
    bad = [cases[i][0] for i in np.nonzero((a != b).any(axis=1))[0]]
    assert not bad, bad
    names = [c[0] for c in cases]
    d = a[:, 12:18].view(np.float32)
    assert not d[names.index("H = 0")].any()                         # the zero_all return
    assert d[names.index("subnormal diagonal"), 5] == 0 and d[names.index("diagonal = FLT_MIN"), 4] == 0
    assert d[names.index("diagonal just above FLT_MIN"), 5] != 0
    conv = {nm: int(a[i, 18]) for i, nm in enumerate(names) if nm.startswith("conv")}
    assert conv["conv 5e-05 5e-05"] == 1 and conv["conv 0.0002 5e-05"] == 0 and conv["conv 5e-05 0.0002"] == 0
    assert conv["conv 9.9e-05 9.9e-05"] == 1 and conv["conv 0.000101 9.9e-05"] == 0 and conv["conv 9.9e-05 0.000101"] == 0
    # a non-finite pose as well: the SVD's non-finite return
    pose2 = pose[:8].copy()
    pose2[0, 0] = np.nan; pose2[1, 5] = np.inf; pose2[2, 3] = np.nan; pose2[3, 10] = -np.inf
    a2, b2 = _solve_both(ctx, tot[7:15], pose2)
    _assert_same(a2, b2)


def test_small_scan_end_to_end_bitwise():
    """A 500-point synthetic scan through optimize in exact mode (its PKO launches solve the candidates across wave 0):
    every iteration's log equals the oracle's."""
    from lidar_odometry_amd import IterativeClosestPointOptimizer, synth
    sc = synth.patch_scene(n_patches=60, seed=3, extent=15.0)
    vm = oracle.VoxelMap(0.5, 3, 0.1, True)
    vm.update(synth.sample_patches(sc, 60000, 4, outlier_frac=0.0), np.zeros(3), 1e3, True)
    T = synth.se3(synth.rot_z(0.1), [0.4, -0.2, 0.1])
    pts = synth.transform(np.linalg.inv(T), synth.sample_patches(sc, 500, 5))
    Ti = synth.perturb(T, np.random.default_rng(0))[:3].astype(np.float32).reshape(12)
    ok_o, To_o, it_o, logs_o = oracle.icp_optimize(vm, pts, Ti)
    o = IterativeClosestPointOptimizer(device=0, max_points=1024)
    try:
        o.set_exact(True)
        k, n, c, _ = vm.surfels()
        o.set_surfels(k, n, c)
        ok_g, To_g = o.optimize(None, pts, Ti)
        st = o.get_last_stats()
        # the scan took the fused candidate path: only its PKO launches write candidate records, and the last
        # launch's chosen candidate is the last iteration's GN step
        from lidar_odometry_amd import lib
        rec = np.zeros((256, 48), np.float32)
        ncand = lib().lo_debug_cand_records(o.ctx, rec.ctypes.data_as(C.POINTER(C.c_float)), rec.size)
        assert ncand > 1, ncand
        rec = rec[:ncand].view(np.uint32)
    finally:
        o.close()
    steps = [np.asarray(lg["delta"], np.float32).view(np.uint32) for lg in st.iterations[:st.num_iterations]]
    hit = [(rec[c, 40:46] == d).all() and d.any() for c in range(ncand) for d in steps]
    assert any(hit), "no candidate record holds a logged GN step: the candidates did not solve it"
    assert ok_g == ok_o and st.num_iterations == it_o and it_o >= 2
    for k, (lo, lg) in enumerate(zip(logs_o, st.iterations)):
        for key in ("pose", "H", "g", "delta"):
            np.testing.assert_array_equal(np.asarray(lg[key], np.float32).view(np.uint32),
                                          np.asarray(lo[key], np.float32).view(np.uint32), err_msg=f"iter {k} {key}")
        assert lg["n_corr"] == lo["n_corr"] and lg["scale"] == lo["scale"] and lg["alpha"] == lo["alpha"], k
        assert np.float32(lg["cost"]) == np.float32(lo["cost"]), k
    np.testing.assert_array_equal(np.asarray(To_g, np.float32).reshape(12).view(np.uint32),
                                  np.asarray(To_o, np.float32).reshape(12).view(np.uint32))
