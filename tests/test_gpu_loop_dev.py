"""lo_icp_optimize_loop_dev (loop-closure ICP on device-resident clouds) against lo_icp_optimize_loop (host clouds).

The two entry points share everything after the matched cloud's local map: for equal inputs the return code, T_rel,
the inlier ratio, every iteration log (as raw bytes), the iteration count and n_corr must be EQUAL.  The host-input
tests (tests/test_gpu_loop.py) pin lo_icp_optimize_loop to the oracle bit for bit, so this equality pins the device
entry to the oracle too.  Also here: lo_gmap_keyframe_points, the in-place view of a stored keyframe.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
from lidar_odometry_amd import _lib
from tests import _data

pytestmark = pytest.mark.gpu

MAX_POINTS = 1 << 16
FP = C.POINTER(C.c_float)


def _fp(a):
    return a.ctypes.data_as(FP)


@pytest.fixture(scope="module")
def icp():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=MAX_POINTS)
    yield o
    o.close()


def _call(icp, dev, cur, Tc, mat, Tm):
    """One raw call of either entry point -> everything it wrote, logs as bytes."""
    import torch
    L = _lib.lib()
    cur = np.ascontiguousarray(cur, np.float32).reshape(-1, 3)
    mat = np.ascontiguousarray(mat, np.float32).reshape(-1, 3)
    Tc = np.ascontiguousarray(Tc, np.float32).reshape(12)
    Tm = np.ascontiguousarray(Tm, np.float32).reshape(12)
    Tr = np.full(12, -7.0, np.float32)
    inl = C.c_float(-7.0)
    logs = (_lib.LoIterLog * _lib.LO_MAX_ITERS)()
    st = _lib.LoStats()
    if dev:
        # (an empty tensor has no storage: any non-null pointer stands in for it, it is never read)
        dc = torch.from_numpy(cur if len(cur) else np.zeros((1, 3), np.float32)).cuda()
        dm = torch.from_numpy(mat if len(mat) else np.zeros((1, 3), np.float32)).cuda()
        torch.cuda.synchronize()
        rc = L.lo_icp_optimize_loop_dev(icp.ctx, C.c_void_p(dc.data_ptr()), len(cur), _fp(Tc), C.c_void_p(dm.data_ptr()),
                                        len(mat), _fp(Tm), _fp(Tr), C.byref(inl), logs, C.byref(st))
        del dc, dm
    else:
        rc = L.lo_icp_optimize_loop(icp.ctx, _fp(cur), len(cur), _fp(Tc), _fp(mat), len(mat), _fp(Tm), _fp(Tr),
                                    C.byref(inl), logs, C.byref(st))
    n = min(max(st.iterations, 0), _lib.LO_MAX_ITERS)
    return {"rc": rc, "T_rel": Tr.view(np.uint32).copy(), "inlier": np.float32(inl.value).view(np.uint32),
            "logs": bytes(memoryview(logs))[: n * C.sizeof(_lib.LoIterLog)], "iterations": st.iterations,
            "n_corr": st.n_corr, "status": st.status, "converged": st.converged}


def _assert_equal(a, b):
    assert a["rc"] == b["rc"]
    assert (a["iterations"], a["n_corr"], a["status"], a["converged"]) == \
           (b["iterations"], b["n_corr"], b["status"], b["converged"])
    np.testing.assert_array_equal(a["T_rel"], b["T_rel"])
    assert a["inlier"] == b["inlier"]
    assert a["logs"] == b["logs"]


def _both_modes(icp, cur, Tc, mat, Tm):
    """Host and device entry in the default exact mode and in the fast mode; -> the exact-mode host result."""
    out = None
    try:
        for exact in (True, False):
            icp.set_exact(exact)
            h = _call(icp, False, cur, Tc, mat, Tm)
            d = _call(icp, True, cur, Tc, mat, Tm)
            _assert_equal(d, h)
            out = out or h
    finally:
        icp.set_exact(True)
    return out


@pytest.mark.parametrize("fa,fb,seed", [(2, 6, 0), (20, 23, 9)])
def test_all_pairs_path_equals_host_entry(icp, fa, fb, seed):
    cur, Tc, mat, Tm, _ = _data.loop_case(fa, fb, seed)
    assert len(mat) <= 8192 and len(cur) <= 8192
    h = _both_modes(icp, cur, Tc, mat, Tm)
    assert h["rc"] == _lib.LO_OK and h["converged"] == 1 and h["iterations"] > 0


def test_grid_path_equals_host_entry(icp):
    """A matched cloud beyond kKnnAllMax: the device-built cell grid (with the loop's occupancy rule) against the
    host-built one."""
    cur, Tc, _, Tm, _ = _data.loop_case(4, 7, 3)
    mat = oracle.voxel_filter(_data.kitti_scan(4, 40), 0.3, 1)          # 11.6k points
    assert len(mat) > 8192
    h = _both_modes(icp, cur, Tc, mat, Tm)
    assert h["rc"] == _lib.LO_OK and h["converged"] == 1


def _lattice():
    g = np.arange(-8.0, 8.0, 0.5, dtype=np.float32)
    X, Y = np.meshgrid(g, g, indexing="ij")
    floor = np.stack([X.ravel(), Y.ravel(), np.zeros(X.size, np.float32)], 1)
    wall = np.stack([np.full(X.size, 8.0, np.float32), X.ravel(), Y.ravel() * 0.25 + 2.0], 1)
    wall2 = np.stack([X.ravel(), np.full(X.size, -8.0, np.float32), Y.ravel() * 0.25 + 2.0], 1)
    mat = np.concatenate([floor, wall, wall2]).astype(np.float32)
    cur = (mat + np.array([0.25, 0.0, 0.0], np.float32)).astype(np.float32)      # midway along x: ties
    I = np.eye(3, 4, dtype=np.float32).reshape(12)
    Tc = I.copy()
    Tc[3] = 0.02
    return cur, Tc, mat, I


def test_lattice_ties_rerun_on_the_device_entry(icp):
    """Deciding distance ties: the device entry brings the gridded points down, builds the visit order and runs again
    (counted in lo_loop_reruns), and still equals the host entry."""
    L = _lib.lib()
    cur, Tc, mat, Tm = _lattice()
    h = _call(icp, False, cur, Tc, mat, Tm)
    before = L.lo_loop_reruns(icp.ctx)
    d = _call(icp, True, cur, Tc, mat, Tm)
    assert L.lo_loop_reruns(icp.ctx) == before + 1
    _assert_equal(d, h)
    assert h["iterations"] > 0


def test_failure_paths_equal_host_entry(icp):
    cur, Tc, mat, Tm, _ = _data.loop_case(2, 6)
    for c, m in ((cur[:0], mat), (cur, mat[:0]), (cur, mat[:4])):
        h = _call(icp, False, c, Tc, m, Tm)
        d = _call(icp, True, c, Tc, m, Tm)
        _assert_equal(d, h)
        assert d["rc"] == _lib.LO_INSUFFICIENT
    far = np.asarray(Tm, np.float32).copy()
    far[3] += 500.0
    h = _call(icp, False, cur, Tc, mat, far)
    d = _call(icp, True, cur, Tc, mat, far)
    _assert_equal(d, h)
    assert d["rc"] == _lib.LO_INSUFFICIENT


def test_capacity_and_null_arguments():
    import torch
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    L = _lib.lib()
    o = IterativeClosestPointOptimizer(max_points=1024)
    try:
        cur, Tc, mat, Tm, _ = _data.loop_case(2, 6)
        assert len(cur) > 1024
        d = _call(o, True, cur, Tc, mat, Tm)
        assert d["rc"] == _lib.LO_ERR_CAPACITY
        t = torch.zeros((8, 3), dtype=torch.float32).cuda()
        Tr = np.zeros(12, np.float32)
        inl = C.c_float(0.0)
        assert L.lo_icp_optimize_loop_dev(o.ctx, None, 8, _fp(Tc), C.c_void_p(t.data_ptr()), 8, _fp(Tm), _fp(Tr),
                                          C.byref(inl), None, None) == _lib.LO_ERR_ARG
        assert L.lo_icp_optimize_loop_dev(o.ctx, C.c_void_p(t.data_ptr()), 8, _fp(Tc), None, 8, _fp(Tm), _fp(Tr),
                                          C.byref(inl), None, None) == _lib.LO_ERR_ARG
    finally:
        o.close()


def test_device_loop_solve_leaves_the_map_alone(icp):
    """The context's surfel table and a following lo_icp_optimize are bit-identical before and after."""
    m, pts, Ti, _ = _data.kitti_case(11)
    k, n, c = _data.surfels(m)
    icp.set_surfels(k, n, c)
    count = _lib.lib().lo_map_surfel_count(icp.ctx)
    _, A = icp.optimize(None, pts, Ti)
    logs_a = [it["pose"].copy() for it in icp.get_last_stats().iterations]
    cur, Tc, mat, Tm, _ = _data.loop_case(2, 6)
    d = _call(icp, True, cur, Tc, mat, Tm)
    assert d["rc"] == _lib.LO_OK
    assert _lib.lib().lo_map_surfel_count(icp.ctx) == count
    _, B = icp.optimize(None, pts, Ti)
    logs_b = [it["pose"].copy() for it in icp.get_last_stats().iterations]
    np.testing.assert_array_equal(np.asarray(A), np.asarray(B))
    assert len(logs_a) == len(logs_b)
    for a, b in zip(logs_a, logs_b):
        np.testing.assert_array_equal(a, b)


def test_current_cloud_in_the_contexts_buffer_is_used_in_place(icp):
    """The frame loop's case: the current cloud is the context's own filtered scan."""
    from lidar_odometry_amd import GlobalMapBuilder
    _, Tc, mat, Tm, _ = _data.loop_case(2, 6)
    raw = _data.kitti_scan(6, 40)
    cur = icp.voxel_filter(raw, 0.5, stride=8)                     # leaves the filtered scan in the context's buffer
    np.testing.assert_array_equal(cur, oracle.voxel_filter(raw, 0.5, 8))
    h = _call(icp, False, cur, Tc, mat, Tm)
    icp.voxel_filter(raw, 0.5, stride=8)
    g = GlobalMapBuilder(icp, max_points=1 << 15, max_keyframes=4)
    try:
        g.add_from_scan(0)                                         # the same cloud, as a stored keyframe
        g.add_keyframe(1, mat)
        _, p_cur, n_cur = g.keyframe_points(0)
        _, p_mat, n_mat = g.keyframe_points(1)
        assert (n_cur, n_mat) == (len(cur), len(mat))
        ok, Tr, inl = icp.optimize_loop_dev((p_cur, n_cur), Tc, (p_mat, n_mat), Tm)
        assert ok and np.array_equal(np.asarray(Tr, np.float32).reshape(12).view(np.uint32), h["T_rel"])
        assert np.float32(inl).view(np.uint32) == h["inlier"]
        np.testing.assert_array_equal(icp.filtered_points(), cur)  # the scan is still the context's
    finally:
        g.close()


def test_gmap_keyframe_points(icp):
    from lidar_odometry_amd import GlobalMapBuilder
    L = _lib.lib()
    rng = np.random.default_rng(12)
    clouds = [rng.uniform(-5.0, 5.0, (n, 3)).astype(np.float32) for n in (700, 0, 1500, 33)]
    ids = [5, 9, 11, 40]
    g = GlobalMapBuilder(icp, max_points=4096, max_keyframes=8)
    back = GlobalMapBuilder(icp, max_points=4096, max_keyframes=8)   # reads the pointers back: device-to-device adds
    try:
        for i, c in zip(ids, clouds):
            g.add_keyframe(i, c)
        base, offset = None, 0
        for k, (i, c) in enumerate(zip(ids, clouds)):
            kid, ptr, n = g.keyframe_points(k)
            assert (kid, n) == (i, len(c))
            base = ptr if base is None else base
            assert ptr == base + 12 * offset                       # in place: consecutive inside the arena
            offset += n
            assert L.lo_gmap_add_keyframe(back._h, i, C.c_void_p(ptr), n, 1) == _lib.LO_OK
        identity = np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (len(ids), 1))
        # (1 * x + 0 * y + 0 * z + 0 is x itself: voxel_size 0 returns the stored points in insertion order)
        np.testing.assert_array_equal(back.build(identity, 0.0), np.concatenate(clouds))
        kid, p, n = C.c_int64(0), C.c_void_p(0), C.c_size_t(0)
        assert L.lo_gmap_keyframe_points(g._h, len(ids), C.byref(kid), C.byref(p), C.byref(n)) == _lib.LO_ERR_ARG
        assert L.lo_gmap_keyframe_points(None, 0, C.byref(kid), C.byref(p), C.byref(n)) == _lib.LO_ERR_ARG
        with pytest.raises(IndexError):
            g.keyframe_points(len(ids))
    finally:
        back.close()
        g.close()
