"""lo_batch_optimize_loop_dev (the loop-closure ICP of many jobs in one lockstep run) against lo_icp_optimize_loop_dev.

Every batched record must EQUAL the solo entry's result for the same inputs and the same arithmetic mode: codes and
counts, T_rel and the inlier ratio as bit patterns, the costs, the iteration logs as raw bytes.  The solo runs are made
on a context of their own (same configuration), never on a context of the batch.
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
SENT = -7.0


def _fp(a):
    return a.ctypes.data_as(FP)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _make(n, kd=False):
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer
    if kd:
        return [IterativeClosestPointOptimizer(ICPConfig(use_surfel_correspondence=False), max_points=MAX_POINTS)
                for _ in range(n)]
    return [IterativeClosestPointOptimizer(max_points=MAX_POINTS) for _ in range(n)]


@pytest.fixture(scope="module")
def pool():
    """Six surfel-mode contexts in one batch, and a seventh for the solo runs."""
    from lidar_odometry_amd import BatchOptimizer
    ctxs = _make(7)
    b = BatchOptimizer(ctxs[:6])
    yield ctxs[:6], b, ctxs[6]
    b.close()
    for o in ctxs:
        o.close()


@pytest.fixture(scope="module")
def clouds():
    """The inputs every test draws from (computed once): name -> (cur, T_curr, mat, T_matched)."""
    c = {}
    cur, Tc, mat, Tm, _ = _data.loop_case(2, 6, 0)
    c["a"] = (cur, Tc, mat, Tm)
    cur, Tc, mat, Tm, _ = _data.loop_case(20, 23, 9)
    c["b"] = (cur, Tc, mat, Tm)
    cur, Tc, _, Tm, _ = _data.loop_case(4, 7, 3)
    big = oracle.voxel_filter(_data.kitti_scan(4, 40), 0.3, 1)          # 11.6k points
    assert len(big) > 8192
    c["grid"] = (cur, Tc, big, Tm)
    cur, Tc, mat, Tm, _ = _data.loop_case(10, 14, 5)
    far = _f32(Tm).copy()
    far[3] += 500.0
    c["far"] = (cur, Tc, mat, far)
    c["few"] = (c["a"][0], c["a"][1], c["a"][2][:4], c["a"][3])
    c["bigcur"] = (big, c["grid"][1], c["a"][2], c["a"][3])             # n_curr > 8192
    # a start close to the answer: fewer iterations than "a"
    cur, Tc, mat, Tm, _ = _data.loop_case(20, 23, 9, sigma_t=0.01, sigma_r=0.001)
    c["near"] = (cur, Tc, mat, Tm)
    for k, v in c.items():
        c[k] = (_f32(v[0]).reshape(-1, 3), _f32(v[1]).reshape(12), _f32(v[2]).reshape(-1, 3), _f32(v[3]).reshape(12))
    return c


def _dev(a):
    import torch
    t = torch.from_numpy(a if len(a) else np.zeros((1, 3), np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def _solo(icp, case):
    """lo_icp_optimize_loop_dev on `icp` -> what it wrote, as test_gpu_loop_dev._call."""
    cur, Tc, mat, Tm = case
    dc, dm = _dev(cur), _dev(mat)
    Tr = np.full(12, SENT, np.float32)
    inl = C.c_float(SENT)
    logs = (_lib.LoIterLog * _lib.LO_MAX_ITERS)()
    st = _lib.LoStats()
    rc = _lib.lib().lo_icp_optimize_loop_dev(icp.ctx, C.c_void_p(dc.data_ptr()), len(cur), _fp(Tc),
                                             C.c_void_p(dm.data_ptr()), len(mat), _fp(Tm), _fp(Tr), C.byref(inl), logs,
                                             C.byref(st))
    n = min(max(st.iterations, 0), _lib.LO_MAX_ITERS)
    return {"rc": rc, "T_rel": Tr.view(np.uint32).copy(), "inlier": np.float32(inl.value).view(np.uint32),
            "logs": bytes(memoryview(logs))[: n * C.sizeof(_lib.LoIterLog)], "iterations": st.iterations,
            "n_corr": st.n_corr, "status": st.status, "converged": st.converged,
            "costs": (np.float32(st.initial_cost).view(np.uint32), np.float32(st.final_cost).view(np.uint32))}


def _batched(b, jobs, cases):
    """One lo_batch_optimize_loop_dev call: jobs[i] runs cases[i]."""
    keep = [(_dev(c[0]), _dev(c[2])) for c in cases]
    arg = [(j, (dc.data_ptr(), len(c[0])), c[1], (dm.data_ptr(), len(c[2])), c[3])
           for j, c, (dc, dm) in zip(jobs, cases, keep)]
    return b.optimize_loop_dev(arg, sentinel=SENT)


def _assert_equal(r, s):
    print(f"batched: status {r.status} conv {r.converged} iters {r.iterations} n_corr {r.n_corr} rerun {r.rerun} | "
          f"solo: rc {s['rc']} conv {s['converged']} iters {s['iterations']} n_corr {s['n_corr']}")
    assert r.status == s["rc"] == s["status"]
    assert (r.iterations, r.n_corr, int(r.converged)) == (s["iterations"], s["n_corr"], s["converged"])
    np.testing.assert_array_equal(r.T_rel.view(np.uint32), s["T_rel"])
    assert np.float32(r.inlier_ratio).view(np.uint32) == s["inlier"]
    assert (np.float32(r.initial_cost).view(np.uint32), np.float32(r.final_cost).view(np.uint32)) == s["costs"]
    assert r.logs == s["logs"]


def _set_modes(ctxs, modes):
    for o, m in zip(ctxs, modes):
        o.set_exact(m)


def _mixed_call(pool, clouds, modes):
    ctxs, b, solo = pool
    names = ["a", "b", "grid", "far", "few"]
    cases = [clouds[k] for k in names]
    _set_modes(ctxs[:5], modes)
    try:
        got = _batched(b, [0, 1, 2, 3, 4], cases)
        for r, case, m in zip(got, cases, modes):
            solo.set_exact(m)
            _assert_equal(r, _solo(solo, case))
        for r in got[:3]:
            assert r.status == _lib.LO_OK and r.converged and r.iterations > 0
        for r in got[3:]:
            assert r.status == _lib.LO_INSUFFICIENT
            if not r.converged:                                  # untouched, as the solo entry leaves them
                assert np.all(r.T_rel == np.float32(SENT)) and r.inlier_ratio == np.float32(SENT)
        assert not got[4].converged
    finally:
        _set_modes(ctxs, [True] * len(ctxs))
        solo.set_exact(True)


def test_mixed_call_exact(pool, clouds):
    _mixed_call(pool, clouds, [True] * 5)


def test_mixed_call_fast_and_mixed_modes(pool, clouds):
    _mixed_call(pool, clouds, [False] * 5)
    _mixed_call(pool, clouds, [True, False, True, False, True])


def _optimize_bits(o, pts, Ti):
    _, T = o.optimize(None, pts, Ti)
    logs = [it["pose"].copy() for it in o.get_last_stats().iterations]
    return np.asarray(T, np.float32).view(np.uint32).copy(), logs


def test_subset_and_order(pool, clouds):
    ctxs, b, solo = pool
    m, pts, Ti, _ = _data.kitti_case(11)
    k, n, c = _data.surfels(m)
    ctxs[2].set_surfels(k, n, c)
    A, logs_a = _optimize_bits(ctxs[2], pts, Ti)
    sa, sb = _solo(solo, clouds["a"]), _solo(solo, clouds["b"])
    got = _batched(b, [4, 1], [clouds["a"], clouds["b"]])
    _assert_equal(got[0], sa)
    _assert_equal(got[1], sb)
    B, logs_b = _optimize_bits(ctxs[2], pts, Ti)                   # an unlisted context: its map and GN state untouched
    np.testing.assert_array_equal(A, B)
    assert len(logs_a) == len(logs_b)
    for x, y in zip(logs_a, logs_b):
        np.testing.assert_array_equal(x, y)
    got = _batched(b, [1, 4], [clouds["a"], clouds["b"]])         # swapped inputs: nothing left over from the first call
    _assert_equal(got[0], sa)
    _assert_equal(got[1], sb)


def test_different_iteration_counts(pool, clouds):
    ctxs, b, solo = pool
    sa, sn = _solo(solo, clouds["a"]), _solo(solo, clouds["near"])
    print("solo iteration counts:", sa["iterations"], sn["iterations"])
    assert sa["iterations"] != sn["iterations"]
    got = _batched(b, [0, 1], [clouds["a"], clouds["near"]])
    _assert_equal(got[0], sa)
    _assert_equal(got[1], sn)


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


def test_tie_rerun(pool, clouds):
    ctxs, b, solo = pool
    L = _lib.lib()
    lat = _lattice()
    sl, sa = _solo(solo, lat), _solo(solo, clouds["a"])
    before = [L.lo_loop_reruns(o.ctx) for o in ctxs]
    got = _batched(b, [3, 0], [lat, clouds["a"]])
    assert got[0].rerun and not got[1].rerun
    after = [L.lo_loop_reruns(o.ctx) for o in ctxs]
    assert after[3] == before[3] + 1
    assert [x for i, x in enumerate(after) if i != 3] == [x for i, x in enumerate(before) if i != 3]
    _assert_equal(got[0], sl)
    _assert_equal(got[1], sa)
    assert sl["iterations"] > 0


def test_large_exact_job(pool, clouds):
    ctxs, b, solo = pool
    assert len(clouds["bigcur"][0]) > 8192
    got = _batched(b, [0, 5], [clouds["bigcur"], clouds["b"]])
    _assert_equal(got[0], _solo(solo, clouds["bigcur"]))
    _assert_equal(got[1], _solo(solo, clouds["b"]))


def test_current_cloud_in_place(pool, clouds):
    from lidar_odometry_amd import GlobalMapBuilder
    ctxs, b, solo = pool
    raws = [_data.kitti_scan(6, 40), _data.kitti_scan(23, 40)]
    names = ["a", "b"]
    gs, arg, want, curs = [], [], [], []
    try:
        for o, raw, k in zip(ctxs[:2], raws, names):
            cur = o.voxel_filter(raw, 0.5, stride=8)               # leaves the filtered scan in the context's buffer
            _, Tc, mat, Tm = clouds[k]
            g = GlobalMapBuilder(o, max_points=1 << 15, max_keyframes=4)
            gs.append(g)
            g.add_from_scan(0)
            g.add_keyframe(1, mat)
            _, p_cur, n_cur = g.keyframe_points(0)
            _, p_mat, n_mat = g.keyframe_points(1)
            assert (n_cur, n_mat) == (len(cur), len(mat))
            arg.append((len(arg), (p_cur, n_cur), Tc, (p_mat, n_mat), Tm))
            want.append(_solo(solo, (_f32(cur), Tc, mat, Tm)))
            curs.append(cur)
        got = b.optimize_loop_dev(arg, sentinel=SENT)
        for r, s in zip(got, want):
            _assert_equal(r, s)
            assert r.status == _lib.LO_OK
        for o, cur in zip(ctxs[:2], curs):
            np.testing.assert_array_equal(o.filtered_points(), cur)
    finally:
        for g in gs:
            g.close()


def test_argument_checks(pool, clouds):
    ctxs, b, solo = pool
    L = _lib.lib()
    cur, Tc, mat, Tm = clouds["a"]
    dc, dm = _dev(cur), _dev(mat)

    def job(j, pc, nc, pm=None, nm=None):
        J = _lib.LoLoopJob()
        J.job, J.d_curr, J.n_curr = j, pc, nc
        J.d_matched, J.n_matched = (dm.data_ptr() if pm is None else pm), (len(mat) if nm is None else nm)
        J.T_curr[:] = Tc.tolist()
        J.T_matched[:] = Tm.tolist()
        return J

    def call(js):
        arr = (_lib.LoLoopJob * len(js))(*js)
        recs = (_lib.LoLoopRec * len(js))()
        rc = L.lo_batch_optimize_loop_dev(b._b, arr, len(js), recs, None, None)
        return rc, L.lo_batch_last_error(b._b).decode()

    ok = job(0, dc.data_ptr(), len(cur))
    rc, msg = call([ok, job(0, dc.data_ptr(), len(cur))])
    assert rc == _lib.LO_ERR_ARG and "job 0" in msg
    rc, msg = call([ok, job(6, dc.data_ptr(), len(cur))])
    assert rc == _lib.LO_ERR_ARG and "6" in msg
    rc, msg = call([job(1, None, 8)])
    assert rc == _lib.LO_ERR_ARG and "job 1" in msg
    rc, msg = call([job(2, dc.data_ptr(), MAX_POINTS + 1)])
    assert rc == _lib.LO_ERR_CAPACITY and "job 2" in msg
    assert L.lo_batch_optimize_loop_dev(b._b, None, 0, None, None, None) == _lib.LO_OK
    b.optimize_async([0] * 6, [0] * 6, np.tile(np.eye(3, 4, dtype=np.float32).reshape(1, 12), (6, 1)))
    try:
        rc, msg = call([ok])
        assert rc == _lib.LO_ERR_STATE
    finally:
        b.result()
    got = _batched(b, [0], [clouds["a"]])                          # and the batch still works
    _assert_equal(got[0], _solo(solo, clouds["a"]))


def _grid_bits(o, loop=False):
    L = _lib.lib()
    f = L.lo_debug_loop_grid if loop else L.lo_debug_grid
    h, org, dim, m = C.c_float(0), (C.c_int * 3)(), (C.c_int * 3)(), C.c_int(0)
    assert f(o.ctx, C.byref(h), org, dim, C.byref(m), None, 0, None, 0) == _lib.LO_OK
    ncell = dim[0] * dim[1] * dim[2]
    start = np.zeros(ncell + 1, np.uint32)
    pts = np.zeros((max(m.value, 1), 4), np.float32)
    assert f(o.ctx, C.byref(h), org, dim, C.byref(m), start.ctypes.data_as(C.POINTER(C.c_uint32)), len(start), _fp(pts),
             len(pts)) == _lib.LO_OK
    return h.value, tuple(org), tuple(dim), m.value, start.tobytes(), pts[:m.value].tobytes()


def test_cell_grid_jobs_in_lockstep(pool, clouds):
    """Two matched clouds beyond 8192 points of different sizes (one context exact, one fast) beside an all-pairs job:
    records equal to solo, and each context's loop grid is the grid the solo entry builds (geometry after the occupancy
    rule, cell starts, points)."""
    ctxs, b, solo = pool
    big2 = _f32(oracle.voxel_filter(_data.kitti_scan(20, 40), 0.25, 1))
    assert len(big2) > 8192 and len(big2) != len(clouds["grid"][2])
    g2 = (clouds["b"][0], clouds["b"][1], big2, clouds["b"][3])
    cases, jobs, modes = [clouds["grid"], clouds["a"], g2], [1, 3, 4], [True, True, False]
    try:
        for j, m in zip(jobs, modes):
            ctxs[j].set_exact(m)
        got = _batched(b, jobs, cases)
        grids = [_grid_bits(ctxs[j], loop=True) for j in jobs]
        for r, case, m, g in zip(got, cases, modes, grids):
            solo.set_exact(m)
            _assert_equal(r, _solo(solo, case))
            want = _grid_bits(solo, loop=True)
            if len(case[2]) > 8192:
                print("loop grid: h", g[0], "dim", g[2], "m", g[3], "rerun", r.rerun)
                assert g == want
        assert got[0].status == _lib.LO_OK and got[1].status == _lib.LO_OK
    finally:
        _set_modes(ctxs, [True] * len(ctxs))
        solo.set_exact(True)


def test_non_finite_matched_point_is_an_argument_error(pool, clouds):
    """As the solo entry: LO_ERR_ARG for the call, naming the job, whichever form the job's local map takes."""
    ctxs, b, solo = pool
    L = _lib.lib()
    for name in ("a", "grid", "bigcur"):
        cur, Tc, mat, Tm = clouds[name]
        bad = mat.copy()
        bad[len(bad) // 2, 1] = np.nan
        assert _solo(solo, (cur, Tc, bad, Tm))["rc"] == _lib.LO_ERR_ARG
        with pytest.raises(RuntimeError, match="job 2.*non-finite"):
            _batched(b, [0, 2], [clouds["b"], (cur, Tc, bad, Tm)])
        assert L.lo_loop_reruns(ctxs[2].ctx) >= 0
    got = _batched(b, [0, 2], [clouds["b"], clouds["a"]])
    _assert_equal(got[0], _solo(solo, clouds["b"]))
    _assert_equal(got[1], _solo(solo, clouds["a"]))


def test_kdtree_batch(clouds):
    from lidar_odometry_amd import BatchOptimizer
    ctxs = _make(3, kd=True)
    b = None
    try:
        for o, k in zip(ctxs[:2], ("a", "b")):
            o.set_map_points(clouds[k][2])
        b = BatchOptimizer(ctxs[:2])
        before = [_grid_bits(o) for o in ctxs[:2]]
        got = _batched(b, [0, 1], [clouds["a"], clouds["b"]])
        assert [_grid_bits(o) for o in ctxs[:2]] == before
        _assert_equal(got[0], _solo(ctxs[2], clouds["a"]))
        _assert_equal(got[1], _solo(ctxs[2], clouds["b"]))
        assert got[0].status == _lib.LO_OK and got[1].status == _lib.LO_OK
    finally:
        if b is not None:
            b.close()
        for o in ctxs:
            o.close()
