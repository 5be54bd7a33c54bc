"""GPU tests of the scan overlap (lo_set_scan_overlap): a pipelined scan's hold of the context stream is enqueued by
the NEXT queued scan, behind that scan's own head (first correspondence launch + exact scale), which therefore runs
beside the previous scan's tail on a second set of per-scan state; every other library call enqueues the pending hold
first (flush_hold) and then behaves as before.

Bar: bit-identical to the same scans run one at a time with overlap off -- pose, status, iteration count, n_corr (the
exported record) and every iteration's log (lo_icp_result) -- in reference-exact and in fast mode, and the counter of
overlapped scans says where the overlap happened and where a call flushed it.
Small scene: the first keyframes of the KITTI-like sequence as the map, scans subsampled to 300-700 points (one above
the 1024-point sort width of the exact scale).
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _data

pytestmark = pytest.mark.gpu

LOG_FIELDS = ("pose", "n_corr", "scale", "alpha", "cost", "H", "g", "delta")


def _sub(pts, target):
    return np.ascontiguousarray(pts[np.linspace(0, len(pts) - 1, min(target, len(pts))).astype(np.int64)], np.float32)


@functools.lru_cache(maxsize=None)
def _scene():
    """(map, [(name, points, T_init)]): scans that converge in 1, 2 and 4 iterations are picked in _picked()."""
    m = _data.kitti_map(last_kf=4)
    pool = []
    for f, sig, tgt in ((3, 0.0, 500), (5, 0.003, 640), (7, 0.003, 420), (3, 0.006, 560), (5, 0.006, 400), (7, 0.01, 330),
                        (3, 0.01, 480), (5, 0.015, 700), (7, 0.015, 520), (3, 0.02, 600), (5, 0.02, 450), (7, 0.03, 520),
                        (3, 0.03, 380), (5, 0.05, 400), (3, 0.3, 600)):
        _, pts, Ti, _ = _data.kitti_case(f, seed=11, last_kf=4, sigma_t=sig, sigma_r=sig / 10)
        pool.append((f"f{f}s{sig}", _sub(pts, tgt), Ti))
    _, big, Tb, _ = _data.kitti_case(5, seed=3, last_kf=4)
    wide = np.ascontiguousarray(big[: min(len(big), 1500)], np.float32)      # beyond the 1024-point sort width
    return m, pool, (wide, Tb)


def _ctx(m, kd=False, max_points=1 << 15):
    from lidar_odometry_amd import ICPConfig, IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(config=ICPConfig(use_surfel_correspondence=not kd), max_points=max_points)
    if kd:
        o.set_map_points(m.l0_cloud())
    else:
        k, n, c = _data.surfels(m)
        o.set_surfels(k, n, c)
    return o


def _dev(pts):
    import torch
    if len(pts) == 0:
        return torch.zeros(1, 3, dtype=torch.float32, device="cuda:0"), 0
    return torch.from_numpy(np.ascontiguousarray(pts, np.float32).reshape(-1, 3)).to("cuda:0"), len(pts)


def _enqueue(o, d, n, Ti):
    T = np.ascontiguousarray(Ti, np.float32)
    rc = o._L.lo_icp_optimize_async(o.ctx, C.c_void_p(d.data_ptr()), n, T.ctypes.data_as(C.POINTER(C.c_float)))
    assert rc == 0, (rc, o._L.lo_last_error(o.ctx))


def _result(o):
    from lidar_odometry_amd._lib import LoIterLog, LoStats
    To = np.zeros(12, np.float32)
    logs = (LoIterLog * 4)()
    st = LoStats()
    rc = o._L.lo_icp_result(o.ctx, To.ctypes.data_as(C.POINTER(C.c_float)), logs, C.byref(st))
    its = []
    for i in range(min(st.iterations, 4)):
        its.append(tuple(np.asarray(getattr(logs[i], f)).tobytes() for f in LOG_FIELDS))
    return rc, To.tobytes(), st.iterations, st.n_corr, st.status, its


def _overlapped(o):
    out = (C.c_longlong * 2)()
    assert o._L.lo_scan_overlap_status(o.ctx, out) == 0
    return int(out[1])


def _solo(o, scans):
    """Each scan alone with overlap off: its exported record and its lo_icp_result."""
    import torch
    assert o._L.lo_set_scan_overlap(o.ctx, 0) == 0
    base = _overlapped(o)
    recs, res = [], []
    for d, n, Ti in scans:
        rec = torch.zeros(16, dtype=torch.float32, device="cuda:0")
        _enqueue(o, d, n, Ti)
        assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(rec.data_ptr())) == 0
        res.append(_result(o))
        assert o._L.lo_sync(o.ctx) == 0
        recs.append(rec.cpu().numpy().view(np.uint32).copy())
    assert _overlapped(o) == base
    assert o._L.lo_set_scan_overlap(o.ctx, 1) == 0
    return recs, res


def _queue_export(o, scans):
    """All scans queued back to back, each one's record exported behind it."""
    import torch
    recs = torch.zeros(len(scans), 16, dtype=torch.float32, device="cuda:0")
    for k, (d, n, Ti) in enumerate(scans):
        _enqueue(o, d, n, Ti)
        assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(recs[k].data_ptr())) == 0
    assert o._L.lo_sync(o.ctx) == 0
    return [r.view(np.uint32) for r in recs.cpu().numpy()]


def _queue_plain(o, scans):
    """All scans queued with no call in between, lo_icp_flush at the end: the last scan's result."""
    for d, n, Ti in scans:
        _enqueue(o, d, n, Ti)
    assert o._L.lo_icp_flush(o.ctx) == 0
    return _result(o)


@functools.lru_cache(maxsize=None)
def _picked(exact):
    """The six scans of the queue: converging in 1, 2 and 4 iterations (found among the pool by running it solo; the
    counts are asserted), the wide scan, one below min_correspondence_points, and an empty one."""
    m, pool, (wide, Tw) = _scene()
    o = _ctx(m)
    try:
        o.set_exact(exact)
        dev = [(*_dev(p), Ti) for _, p, Ti in pool]
        _, res = _solo(o, dev)
        by_iter = {}
        for (name, p, Ti), r in zip(pool, res):
            if r[0] == 0:
                by_iter.setdefault(r[2], (p, Ti))
        assert {1, 2, 4} <= set(by_iter), [(nm, r[0], r[2]) for (nm, _, _), r in zip(pool, res)]
    finally:
        o.close()
    far = by_iter[2][0] + np.float32(5000.0)
    # neighbours change their point count every time, once across the 1024-point edge in each direction
    return m, [by_iter[4], by_iter[1], (wide, Tw), by_iter[2], (far, by_iter[2][1]), (wide[:0], Tw)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_queued_equals_solo_bitwise(exact):
    m, scans = _picked(exact)
    o = _ctx(m)
    try:
        o.set_exact(exact)
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        assert all(300 <= n <= 700 for _, n, _ in dev[:2] + dev[3:5]) and dev[2][1] > 1024 and dev[5][1] == 0
        ref_rec, ref_res = _solo(o, dev)
        assert [r[2] for r in ref_res[:4]] == [4, 1, ref_res[2][2], 2]
        assert ref_res[4][0] == 1 and ref_res[5][0] == 1          # LO_INSUFFICIENT: too few correspondences, n == 0
        # records exported behind each scan (every export enqueues the hold: no overlap, same records)
        base = _overlapped(o)
        got = _queue_export(o, dev)
        assert _overlapped(o) == base
        for k in range(len(dev)):
            np.testing.assert_array_equal(got[k], ref_rec[k], err_msg=f"scan {k}")
        # nothing between the scans: every rotation of the queue, so that each scan is read as the last one
        for r in range(len(dev)):
            order = [(r + 1 + k) % len(dev) for k in range(len(dev))]
            res = _queue_plain(o, [dev[i] for i in order])
            assert res == ref_res[order[-1]], f"rotation {r}"
        # a scan whose tail ran beside the next scan's head: four pipelined scans queued, then the third one's record
        # read from the other lane (nothing was called between the scans, so nothing flushed)
        piped = [0, 1, 2, 3]
        for r in range(len(piped)):
            order = [piped[(r + k) % len(piped)] for k in range(len(piped))]
            base = _overlapped(o)
            res = _queue_plain(o, [dev[i] for i in order])
            assert _overlapped(o) == base + 3 and res == ref_res[order[-1]]
            rec = np.zeros(16, np.float32)
            assert o._L.lo_debug_other_lane_record(o.ctx, rec.ctypes.data_as(C.POINTER(C.c_float))) == 0
            np.testing.assert_array_equal(rec.view(np.uint32), ref_rec[order[-2]], err_msg=f"other lane, rotation {r}")
    finally:
        o.close()


def test_lane_hygiene():
    m, scans = _picked(True)
    o = _ctx(m)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        good, bad, other = dev[0], dev[4], dev[3]
        _, (r_good, r_bad, r_other) = _solo(o, [good, bad, other])
        assert r_bad[0] == 1 and r_good[0] == 0
        assert _queue_plain(o, [bad, good]) == r_good
        assert _queue_plain(o, [good, bad]) == r_bad
        assert _queue_plain(o, [bad, good, bad]) == r_bad
        assert _queue_plain(o, [good, bad, other]) == r_other     # the third of three queued scans
    finally:
        o.close()


def test_flush_points():
    """A call between two queued scans enqueues the first one's hold: results as the serial run, no overlap counted."""
    import torch
    m, scans = _picked(True)
    o = _ctx(m)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        a, b = dev[0], dev[3]
        k, n, c = _data.surfels(m)
        keys = np.ascontiguousarray(k[:8], np.int32)
        nn, cc = np.ascontiguousarray(n[:8], np.float32), np.ascontiguousarray(c[:8], np.float32)
        pres = np.ones(8, np.uint8)
        own = torch.cuda.Stream("cuda:0")

        def patch():
            assert o._L.lo_map_patch_surfels(o.ctx, keys.ctypes.data, nn.ctypes.data, cc.ctypes.data, pres.ctypes.data, 8) == 0

        calls = {
            "map_patch": (patch, lambda: None),                                       # the same surfels again
            "set_exact": (lambda: o.set_exact(False), lambda: o.set_exact(True)),
            "set_pipeline": (lambda: o.set_pipeline(False, 0), lambda: o.set_pipeline(True, 0)),
            "set_stream": (lambda: o._L.lo_set_stream(o.ctx, C.c_void_p(own.cuda_stream)),
                           lambda: o._L.lo_set_stream(o.ctx, None)),
        }
        for name, (call, undo) in calls.items():
            # serial: each scan read before the next call
            assert o._L.lo_set_scan_overlap(o.ctx, 0) == 0
            _enqueue(o, *a)
            ra = _result(o)
            call()
            _enqueue(o, *b)
            rb = _result(o)
            undo()
            assert o._L.lo_set_scan_overlap(o.ctx, 1) == 0
            # queued: scan, call, scan
            rec = torch.zeros(16, dtype=torch.float32, device="cuda:0")
            base = _overlapped(o)
            _enqueue(o, *a)
            call()
            assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(rec.data_ptr())) == 0   # scan a's record, after the call
            _enqueue(o, *b)
            got_b = _result(o)
            assert o._L.lo_sync(o.ctx) == 0
            undo()
            assert _overlapped(o) == base, name
            assert got_b == rb, name
            r = rec.cpu().numpy()
            assert r[:12].tobytes() == ra[1] and int(r[13]) == ra[2] and int(r[14]) == ra[3], name
    finally:
        o.close()


def test_counter_and_switches(monkeypatch):
    m, scans = _picked(True)
    dev = [(*_dev(p), Ti) for p, Ti in scans]
    six = [dev[0], dev[1], dev[2], dev[3], dev[0], dev[3]]         # six pipelined scans
    o = _ctx(m)
    try:
        ref = _queue_plain(o, six)
        assert _overlapped(o) == 5
        assert o._L.lo_set_scan_overlap(o.ctx, 0) == 0
        assert _queue_plain(o, six) == ref
        assert _overlapped(o) == 5
        assert o._L.lo_set_scan_overlap(None, 1) != 0 and o._L.lo_icp_flush(None) != 0
        assert o._L.lo_scan_overlap_status(o.ctx, None) != 0
    finally:
        o.close()
    monkeypatch.setenv("LO_OVERLAP", "0")
    o = _ctx(m)
    try:
        assert _queue_plain(o, six) == ref
        assert _overlapped(o) == 0
    finally:
        o.close()


def test_untouched_paths():
    """KDTree mode, the raw (device filter) path and a scan above the exact mode's one-workgroup limit: two queued
    scans each, equal to their solo runs, nothing overlapped."""
    import torch
    m, scans = _picked(True)
    # KDTree-mode context
    o = _ctx(m, kd=True)
    try:
        dev = [(*_dev(scans[0][0]), scans[0][1]), (*_dev(scans[3][0]), scans[3][1])]
        _, ref = _solo(o, dev)
        assert _queue_plain(o, dev) == ref[1]
        assert _queue_plain(o, dev[::-1]) == ref[0]
        assert _overlapped(o) == 0
    finally:
        o.close()
    o = _ctx(m, max_points=1 << 16)
    try:
        # raw scans through the device voxel filter
        raws = [_data.kitti_scan(3), _data.kitti_scan(5)]
        Ts = [_data.kitti_case(3, last_kf=4)[2], _data.kitti_case(5, last_kf=4)[2]]
        d_raw = [torch.from_numpy(np.ascontiguousarray(r, np.float32)).to("cuda:0") for r in raws]

        def raw(i):
            T = np.ascontiguousarray(Ts[i], np.float32)
            assert o._L.lo_icp_optimize_raw_async(o.ctx, C.c_void_p(d_raw[i].data_ptr()), d_raw[i].shape[0], 8,
                                                  C.c_float(0.5), T.ctypes.data_as(C.POINTER(C.c_float))) == 0
        assert o._L.lo_set_scan_overlap(o.ctx, 0) == 0
        solo = []
        for i in (0, 1):
            raw(i)
            solo.append(_result(o))
        assert o._L.lo_set_scan_overlap(o.ctx, 1) == 0
        raw(0)
        raw(1)
        assert _result(o) == solo[1]
        raw(1)
        raw(0)
        assert _result(o) == solo[0]
        assert _overlapped(o) == 0
        # one scan above kExactMaxPoints (17k points), queued behind a small one and in front of one
        rng = np.random.default_rng(5)
        base = np.concatenate([scans[2][0]] * 12)[:17000]
        big = (base + rng.normal(0.0, 0.002, base.shape)).astype(np.float32)
        dbig = (*_dev(big), scans[2][1])
        small = (*_dev(scans[0][0]), scans[0][1])
        _, ref = _solo(o, [dbig, small])
        assert _queue_plain(o, [small, dbig]) == ref[0]
        assert _overlapped(o) == 0
        assert _queue_plain(o, [dbig, small]) == ref[1]
        assert _overlapped(o) == 0
    finally:
        o.close()
