"""GPU tests of two queued scans in flight (lo_set_scan_depth) and of the record ring (lo_icp_queue_records).

With depth 2 a queued scan k enqueues the hold of scan k - 2 in front of its own head and leaves the hold of scan k - 1
pending: its Gauss-Newton iterations run beside scan k - 1's tail on the other lane, each lane with its own tail stream
and fence words, and the scans of a queue may become final out of order.

Bar: every record of a queue -- pose, status, iteration count, n_corr -- is bit-identical to the same scan run alone
with overlap off, in reference-exact and in fast mode, with depth 2, depth 1 and overlap off.
The scans are those of tests/test_gpu_scan_overlap.py's pool (300-600 points against the first keyframes' map,
max_iterations 4); their iteration counts were taken from the CPU oracle (oracle.icp_optimize) and are asserted, so
the queue is known to hold a 4-iteration scan followed by a 1-iteration one twice: there scan k is final before k - 1.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import _data
from tests.test_gpu_scan_overlap import _ctx as _ctx_default
from tests.test_gpu_scan_overlap import _dev, _enqueue, _overlapped, _queue_plain, _result, _scene, _solo

pytestmark = pytest.mark.gpu

LO_ERR_ARG = -1
LO_ERR_PIPELINE = -5
RING = 64
# (scan of the pool, GN iterations by the oracle): 4 -> 1 at places 0-1 and 3-4
QUEUE = (("f5s0.05", 4), ("f3s0.0", 1), ("f3s0.006", 2), ("f3s0.3", 4), ("f7s0.003", 1), ("f7s0.01", 3), ("f7s0.015", 2))
MODES = (("depth2", 1, 2), ("depth1", 1, 1), ("off", 0, 2))        # name, overlap, depth


def _ctx(m, **kw):
    """A context with two scans in flight chosen explicitly: the default keeps one while other contexts of the process
    have scans in flight, and nothing here should depend on what earlier tests left alive."""
    o = _ctx_default(m, **kw)
    assert o._L.lo_set_scan_depth(o.ctx, 2) == 0
    return o


@functools.lru_cache(maxsize=None)
def _scans():
    m, pool, _ = _scene()
    by_name = {name: (p, Ti) for name, p, Ti in pool}
    scans = [by_name[name] for name, _ in QUEUE]
    assert all(300 <= len(p) <= 600 for p, _ in scans)
    return m, scans


@functools.lru_cache(maxsize=None)
def _reference(exact):
    """Each scan of QUEUE alone, overlap off: (exported records as uint32 rows, lo_icp_result tuples).  Computed once per
    mode and shared; nothing changes it."""
    m, scans = _scans()
    o = _ctx(m)
    try:
        o.set_exact(exact)
        recs, res = _solo(o, [(*_dev(p), Ti) for p, Ti in scans])
    finally:
        o.close()
    recs = np.stack(recs)
    recs.setflags(write=False)
    assert [r[0] for r in res] == [0] * len(QUEUE)
    assert [r[2] for r in res] == [it for _, it in QUEUE], [r[2] for r in res]      # the oracle's iteration counts
    assert [int(x) for x in recs.view(np.float32)[:, 13]] == [it for _, it in QUEUE]
    return recs, tuple(res)


def _set(o, overlap, depth):
    assert o._L.lo_set_scan_overlap(o.ctx, overlap) == 0
    assert o._L.lo_set_scan_depth(o.ctx, depth) == 0


def _records(o, n):
    out = np.zeros((max(n, 1), 16), np.float32)
    rc = o._L.lo_icp_queue_records(o.ctx, n, out.ctypes.data_as(C.POINTER(C.c_float)))
    return rc, out[:n].view(np.uint32)


def _pipe_status(o):
    st = (C.c_int * 4)()
    assert o._L.lo_pipeline_status(o.ctx, st) == 0
    return list(st)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_queue_records_equal_solo_bitwise(exact):
    ref_rec, ref_res = _reference(exact)
    m, scans = _scans()
    o = _ctx(m)
    try:
        o.set_exact(exact)
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        for name, overlap, depth in MODES:
            _set(o, overlap, depth)
            base = _overlapped(o)
            for d in dev:
                _enqueue(o, *d)
            rc, got = _records(o, len(dev))
            assert rc == 0, (name, rc)
            assert _overlapped(o) == base + (len(dev) - 1 if overlap else 0), name
            np.testing.assert_array_equal(got, ref_rec, err_msg=name)
            assert _result(o) == ref_res[-1], name                  # the last scan's result is still there to take
            # the queue turned round: 1 -> 4 and 2 -> 4 neighbours, and another scan read as the last one
            for d in dev[::-1]:
                _enqueue(o, *d)
            rc, got = _records(o, len(dev))
            assert rc == 0, (name, rc)
            np.testing.assert_array_equal(got, ref_rec[::-1], err_msg=name + " reversed")
            assert _result(o) == ref_res[0], name
        assert _pipe_status(o)[2] == 0
        assert o._L.lo_set_scan_depth(o.ctx, 0) == LO_ERR_ARG and o._L.lo_set_scan_depth(o.ctx, 3) == LO_ERR_ARG
    finally:
        o.close()


def test_lane_hygiene():
    """A queue of 5, a synchronous call, a raw (device filter) scan, a new queue: each equal to its solo run."""
    import torch
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _ctx(m, max_points=1 << 16)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        raw = np.ascontiguousarray(_data.kitti_scan(3), np.float32)
        d_raw = torch.from_numpy(raw).to("cuda:0")
        T_raw = np.ascontiguousarray(_data.kitti_case(3, last_kf=4)[2], np.float32)

        def raw_async():
            assert o._L.lo_icp_optimize_raw_async(o.ctx, C.c_void_p(d_raw.data_ptr()), d_raw.shape[0], 8, C.c_float(0.5),
                                                  T_raw.ctypes.data_as(C.POINTER(C.c_float))) == 0

        _set(o, 0, 2)
        raw_async()
        solo_raw = _result(o)
        _set(o, 1, 2)
        for rep in range(2):
            for d in dev[:5]:
                _enqueue(o, *d)
            rc, got = _records(o, 5)
            assert rc == 0
            np.testing.assert_array_equal(got, ref_rec[:5], err_msg=f"queue {rep}")
            # a synchronous call of a scan that needs all its iterations, on whichever lane the queue ended
            ok, To = o.optimize(None, scans[3][0], scans[3][1])
            assert ok and np.asarray(To, np.float32).reshape(-1)[:12].tobytes() == ref_res[3][1]
            assert o.get_last_stats().num_iterations == ref_res[3][2]
            _enqueue(o, *dev[0])                                    # one hold pending in front of the raw call
            raw_async()
            assert _result(o) == solo_raw, f"raw {rep}"
            _enqueue(o, *dev[5])                                    # two pending in front of it
            _enqueue(o, *dev[0])
            raw_async()
            assert _result(o) == solo_raw, f"raw behind two holds {rep}"
        assert _queue_plain(o, dev) == ref_res[-1]
        assert _pipe_status(o)[2] == 0                              # no wait timed out
    finally:
        o.close()


def test_flush_with_two_holds_pending():
    """lo_icp_flush with two holds pending orders the shared stream behind both scans: the caller's own work enqueued
    there afterwards -- a copy of the exported record, then a kernel that clears the last two scans' points -- sees the
    last scan's final pose and changes no result."""
    import torch
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _ctx(m)
    own = torch.cuda.Stream("cuda:0")
    try:
        assert o._L.lo_set_stream(o.ctx, C.c_void_p(own.cuda_stream)) == 0
        for last in (3, 4):                                         # a 4-iteration and a 1-iteration scan read last
            dev = [(*_dev(p), Ti) for p, Ti in scans]
            order = [k for k in range(len(dev)) if k != last][:3] + [last]
            rec = torch.zeros(16, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            base = _overlapped(o)
            for k in order:
                _enqueue(o, *dev[k])
            assert _overlapped(o) == base + 3                       # nothing flushed: the last two holds are pending
            assert o._L.lo_icp_flush(o.ctx) == 0
            assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(rec.data_ptr())) == 0
            with torch.cuda.stream(own):
                mine = rec.clone()                                  # the caller's copy kernel, on the shared stream
                dev[order[-1]][0].zero_()                           # ... and the points a running tail would still read
                dev[order[-2]][0].zero_()
            own.synchronize()
            np.testing.assert_array_equal(mine.cpu().numpy().view(np.uint32), ref_rec[last])
            rc, got = _records(o, 4)
            assert rc == 0
            np.testing.assert_array_equal(got, ref_rec[order])
        assert o._L.lo_set_stream(o.ctx, None) == 0
    finally:
        o.close()


def test_recovery_in_the_middle_of_a_queue(monkeypatch):
    """LO_PIPE_FAIL_AT=3 (bound 0: the third pipelined scan's tail wait gives up without waiting) in a queue of 5: the
    pipeline switches off, the host call returns no error, and later scans run on one stream, bit-identical."""
    ref_rec, ref_res = _reference(True)                             # (before the hook is set)
    m, scans = _scans()
    monkeypatch.setenv("LO_PIPE_FAIL_AT", "3")
    o = _ctx(m)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        # 1, 4, 2, 1, 4 iterations: the forced scan and the last one both need their tails, so the last scan cannot
        # end before the broken pipeline is seen -- by the host at an enqueue, or by the scan's own waits
        for k in (1, 0, 2, 4, 3):
            _enqueue(o, *dev[k])
        assert _result(o) == ref_res[3]                             # rc 0: re-run on one stream if its own wait gave up
        st = _pipe_status(o)
        assert st[0] == 0 and st[2] == 1, st                        # pipeline off, one timeout
        for k in (3, 4, 0):
            assert _queue_plain(o, [dev[k - 1], dev[k]]) == ref_res[k], k
        rc, _ = _records(o, 1)
        assert rc == LO_ERR_ARG                                     # scans on one stream leave no record
        assert _pipe_status(o)[2] == 1
    finally:
        o.close()


def test_ring_bounds_and_wrap_around():
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _ctx(m)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        assert _records(o, 1)[0] == LO_ERR_ARG                      # nothing queued yet
        assert _records(o, 0)[0] == 0
        for d in dev[:3]:
            _enqueue(o, *d)
        assert _records(o, 4)[0] == LO_ERR_ARG                      # more than were queued
        assert _records(o, RING + 1)[0] == LO_ERR_ARG
        rc, got = _records(o, 2)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[1:3])
        total = 3
        order = [k % len(dev) for k in range(RING + 9)]             # past the ring's end, two scans in flight all along
        for k in order:
            _enqueue(o, *dev[k])
        total += len(order)
        assert total > RING and _records(o, RING + 1)[0] == LO_ERR_ARG
        rc, got = _records(o, RING)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[order[-RING:]])
        rc, got = _records(o, 5)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[order[-5:]])
        # a synchronous call of a pipelined scan adds its record; an empty scan is not pipelined and ends the run
        ok, _ = o.optimize(None, scans[2][0], scans[2][1])
        assert ok
        rc, got = _records(o, 2)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[[order[-1], 2]])
        empty = _dev(scans[0][0][:0])
        _enqueue(o, *empty, scans[0][1])
        assert _records(o, 1)[0] == LO_ERR_ARG
        _result(o)
        _enqueue(o, *dev[1])
        rc, got = _records(o, 1)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[1:2])
        assert _records(o, 2)[0] == LO_ERR_ARG
        _result(o)
    finally:
        o.close()
