"""GPU tests of the scan groups (lo_set_scan_group, csrc/lo_scan_group_plan.h): queued scans that leave as lockstep runs.

Bar: every record of a queue -- pose, status, iteration count, n_corr -- and the last scan's full lo_icp_result (pose,
statistics, every field of every iteration log) are bit-identical to the same scans run alone with overlap off, in
reference-exact and in fast mode.
The scans and their solo reference are those of tests/test_gpu_scan_depth.py (300-600 points, all of different sizes,
against the first keyframes' map, max_iterations 4; the iteration counts are the CPU oracle's and are asserted there).
The first scan of a queue on an idle context starts at once down the ring, so a queue of q scans is one ring scan and
then groups over the other q - 1; LEAD is that first scan in the queues that check a particular group.  A full group
always runs in lockstep; a partial one of fewer than five scans goes down the ring scan by scan (kGroupLockstepMin).
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import _data
from tests.test_gpu_scan_depth import QUEUE, _records, _reference, _scans
from tests.test_gpu_scan_overlap import _ctx, _dev, _enqueue, _overlapped, _result, _solo

pytestmark = pytest.mark.gpu

LO_ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 4
LEAD = 2
MIXED = (0, 1, 4, 3)                                                # places in QUEUE: 4 1 1 4 iterations


def _group_ctx(m, exact, g=G):
    o = _ctx(m)
    o.set_exact(exact)
    o.set_scan_group(g)
    return o


def _run(o, dev, order, ref_rec, ref_res, name, min_grouped=None):
    before = o.scan_group_status()[2]
    for k in order:
        _enqueue(o, *dev[k])
    rc, got = _records(o, min(len(order), 64))
    assert rc == 0, (name, rc)
    np.testing.assert_array_equal(got, ref_rec[list(order)[-64:]], err_msg=name)
    assert _result(o) == ref_res[order[-1]], name
    if min_grouped is not None:                                     # the lockstep path really ran
        assert o.scan_group_status()[2] - before >= min_grouped, (name, o.scan_group_status())


def test_mixed_order_holds_the_runs():
    assert [QUEUE[k][1] for k in MIXED] == [4, 1, 1, 4]
    _, scans = _scans()
    assert len({len(p) for p, _ in scans}) == len(scans)            # scans of different sizes in one group


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_group_records_equal_solo_bitwise(exact):
    ref_rec, ref_res = _reference(exact)
    m, scans = _scans()
    o = _group_ctx(m, exact)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        nq = len(dev)
        # a group of one (down the ring), partial, full, full + 1, two slots reused
        for q in (1, 2, 3, 4, 5, 6, 11, 14):
            order = [(3 * k + q) % nq for k in range(q)]
            r = q - 1
            _run(o, dev, order, ref_rec, ref_res, f"queue of {q}", min_grouped=G if r >= G else 0)
        _run(o, dev, (LEAD,) + MIXED, ref_rec, ref_res, "4 1 1 4", min_grouped=4)
        _run(o, dev, (LEAD,) + MIXED[::-1], ref_rec, ref_res, "4 1 1 4 reversed", min_grouped=4)
        # 70 queued scans: the last 64 records, in order
        _run(o, dev, [k % nq for k in range(70)], ref_rec, ref_res, "70 scans", min_grouped=G)
        # the default group size too
        o.set_scan_group(0)
        assert o.scan_group_status()[0] == 32
        _run(o, dev, [(5 * k) % nq for k in range(40)], ref_rec, ref_res, "default group", min_grouped=32)
    finally:
        o.close()


def test_group_off_is_the_ring():
    """g = 1: every queued scan takes the ring, overlaps are counted as before, no group is launched."""
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _group_ctx(m, True, g=1)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        base = _overlapped(o)
        _run(o, dev, range(len(dev)), ref_rec, ref_res, "g = 1")
        assert _overlapped(o) == base + len(dev) - 1
        assert o.scan_group_status()[1:3] == (0, 0)
    finally:
        o.close()


def test_empty_and_large_scans_inside_a_queue():
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _group_ctx(m, True)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        # an empty scan (LO_INSUFFICIENT) in the middle: it is not pipelined and ends the run of records, as ever
        empty = (*_dev(scans[0][0][:0]), scans[0][1])
        for d in (dev[2], dev[0], dev[1], empty, dev[4], dev[3], dev[5]):
            _enqueue(o, *d)
        assert _records(o, 4)[0] == LO_ERR_ARG
        rc, got = _records(o, 3)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[[4, 3, 5]])
        assert _result(o) == ref_res[5]
        for d in (dev[2], dev[0], dev[1], empty):                   # ... and as the last scan of the queue
            _enqueue(o, *d)
        r = _result(o)
        assert r[0] == 1 and r[1] == np.ascontiguousarray(scans[0][1], np.float32).tobytes()
        # a reference-exact scan beyond the lockstep limit (8192 points) in the middle: it falls back, order kept
        rng = np.random.default_rng(5)
        base = np.concatenate([scans[0][0]] * 30)[:9000]
        big = (*_dev((base + rng.normal(0.0, 0.002, base.shape)).astype(np.float32)), scans[0][1])
        assert 8192 < big[1] <= 16384
        big_rec, big_res = _solo(o, [big])
        before = o.scan_group_status()[2]
        for d in (dev[2], dev[0], dev[1], dev[5], dev[6], big, dev[4], dev[3]):
            _enqueue(o, *d)
        rc, got = _records(o, 8)
        assert rc == 0
        want = np.stack([ref_rec[2], ref_rec[0], ref_rec[1], ref_rec[5], ref_rec[6], big_rec[0], ref_rec[4], ref_rec[3]])
        np.testing.assert_array_equal(got, want)
        assert _result(o) == ref_res[3]
        assert o.scan_group_status()[2] - before >= G
        for d in (dev[2], dev[0], big):
            _enqueue(o, *d)
        assert _result(o) == big_res[0]
    finally:
        o.close()


def test_flush_points_mid_group():
    import torch
    ref_rec, ref_res = _reference(True)
    ref_rec_f, ref_res_f = _reference(False)
    m, scans = _scans()
    o = _group_ctx(m, True)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        # lo_icp_result in the middle of a group
        for k in (2, 0, 1):
            _enqueue(o, *dev[k])
        assert o.scan_group_status()[3] == 2                        # two scans wait in the open group
        assert _result(o) == ref_res[1]
        for k in (4, 3):
            _enqueue(o, *dev[k])
        assert _result(o) == ref_res[3]
        # lo_icp_export_pose
        rec = torch.zeros(16, dtype=torch.float32, device="cuda:0")
        for k in (2, 0, 1):
            _enqueue(o, *dev[k])
        assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(rec.data_ptr())) == 0
        assert o.scan_group_status()[3] == 0
        for k in (4, 3, 5):
            _enqueue(o, *dev[k])
        rc, got = _records(o, 6)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[[2, 0, 1, 4, 3, 5]])
        np.testing.assert_array_equal(rec.cpu().numpy().view(np.uint32), ref_rec[1])
        # lo_set_exact toggled: the scans before it ran in exact mode, the ones after it in fast mode
        for k in (2, 0, 1):
            _enqueue(o, *dev[k])
        o.set_exact(False)
        for k in (4, 3, 5):
            _enqueue(o, *dev[k])
        rc, got = _records(o, 6)
        assert rc == 0
        np.testing.assert_array_equal(got[:3], ref_rec[[2, 0, 1]])
        np.testing.assert_array_equal(got[3:], ref_rec_f[[4, 3, 5]])
        assert _result(o) == ref_res_f[5]
        o.set_exact(True)
        # the surfel table uploaded again with another map: scans before it saw the old map, scans after it the new one
        k_, n_, c_ = _data.surfels(m)
        o2 = _ctx(m)
        try:
            o2.set_surfels(k_[::2], n_[::2], c_[::2])
            new_rec, new_res = _solo(o2, [dev[4], dev[3], dev[5]])
        finally:
            o2.close()
        assert any(not np.array_equal(a, b) for a, b in zip(new_rec, ref_rec[[4, 3, 5]]))   # the maps do differ
        for k in (2, 0, 1):
            _enqueue(o, *dev[k])
        o.set_surfels(k_[::2], n_[::2], c_[::2])
        for k in (4, 3, 5):
            _enqueue(o, *dev[k])
        rc, got = _records(o, 6)
        assert rc == 0
        np.testing.assert_array_equal(got[:3], ref_rec[[2, 0, 1]])
        np.testing.assert_array_equal(got[3:], np.stack(new_rec))
        assert _result(o) == new_res[2]
    finally:
        o.close()


def test_setter_argument_checks():
    """lo_set_scan_group on a real context: 0 (default), 1 (off) and 2 .. 32 are accepted, anything else is LO_ERR_ARG and
    leaves the setting alone."""
    m, _ = _scans()
    o = _ctx(m)
    try:
        L = o._L
        for g in (0, 1, 2, 32):
            assert L.lo_set_scan_group(o.ctx, g) == 0, g
            assert o.scan_group_status()[0] == (32 if g == 0 else g)
        assert L.lo_set_scan_group(o.ctx, 7) == 0
        for g in (-1, 33, 64, -32):
            assert L.lo_set_scan_group(o.ctx, g) == LO_ERR_ARG, g
            assert o.scan_group_status()[0] == 7
        assert L.lo_scan_group_status(o.ctx, None) == LO_ERR_ARG
    finally:
        o.close()


def test_async_table_patch_between_two_bursts():
    """lo_map_patch_surfels is enqueued on the context stream with no host synchronise.  A burst of queued scans, the
    patch, a second burst at once: the second burst's groups must run behind the patch (the first burst's before it).
    The patch erases every other surfel, so a scan that saw the wrong table differs."""
    ref_rec, _ = _reference(True)
    m, scans = _scans()
    k_, n_, c_ = _data.surfels(m)
    keys = np.ascontiguousarray(k_[1::2], np.int32)
    nn, cc = np.ascontiguousarray(n_[1::2], np.float32), np.ascontiguousarray(c_[1::2], np.float32)
    gone = np.zeros(len(keys), np.uint8)
    dev = [(*_dev(p), Ti) for p, Ti in scans]
    nq = len(dev)
    o2 = _ctx(m)
    try:
        assert o2._L.lo_map_patch_surfels(o2.ctx, keys.ctypes.data, nn.ctypes.data, cc.ctypes.data, gone.ctypes.data,
                                          len(keys)) == 0          # the same patch, then every scan alone
        new_rec, new_res = _solo(o2, dev)
    finally:
        o2.close()
    new_rec = np.stack(new_rec)
    assert any(not np.array_equal(a, b) for a, b in zip(new_rec, ref_rec))   # the tables do differ
    for g in (G, 0):
        o = _group_ctx(m, True, g=g)
        try:
            first = [k % nq for k in range(1 + 2 * G)]
            second = [(3 * k + 1) % nq for k in range(2 * G + 3)]
            before = o.scan_group_status()[2]
            for k in first:
                _enqueue(o, *dev[k])
            assert o._L.lo_map_patch_surfels(o.ctx, keys.ctypes.data, nn.ctypes.data, cc.ctypes.data, gone.ctypes.data,
                                             len(keys)) == 0
            for k in second:
                _enqueue(o, *dev[k])
            rc, got = _records(o, len(first) + len(second))
            assert rc == 0
            np.testing.assert_array_equal(got[:len(first)], ref_rec[first], err_msg=f"before the patch, g={g}")
            np.testing.assert_array_equal(got[len(first):], new_rec[second], err_msg=f"after the patch, g={g}")
            assert _result(o) == new_res[second[-1]]
            assert o.scan_group_status()[2] - before >= 5
        finally:
            o.close()


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_ring_scans_behind_two_full_groups_at_the_default_size(exact):
    """64 grouped records in flight, then ring-path scans whose records reuse the first group's slots of the 64-record
    ring: 1 + 32 + 32 + 3 scans (the last three leave down the ring at the flush), and a scan that is not groupable
    (reference-exact above the lockstep limit; an empty one in fast mode) right behind two full groups."""
    ref_rec, ref_res = _reference(exact)
    m, scans = _scans()
    o = _group_ctx(m, exact, g=0)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        nq = len(dev)
        order = [(2 * k + 1) % nq for k in range(1 + 32 + 32 + 3)]
        before = o.scan_group_status()[2]
        for k in order:
            _enqueue(o, *dev[k])
        rc, got = _records(o, 64)
        assert rc == 0
        np.testing.assert_array_equal(got, ref_rec[order[-64:]])
        assert _result(o) == ref_res[order[-1]]
        assert o.scan_group_status()[2] - before >= 32
        # a scan that yields to the ring behind two full groups
        rng = np.random.default_rng(7)
        base = np.concatenate([scans[1][0]] * 30)[:9000]
        big = (*_dev((base + rng.normal(0.0, 0.002, base.shape)).astype(np.float32)), scans[1][1])
        odd = big if exact else (*_dev(scans[0][0][:0]), scans[0][1])
        odd_rec, odd_res = _solo(o, [odd])
        o.set_scan_group(0)
        order = [(3 * k) % nq for k in range(1 + 32 + 32)]
        for k in order:
            _enqueue(o, *dev[k])
        _enqueue(o, *odd)
        tail = [5, 2]
        for k in tail:
            _enqueue(o, *dev[k])
        if exact:                                                   # the large scan is pipelined: it leaves a record
            rc, got = _records(o, 64)
            assert rc == 0
            want = np.concatenate([ref_rec[order[-61:]], np.stack(odd_rec), ref_rec[tail]])
            np.testing.assert_array_equal(got, want)
        else:                                                       # the empty scan ends the run of records
            rc, got = _records(o, 2)
            assert rc == 0
            np.testing.assert_array_equal(got, ref_rec[tail])
            assert _records(o, 3)[0] == LO_ERR_ARG
        assert _result(o) == ref_res[tail[-1]]
    finally:
        o.close()


def test_idle_single_async_scan_starts_at_once():
    """A lone asynchronous scan on an idle context is launched by its own enqueue: nothing waits in the open group, and
    the context stream drains without any further call on the context."""
    import torch
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _group_ctx(m, True)
    try:
        own = torch.cuda.Stream("cuda:0")
        assert o._L.lo_set_stream(o.ctx, C.c_void_p(own.cuda_stream)) == 0
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        torch.cuda.synchronize()
        _enqueue(o, *dev[0])
        out = (C.c_longlong * 4)()
        assert o._L.lo_scan_group_status(o.ctx, out) == 0 and out[3] == 0      # (a getter: it launches nothing)
        t0 = time.monotonic()
        while not own.query():
            assert time.monotonic() - t0 < 5.0, "the scan's launches did not drain"
        assert _result(o) == ref_res[0]
        assert o._L.lo_set_stream(o.ctx, None) == 0
    finally:
        o.close()


def test_same_file_on_one_hardware_queue():
    """Every test above again in a child process with GPU_MAX_HW_QUEUES=1: the group streams, the ring's streams and the
    context stream then share one hardware queue, and nothing may depend on their running side by side."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1")
    r = subprocess.run([sys.executable, "-s", "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        "-m", "gpu", "-k", "not one_hardware_queue"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
