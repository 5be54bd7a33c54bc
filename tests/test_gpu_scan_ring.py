"""GPU tests of the scan ring (lo_set_scan_lanes): three or four queued scans in flight, scan k of a queue on lane
k % lanes with its own set of per-scan state, fence words and stream, and -- unless a split was chosen -- all its
Gauss-Newton iterations on that lane's stream (split 0: the context stream carries only holds and heads).

Bar: every record of a queue -- pose, status, iteration count, n_corr -- is bit-identical to the same scan run alone
with overlap off, in reference-exact and in fast mode.
The scans and their solo reference are those of tests/test_gpu_scan_depth.py (300-600 points against the first keyframes'
map, max_iterations 4; the iteration counts are the CPU oracle's and are asserted there).  RING orders them so that a
4-iteration scan is followed by two 1-iteration scans (places 0-2: scans k + 1 and k + 2 are final before k) and a
4, 4, 1 run follows (places 4-6).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_scan_depth import QUEUE, _pipe_status, _records, _reference, _scans
from tests.test_gpu_scan_overlap import _ctx, _dev, _enqueue, _overlapped, _queue_plain, _result

pytestmark = pytest.mark.gpu

LO_ERR_ARG = -1
LO_ERR_PIPELINE = -5
RING = (0, 1, 4, 2, 3, 0, 1, 5, 6)                                  # places in QUEUE: 4 1 1 2 4 4 1 3 2 iterations
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_order_holds_the_runs():
    its = [QUEUE[k][1] for k in RING]
    assert len(RING) >= 8 and its[0:3] == [4, 1, 1] and its[4:7] == [4, 4, 1]


def _lanes(o, n):
    assert o._L.lo_set_scan_lanes(o.ctx, n) == 0


def _run_queue(o, dev, order, ref_rec, ref_res, name):
    base = _overlapped(o)
    for k in order:
        _enqueue(o, *dev[k])
    rc, got = _records(o, len(order))
    assert rc == 0, (name, rc)
    assert _overlapped(o) == base + len(order) - 1, name
    np.testing.assert_array_equal(got, ref_rec[list(order)], err_msg=name)
    assert _result(o) == ref_res[order[-1]], name                   # the last scan's result is still there to take


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_ring_records_equal_solo_bitwise(exact):
    ref_rec, ref_res = _reference(exact)
    m, scans = _scans()
    o = _ctx(m)
    try:
        o.set_exact(exact)
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        for name, lanes, split in (("lanes3", 3, 0), ("lanes4", 4, 0), ("lanes3 split1", 3, 1)):
            _lanes(o, lanes)
            if split:
                o.set_pipeline(True, split)                         # an explicit split is obeyed at any depth
            _run_queue(o, dev, RING, ref_rec, ref_res, name)
            _run_queue(o, dev, RING[::-1], ref_rec, ref_res, name + " reversed")
        assert _pipe_status(o)[2] == 0
    finally:
        o.close()


def test_ring_hygiene_and_error_codes():
    """A queue of 5 at lanes 3, a synchronous call, lanes 2, a new queue, depth 1, a new queue: each equal to its solo
    run, and no wait timed out."""
    ref_rec, ref_res = _reference(True)
    m, scans = _scans()
    o = _ctx(m)
    try:
        dev = [(*_dev(p), Ti) for p, Ti in scans]
        assert o._L.lo_set_scan_lanes(o.ctx, 0) == LO_ERR_ARG and o._L.lo_set_scan_lanes(o.ctx, 5) == LO_ERR_ARG
        _lanes(o, 3)
        _run_queue(o, dev, RING[:5], ref_rec, ref_res, "lanes3")
        for k in RING[:5]:                                          # five more, left in flight in front of the call
            _enqueue(o, *dev[k])
        ok, To = o.optimize(None, scans[3][0], scans[3][1])         # a scan that needs all its iterations
        assert ok and np.asarray(To, np.float32).reshape(-1)[:12].tobytes() == ref_res[3][1]
        assert o.get_last_stats().num_iterations == ref_res[3][2]
        _lanes(o, 2)
        _run_queue(o, dev, RING[2:8], ref_rec, ref_res, "lanes2")
        assert o._L.lo_set_scan_depth(o.ctx, 1) == 0
        _run_queue(o, dev, RING[1:7], ref_rec, ref_res, "depth1")
        _lanes(o, 4)                                                # and up again, from whichever lane that ended on
        _run_queue(o, dev, RING, ref_rec, ref_res, "lanes4")
        assert _queue_plain(o, [dev[k] for k in RING[:4]]) == ref_res[RING[3]]
        assert _pipe_status(o)[2] == 0                              # no wait timed out
    finally:
        o.close()


def test_ring_forced_timeout_in_a_fresh_process():
    """LO_PIPE_FAIL_AT (bound 0: the wait gives up without waiting) at lanes 3, in a child process of its own
    (tests/_scan_ring_child.py): the flagged scan reports LO_ERR_PIPELINE, every scan in flight beside it is flagged or
    bit-identical (never silently different), the queue's records are refused with LO_ERR_PIPELINE, and the next
    enqueue runs on one stream and equals the solo run."""
    env = dict(os.environ)
    env.pop("LO_PIPE_FAIL_AT", None)
    r = subprocess.run([sys.executable, "-s", os.path.join(ROOT, "tests", "_scan_ring_child.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(out)
    # the flagged scan was the last of the queue
    assert out["last"]["flagged_status"] == LO_ERR_PIPELINE
    assert out["last"]["other_lane_status"] == LO_ERR_PIPELINE or out["last"]["other_lane_equal"]
    assert out["last"]["records_rc"] == LO_ERR_PIPELINE
    assert out["last"]["status"][0] == 0 and out["last"]["status"][2] == 1      # pipeline off, one timeout
    assert out["last"]["result_equal"] and out["last"]["reruns"] == 1          # re-run on one stream
    assert out["last"]["next_queue_equal"] and out["last"]["next_overlapped"] == 0
    # ... and in the middle of it
    assert out["middle"]["result_equal"]
    assert out["middle"]["status"][0] == 0 and out["middle"]["status"][2] == 1
    assert out["middle"]["later_equal"] == [True, True, True]
    assert out["middle"]["records_rc"] == LO_ERR_ARG                            # scans on one stream leave no record
