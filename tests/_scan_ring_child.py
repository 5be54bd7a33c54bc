"""Child process of tests/test_gpu_scan_ring.py::test_ring_forced_timeout_in_a_fresh_process: the forced pipeline
timeout (LO_PIPE_FAIL_AT, read at lo_create) with three scans in flight.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.test_gpu_scan_depth import _pipe_status, _records, _reference, _scans            # noqa: E402
from tests.test_gpu_scan_overlap import _ctx, _dev, _enqueue, _overlapped, _queue_plain, _result   # noqa: E402

ORDER = (1, 0, 2, 4, 3)                  # 1, 4, 2, 1, 4 iterations: the third and the last one need their tails


def _ring_ctx(m, fail_at):
    os.environ["LO_PIPE_FAIL_AT"] = str(fail_at)
    try:
        o = _ctx(m)
    finally:
        del os.environ["LO_PIPE_FAIL_AT"]
    assert o._L.lo_set_scan_lanes(o.ctx, 3) == 0
    return o


def main():
    import torch
    torch.zeros(1, device="cuda")                                    # torch's HIP runtime up before the library's
    ref_rec, ref_res = _reference(True)                              # (before the hook is set)
    m, scans = _scans()
    dev = [(*_dev(p), Ti) for p, Ti in scans]
    out = {}

    # the LAST scan of the queue is the flagged one: nothing is enqueued behind it, so the host has not recovered yet
    o = _ring_ctx(m, len(ORDER))
    try:
        for k in ORDER:
            _enqueue(o, *dev[k])
        rec = torch.zeros(16, dtype=torch.float32, device="cuda:0")
        assert o._L.lo_icp_export_pose(o.ctx, C.c_void_p(rec.data_ptr())) == 0      # all holds, then this scan's state
        other = np.zeros(16, np.float32)
        assert o._L.lo_debug_other_lane_record(o.ctx, other.ctypes.data_as(C.POINTER(C.c_float))) == 0
        flagged = rec.cpu().numpy()
        rc, _ = _records(o, len(ORDER))                              # refused; the host recovers here
        st = _pipe_status(o)
        res = _result(o)                                             # the flagged scan again, on one stream
        st[3] = _pipe_status(o)[3]
        base = _overlapped(o)
        nxt = _queue_plain(o, [dev[3], dev[0]])
        out["last"] = {
            "flagged_status": int(flagged[12]),
            "other_lane_status": int(other[12]),
            "other_lane_equal": bool(np.array_equal(other.view(np.uint32), ref_rec[ORDER[-2]])),
            "records_rc": rc, "status": st, "result_equal": res == ref_res[ORDER[-1]], "reruns": st[3],
            "next_queue_equal": nxt == ref_res[0], "next_overlapped": _overlapped(o) - base,
        }
    finally:
        o.close()

    # the third of five: the scans behind it find the pipeline broken, or the host recovers at their enqueue
    o = _ring_ctx(m, 3)
    try:
        for k in ORDER:
            _enqueue(o, *dev[k])
        res = _result(o)
        st = _pipe_status(o)
        later = [_queue_plain(o, [dev[k - 1], dev[k]]) == ref_res[k] for k in (3, 4, 0)]
        out["middle"] = {"result_equal": res == ref_res[ORDER[-1]], "status": st, "later_equal": later,
                         "records_rc": _records(o, 1)[0]}
    finally:
        o.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
