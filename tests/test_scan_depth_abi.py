"""CPU test of the scan-depth entry points (lo_set_scan_depth, lo_icp_queue_records): declared in include/lo_icp.h,
exported by the library, bound in lidar_odometry_amd/_lib.py with matching argument types, and their argument errors
that need no context.  No GPU call happens here."""
import ctypes as C
import os
import re

from lidar_odometry_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "lo_set_scan_depth": r"int\s+lo_set_scan_depth\s*\(\s*lo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;",
    "lo_icp_queue_records": r"int\s+lo_icp_queue_records\s*\(\s*lo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;",
}
BOUND = {
    "lo_set_scan_depth": [C.c_void_p, C.c_int],
    "lo_icp_queue_records": [C.c_void_p, C.c_int, C.POINTER(C.c_float)],
}


def test_header_declares_the_signatures():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lo_icp.h")).read(), flags=re.S)
    for name, pattern in DECLARED.items():
        assert re.search(pattern, txt), name


def test_library_exports_and_binding_types():
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, argtypes in BOUND.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert list(f.argtypes) == argtypes, (name, f.argtypes)
        assert f.restype is C.c_int, (name, f.restype)


def test_argument_errors_without_a_context():
    L = _lib.lib()
    out = (C.c_float * (16 * 65))()
    for depth in (0, 1, 2, 3):
        assert L.lo_set_scan_depth(None, depth) == _lib.LO_ERR_ARG
    for n_last in (-1, 0, 1, 64, 65):                    # a null context, with n_last in and out of range
        assert L.lo_icp_queue_records(None, n_last, out) == _lib.LO_ERR_ARG
    assert L.lo_icp_queue_records(None, 1, None) == _lib.LO_ERR_ARG


def test_optimizer_has_the_methods():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    assert callable(IterativeClosestPointOptimizer.set_scan_depth)
    assert callable(IterativeClosestPointOptimizer.queue_records)
