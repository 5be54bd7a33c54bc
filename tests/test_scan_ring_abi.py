"""CPU test of the scan-ring entry point (lo_set_scan_lanes): declared in include/lo_icp.h, exported by the library,
bound in lidar_odometry_amd/_lib.py with matching argument types, and its argument error that needs no context.  No GPU
call happens here."""
import ctypes as C
import os
import re

from lidar_odometry_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_signature():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lo_icp.h")).read(), flags=re.S)
    assert re.search(r"int\s+lo_set_scan_lanes\s*\(\s*lo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", txt)


def test_library_exports_and_binding_types():
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    assert "lo_set_scan_lanes" in _lib.EXPORTED_SYMBOLS
    assert hasattr(raw, "lo_set_scan_lanes")
    assert list(L.lo_set_scan_lanes.argtypes) == [C.c_void_p, C.c_int]
    assert L.lo_set_scan_lanes.restype is C.c_int


def test_argument_error_without_a_context():
    L = _lib.lib()
    for lanes in (0, 1, 2, 3, 4, 5):
        assert L.lo_set_scan_lanes(None, lanes) == _lib.LO_ERR_ARG


def test_optimizer_has_the_method():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    assert callable(IterativeClosestPointOptimizer.set_scan_lanes)
