"""CPU test of the scan-group entry points (lo_set_scan_group, lo_scan_group_status): declared in include/lo_icp.h with
these signatures, exported by the library, bound in lidar_odometry_amd/_lib.py with matching argument types, wrapped by
IterativeClosestPointOptimizer, and refusing a null context whatever the group size.  The range check of the group size
(0 .. 32 accepted, -1 and 33 refused) needs a context: tests/test_gpu_scan_group.py::test_setter_argument_checks.  No
GPU call happens here."""
import ctypes as C
import os
import re

from lidar_odometry_amd import _lib
from lidar_odometry_amd.icp import IterativeClosestPointOptimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "lo_set_scan_group": ("int", ["lo_ctx*", "int"]),
    "lo_scan_group_status": ("int", ["lo_ctx*", "long long[4]"]),
}
BOUND = {
    "lo_set_scan_group": [C.c_void_p, C.c_int],
    "lo_scan_group_status": [C.c_void_p, C.POINTER(C.c_longlong)],
}


def test_header_declares_the_signatures():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lo_icp.h")).read(), flags=re.S)
    for name, (ret, args) in DECLARED.items():
        m = re.search(r"\b(\w[\w ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, name
        assert m.group(1).strip() == ret, (name, m.group(1))
        got = []
        for a in m.group(2).split(","):
            a = a.strip()
            arr = re.search(r"(\[\d*\])$", a)
            a = re.sub(r"\s*\w+\s*(\[\d*\])?$", "", a)            # drop the parameter name
            got.append(a.replace(" *", "*") + (arr.group(1) if arr else ""))
        assert got == args, (name, got)


def test_library_exports_and_binding_types():
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for name, argtypes in BOUND.items():
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(raw, name), name
        f = getattr(L, name)
        assert list(f.argtypes) == argtypes, (name, f.argtypes)
        assert f.restype is C.c_int, (name, f.restype)
    assert callable(IterativeClosestPointOptimizer.set_scan_group)
    assert callable(IterativeClosestPointOptimizer.scan_group_status)


def test_argument_checks_without_a_context():
    L = _lib.lib()
    for g in (-1, 0, 1, 16, 32, 33):
        assert L.lo_set_scan_group(None, g) == _lib.LO_ERR_ARG
    assert L.lo_scan_group_status(None, (C.c_longlong * 4)()) == _lib.LO_ERR_ARG
