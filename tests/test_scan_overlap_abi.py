"""CPU test of the scan-overlap entry points (lo_set_scan_overlap, lo_scan_overlap_status, lo_icp_flush): declared in
include/lo_icp.h with these signatures, exported by the library, and bound in lidar_odometry_amd/_lib.py with matching
argument types.  No GPU call happens here."""
import ctypes as C
import os
import re

from lidar_odometry_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECLARED = {
    "lo_set_scan_overlap": ("int", ["lo_ctx*", "int"]),
    "lo_scan_overlap_status": ("int", ["lo_ctx*", "long long[2]"]),
    "lo_icp_flush": ("int", ["lo_ctx*"]),
    "lo_debug_other_lane_record": ("int", ["lo_ctx*", "float[16]"]),
}
BOUND = {
    "lo_set_scan_overlap": [C.c_void_p, C.c_int],
    "lo_scan_overlap_status": [C.c_void_p, C.POINTER(C.c_longlong)],
    "lo_icp_flush": [C.c_void_p],
    "lo_debug_other_lane_record": [C.c_void_p, C.POINTER(C.c_float)],
}


def _header():
    txt = open(os.path.join(ROOT, "include", "lo_icp.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_signatures():
    txt = _header()
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


def test_null_context_is_an_argument_error():
    L = _lib.lib()
    assert L.lo_set_scan_overlap(None, 1) == _lib.LO_ERR_ARG
    assert L.lo_icp_flush(None) == _lib.LO_ERR_ARG
    assert L.lo_scan_overlap_status(None, (C.c_longlong * 2)()) == _lib.LO_ERR_ARG
