"""CPU tests of the batched map correction's boundary (lo_batch_apply_transform): exported by liblo_icp.so, declared
to the binding with its four argument types, declared in include/lo_map.h, and reachable from BatchOptimizer.  No GPU
call happens here."""
import ctypes as C
import os
import re

from lidar_odometry_amd import _lib

NAME = "lo_batch_apply_transform"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_batched_correction():
    assert hasattr(C.CDLL(_lib.LIB_PATH), NAME)


def test_binding_lists_it_with_four_argtypes():
    assert NAME in _lib.EXPORTED_SYMBOLS
    from lidar_odometry_amd import lib
    fn = getattr(lib(), NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 4
    assert fn.restype is C.c_int


def test_header_declares_it():
    with open(os.path.join(ROOT, "include", "lo_map.h")) as f:
        text = f.read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "include/lo_map.h does not declare " + NAME
    assert len(m.group(1).split(",")) == 4


def test_batch_optimizer_has_apply_transform():
    from lidar_odometry_amd.icp import BatchOptimizer
    assert callable(getattr(BatchOptimizer, "apply_transform", None))
