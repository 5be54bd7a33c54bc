"""CPU tests of the raw-scan batch entry points' boundary: lo_batch_filter_raw and lo_batch_optimize_raw are declared
to the binding, exported by liblo_icp.so, and reachable from BatchOptimizer.  (Header / binding / link agreement of
every symbol: tests/test_abi.py and tests/test_header_abi.py.)  No GPU call happens here."""
import ctypes as C

from lidar_odometry_amd import _lib

NAMES = ("lo_batch_filter_raw", "lo_batch_optimize_raw")


def test_binding_declares_the_raw_batch_entry_points():
    for name in NAMES:
        assert name in _lib.EXPORTED_SYMBOLS, name


def test_library_exports_the_raw_batch_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name


def test_batch_optimizer_has_the_raw_methods():
    from lidar_odometry_amd.icp import BatchOptimizer
    assert callable(getattr(BatchOptimizer, "filter_raw", None))
    assert callable(getattr(BatchOptimizer, "optimize_raw", None))
