"""CPU tests of the batched map update's and the batched frame loop's boundary: the new C entry points are declared
to the binding and exported by liblo_icp.so, and the Python classes reach them.  (Header / binding / link agreement of
every symbol: tests/test_abi.py and tests/test_header_abi.py.)  No GPU call happens here."""
import ctypes as C

from lidar_odometry_amd import _lib

MAP_NAMES = ("lo_batch_update_maps", "lo_batch_maps_status")
ODOM_NAMES = ("lo_odom_batch_create", "lo_odom_batch_destroy", "lo_odom_batch_last_error",
              "lo_odom_batch_set_initial_pose", "lo_odom_batch_set_exact", "lo_odom_batch_process", "lo_odom_batch_flush",
              "lo_odom_batch_keyframe_count")


def test_binding_declares_the_batched_map_and_frame_loop_entry_points():
    for name in MAP_NAMES + ODOM_NAMES:
        assert name in _lib.EXPORTED_SYMBOLS, name


def test_library_exports_the_batched_map_and_frame_loop_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    for name in MAP_NAMES + ODOM_NAMES:
        assert hasattr(L, name), name


def test_python_classes_have_the_batched_methods():
    from lidar_odometry_amd.icp import BatchOptimizer
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    assert callable(getattr(BatchOptimizer, "update_maps", None))
    assert callable(getattr(BatchOptimizer, "maps_status", None))
    for name in ("process", "flush", "close"):
        assert callable(getattr(BatchLidarOdometry, name, None)), name
