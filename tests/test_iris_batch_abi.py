"""The batched LiDAR-Iris detector's surface without a GPU (include/lo_iris_batch.h): its symbols are exported and
bound, ``BatchIrisDetector`` is importable, and the selection rule -- now one implementation shared by
lo_iris_select_host, lo_iris_detect and lo_iris_batch_detect (csrc/lo_iris_body.h) -- still answers as before at each
of its boundaries."""
import ctypes as C

import numpy as np

from lidar_odometry_amd import LoopClosureConfig, _lib
from lidar_odometry_amd.iris import select_host

SYMBOLS = ("lo_iris_batch_create", "lo_iris_batch_destroy", "lo_iris_batch_last_error", "lo_iris_batch_size",
           "lo_iris_batch_capacity", "lo_iris_batch_clear", "lo_iris_batch_add", "lo_iris_batch_add_from_scans",
           "lo_iris_batch_detect", "lo_iris_batch_compare_all")


def test_symbols_are_exported_and_bound():
    raw = C.CDLL(_lib.LIB_PATH)
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in _lib.EXPORTED_SYMBOLS, s
        assert hasattr(raw, s), s
        assert getattr(L, s).argtypes is not None, s
    assert L.lo_iris_batch_create.restype is C.c_void_p
    assert L.lo_iris_batch_last_error.restype is C.c_char_p
    assert L.lo_iris_batch_size.restype is C.c_size_t and L.lo_iris_batch_capacity.restype is C.c_size_t
    assert len(L.lo_iris_batch_add.argtypes) == 9
    assert len(L.lo_iris_batch_add_from_scans.argtypes) == 6
    assert len(L.lo_iris_batch_detect.argtypes) == 11
    assert len(L.lo_iris_batch_compare_all.argtypes) == 12


def test_null_handles_are_refused_without_a_device():
    L = _lib.lib()
    err = C.c_int(0)
    assert not L.lo_iris_batch_create(None, 8, C.byref(err)) and err.value == _lib.LO_ERR_ARG
    assert L.lo_iris_batch_size(None, 0) == 0 and L.lo_iris_batch_capacity(None) == 0
    assert L.lo_iris_batch_clear(None, -1) == _lib.LO_ERR_ARG
    assert L.lo_iris_batch_last_error(None) == b"null detector"
    L.lo_iris_batch_destroy(None)


def test_python_class_is_exported():
    import lidar_odometry_amd
    from lidar_odometry_amd import BatchIrisDetector
    assert "BatchIrisDetector" in lidar_odometry_amd.__all__
    for name in ("add", "add_from_scans", "detect", "compare_all", "size", "clear"):
        assert callable(getattr(BatchIrisDetector, name)), name


# ------------------------------------------------------------------------------------------- the selection rule
CFG = LoopClosureConfig(0.3, 50, 10.0)
CUR = [0.0, 0.0, 0.0]


def _pick(ids, pos, dist, cfg=CFG, cur_id=100):
    return select_host(cfg, cur_id, CUR, ids, np.asarray(pos, np.float32), np.asarray(dist, np.float32))


def test_gap_exactly_the_minimum_is_eligible():
    assert _pick([50], [[1, 0, 0]], [0.1]) == 0                 # 100 - 50 = 50: not < 50
    assert _pick([51], [[1, 0, 0]], [0.1]) == -1                # 49
    assert _pick([51, 50], [[1, 0, 0], [1, 0, 0]], [0.05, 0.2]) == 1


def test_gap_is_taken_on_the_ids_cast_to_int():
    # (int)current_id - (int)id, as the reference: ids that differ by 2^32 have gap 0
    assert _pick([100 - (1 << 32)], [[1, 0, 0]], [0.1]) == -1


def test_distance_exactly_the_maximum_is_eligible():
    assert _pick([0], [[10.0, 0, 0]], [0.1]) == 0               # norm 10.0: not > 10
    assert _pick([0], [[6.0, 8.0, 0]], [0.1]) == 0              # sqrt(36 + 64) = 10 exactly in fp32
    assert _pick([0], [[np.nextafter(np.float32(10.0), np.float32(11.0)), 0, 0]], [0.1]) == -1
    assert _pick([0, 0], [[10.5, 0, 0], [10.0, 0, 0]], [0.01, 0.2]) == 1


def test_tie_goes_to_the_lower_index():
    assert _pick([0, 1, 2], [[1, 0, 0]] * 3, [0.2, 0.1, 0.1]) == 1
    assert _pick([0, 1, 2], [[1, 0, 0]] * 3, [0.0, 0.0, 0.0]) == 0
    # ... among the eligible ones only
    assert _pick([60, 1, 2], [[1, 0, 0]] * 3, [0.1, 0.1, 0.1]) == 1


def test_nan_is_skipped():
    nan = np.float32(np.nan)
    assert _pick([0, 1], [[1, 0, 0]] * 2, [nan, 0.25]) == 1
    assert _pick([0, 1], [[1, 0, 0]] * 2, [0.25, nan]) == 0
    assert _pick([0, 1], [[1, 0, 0]] * 2, [nan, nan]) == -1
    assert _pick([0, 1], [[1, 0, 0]] * 2, [nan, 0.5]) == -1     # the only number is above the threshold


def test_best_exactly_at_the_threshold_is_accepted():
    thr = np.float32(0.3)
    cfg = LoopClosureConfig(float(thr), 50, 10.0)
    assert _pick([0], [[1, 0, 0]], [thr], cfg) == 0
    assert _pick([0], [[1, 0, 0]], [np.nextafter(thr, np.float32(1.0))], cfg) == -1
    # the lowest distance decides alone: a worse entry under the threshold does not stand in for a best one above it
    assert _pick([0, 1], [[1, 0, 0]] * 2, [0.4, 0.5], cfg) == -1


def test_empty_database():
    assert _pick(np.zeros(0, np.int64), np.zeros((0, 3), np.float32), np.zeros(0, np.float32)) == -1
