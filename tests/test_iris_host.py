"""CPU tests of the loop-closure detector's boundary (include/lo_iris.h): the library exports every declared entry
point, the package exports the Python class, and the context-free selection rule (lo_iris_select_host) equals the
numpy restatement of detect_loop_closures' choice (tests/_iris_ref.py).  No GPU call happens here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests import _iris_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "lo_iris.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(lo_[a-z0-9_]+)\s*\(", txt)))


def test_header_declares_the_entry_points_and_the_library_exports_them():
    names = _declared()
    for need in ("lo_iris_create", "lo_iris_destroy", "lo_iris_size", "lo_iris_clear", "lo_iris_last_error",
                 "lo_iris_image", "lo_iris_encode", "lo_iris_add_keyframe", "lo_iris_add_from_scan",
                 "lo_iris_compare_all", "lo_iris_detect", "lo_iris_select_host", "lo_iris_config_default"):
        assert need in names, need
    L = C.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(L, name), name
        assert name in _lib.EXPORTED_SYMBOLS, name


def test_package_exports_the_detector():
    import lidar_odometry_amd
    assert "IrisLoopDetector" in lidar_odometry_amd.__all__
    assert callable(lidar_odometry_amd.IrisLoopDetector)


def test_config_default():
    cfg = _lib.LoIrisConfig()
    _lib.lib().lo_iris_config_default(C.byref(cfg))
    assert (cfg.similarity_threshold, cfg.min_keyframe_gap, cfg.max_search_distance) == (np.float32(0.3), 50, 10.0)


def _both(cfg, cur_id, cur_pos, ids, pos, dist):
    from lidar_odometry_amd.iris import LoopClosureConfig, select_host
    got = select_host(LoopClosureConfig(*cfg), cur_id, cur_pos, ids, pos, dist)
    want = ref.select(cfg[0], cfg[1], cfg[2], cur_id, cur_pos, ids, pos, dist)
    assert got == want, (got, want)
    return got


CFG = (0.3, 50, 10.0)
ZERO = [0.0, 0.0, 0.0]


def test_select_gap_filter_at_the_boundary():
    # current 100: entry 51 has gap 49 (skipped although it is the closest), entry 50 has gap exactly 50 (kept)
    ids = [51, 50, 10]
    dist = [0.05, 0.20, 0.25]
    assert _both(CFG, 100, ZERO, ids, np.zeros((3, 3)), dist) == 1
    assert _both(CFG, 101, ZERO, ids, np.zeros((3, 3)), dist) == 0      # now 51 has gap 50


def test_select_distance_filter_at_the_limit():
    # 6-8-0 triangle: fp32 norm exactly 10 = the limit (kept: the test is >); one float above is skipped
    above = np.nextafter(np.float32(8.0), np.float32(9.0))
    pos = np.array([[6.0, above, 0.0], [6.0, 8.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    dist = [0.01, 0.10, 0.20]
    assert np.sqrt(np.float32(36.0) + above * above) > np.float32(10.0)
    assert _both(CFG, 100, ZERO, [0, 1, 2], pos, dist) == 1
    assert _both(CFG, 100, [0.0, above - np.float32(8.0), 0.0], [0, 1, 2], pos, dist) == 0


def test_select_skips_nan():
    dist = [np.nan, 0.2, np.nan]
    assert _both(CFG, 100, ZERO, [0, 1, 2], np.zeros((3, 3)), dist) == 1
    assert _both(CFG, 100, ZERO, [0, 2], np.zeros((2, 3)), [np.nan, np.nan]) == -1


def test_select_tie_goes_to_the_lower_index():
    dist = [0.25, 0.125, 0.125, 0.125]
    assert _both(CFG, 100, ZERO, [3, 2, 1, 0], np.zeros((4, 3)), dist) == 1


def test_select_nothing_under_the_threshold():
    t = np.float32(0.3)
    assert _both(CFG, 100, ZERO, [0, 1], np.zeros((2, 3)), [0.31, np.nextafter(t, np.float32(1.0))]) == -1
    assert _both(CFG, 100, ZERO, [0, 1], np.zeros((2, 3)), [0.31, t]) == 1           # exactly the threshold passes
    assert _both(CFG, 100, ZERO, [], np.zeros((0, 3)), []) == -1


def test_select_gap_uses_keyframe_ids_not_indices():
    assert _both(CFG, 60, ZERO, [5, 11], np.zeros((2, 3)), [0.2, 0.1]) == 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_select_random_against_numpy(seed):
    rng = np.random.default_rng(seed)
    n = 40
    ids = rng.permutation(200)[:n]
    pos = rng.uniform(-9.0, 9.0, (n, 3)).astype(np.float32)
    dist = rng.uniform(0.1, 0.6, n).astype(np.float32)
    dist[rng.integers(0, n, 4)] = np.nan
    for cur in (60, 120, 199):
        _both((0.35, 50, 10.0), cur, rng.uniform(-3, 3, 3), ids, pos, dist)
