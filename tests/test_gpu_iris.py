"""GPU LiDAR-Iris loop-closure detector (include/lo_iris.h, csrc/lo_iris.hip) against the numpy restatement of its
definitions (tests/_iris_ref.py: the mathematical definition in fp64, not OpenCV's fp32 results).

Image: exact, on a cloud whose every binned quantity sits >= 1e-3 from a bin edge (asserted in fp64 first).
Encode: exact outside a band of 1e-6 around each threshold -- 100 x the fp64 rounding bound of a 360-point unscaled
transform of 0..255 inputs (~1e-8) -- which may cover at most 2 % of the non-empty rows' positions (asserted on the
numpy side alone); all-zero rows exactly T = 0, M = 255.
Match: integer popcounts and one fp32 division, so exact (bit for bit) against numpy run on the bits read back.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests import _data
from tests import _iris_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 17)
    yield o
    o.close()


@pytest.fixture()
def det(icp):
    from lidar_odometry_amd import IrisLoopDetector
    d = IrisLoopDetector(icp, capacity=8)
    yield d
    d.close()


@pytest.fixture(scope="module")
def clouds():
    """The query scene, a copy turned by +73 degrees (shifted and noisy), an unrelated scene."""
    a = ref.scene(1)
    return a, ref.yawed(a, 73, (0.3, -0.2, 0.0), 0.02, 3), ref.scene(2)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _desc(det, cloud):
    T, M = det.encode(det.image(cloud))
    return T, M


def _numpy_records(q, entries):
    out = []
    for e in entries:
        d, t = ref.hamming_all_shifts(q[0], q[1], e[0], e[1])
        out.append(ref.best_shift(d, t))
    return out


def _assert_records(got, want):
    dist, bias, diff, total = got
    assert len(dist) == len(want)
    for i, (wd, wb, wdiff, wtot) in enumerate(want):
        assert (int(bias[i]), int(diff[i]), int(total[i])) == (wb, wdiff, wtot), i
        assert _bits(dist[i]) == _bits(wd) or (np.isnan(dist[i]) and np.isnan(wd)), (i, dist[i], wd)


# ---------------------------------------------------------------------------------------------------- image
def _binned_cloud():
    rng = np.random.default_rng(11)
    n = 2880
    i = np.arange(n)
    r_bin, y_bin, h_bit = i % 80, i % 360, (i // 3) % 8
    rang = r_bin + rng.uniform(0.05, 0.95, n)
    v = rng.uniform(0.05, 0.95, n)
    v[y_bin == 0] = rng.uniform(0.55, 0.95, int((y_bin == 0).sum()))      # bin 0 is only yaw in [0, 0.5)
    ang = np.radians(y_bin + v - 0.5 - 180.0)
    z = h_bit - 1 + rng.uniform(0.05, 0.95, n) - 5.0
    pts = np.stack([rang * np.cos(ang), rang * np.sin(ang), z], 1)
    extra = np.array([
        [95.3 * np.cos(0.3), 95.3 * np.sin(0.3), 0.4],      # range > 80: row 79
        [-200.7, 3.1, -0.6],                                # far, yaw + 0.5 just under 360
        [np.cos(np.radians(179.7)) * 7.4, np.sin(np.radians(179.7)) * 7.4, 0.3],   # yaw + 0.5 = 360.2: clamps to 359
        [3.3, 4.2, -7.3],                                   # z < -5: bit 0
        [-5.4, 2.2, 4.6],                                   # z > 3: bit 7
        [0.0, 0.0, 1.3],                                    # the sensor axis: range 0, atan2(0, 0) = 0
    ])
    return np.concatenate([pts, extra]).astype(np.float32)


def test_image_exact(det):
    pts = _binned_cloud()
    assert ref.edge_margin(pts) >= 1e-3
    want = ref.image(pts)
    assert (want.sum(1) > 0).all() and (want.sum(0) > 0).all()                  # all 80 rows, all 360 columns
    assert np.bitwise_or.reduce(want.ravel()) == 255                            # all 8 height bits
    np.testing.assert_array_equal(det.image(pts), want)


def test_image_one_point_and_empty(det):
    p = np.array([[12.4, -3.3, 0.7]], np.float32)
    assert ref.edge_margin(p) >= 1e-3
    want = ref.image(p)
    assert np.count_nonzero(want) == 1
    np.testing.assert_array_equal(det.image(p), want)
    assert not det.image(np.zeros((0, 3), np.float32)).any()


def test_empty_cloud_adds_nothing(det):
    L = _lib.lib()
    pos = (C.c_float * 3)(0, 0, 0)
    dummy = np.zeros((1, 3), np.float32)
    assert L.lo_iris_add_keyframe(det._h, 5, pos, dummy.ctypes.data, 0, 0) == _lib.LO_INSUFFICIENT
    assert not det.add_keyframe(5, [0, 0, 0], np.zeros((0, 3), np.float32))
    assert len(det) == 0
    assert det.compare_all(np.zeros((0, 3), np.float32)) is None


def test_device_pointer_input_equals_host(det, clouds):
    import torch
    a, b, c = clouds
    det.add_keyframe(0, [0, 0, 0], b)
    det.add_keyframe(1, [0, 0, 0], torch.from_numpy(b).cuda())
    det.add_keyframe(2, [0, 0, 0], c)
    host = det.compare_all(a)
    dev = det.compare_all(torch.from_numpy(a).cuda())
    for h, d in zip(host, dev):
        np.testing.assert_array_equal(h.view(np.uint32), d.view(np.uint32))
    for k in range(4):
        assert host[k][0:1].view(np.uint32) == host[k][1:2].view(np.uint32)     # entry 0 (host) = entry 1 (device)


# ---------------------------------------------------------------------------------------------------- encode
def test_encode_exact_outside_the_band(det, clouds):
    img = ref.image(clouds[0])
    img[70:] = 0
    full = img.sum(1) > 0
    assert full.sum() >= 40 and (~full).sum() >= 10
    T_ref, M_ref, V = ref.encode(img)
    part = np.concatenate([V.real, V.imag]).reshape(640, 360)
    mag = np.concatenate([np.abs(V), np.abs(V)]).reshape(640, 360)
    rows = np.tile(full, 8)
    band_T = (np.abs(part) < 1e-6) & rows[:, None]
    band_M = np.abs(mag - 1e-4) < 1e-6
    n_pos = rows.sum() * 360
    assert band_T.sum() <= 0.02 * n_pos and band_M.sum() <= 0.02 * n_pos, (band_T.sum(), band_M.sum(), n_pos)
    T, M = det.encode(img)
    assert set(np.unique(T)) <= {0, 255} and set(np.unique(M)) <= {0, 255}
    # all-zero image rows: T = 0 and M = 255 exactly
    assert not T[~rows].any() and (M[~rows] == 255).all()
    ok = rows[:, None] & ~band_T
    np.testing.assert_array_equal(T[ok], T_ref[ok])
    np.testing.assert_array_equal(M[~band_M], M_ref[~band_M])


# ---------------------------------------------------------------------------------------------------- match
def test_compare_all_exact(det, clouds):
    a, b, c = clouds
    for k, p in enumerate((a, b, c)):
        assert det.add_keyframe(k, [0, 0, 0], p)
    assert len(det) == 3
    descs = [_desc(det, p) for p in (a, b, c)]
    want = _numpy_records(descs[0], descs)
    # the packed-byte numpy loop against the definition itself, at the winning shift of the rotated copy
    assert ref.hamming_at_shift(*descs[0], *descs[1], want[1][1]) == (want[1][2], want[1][3])
    got = det.compare_all(a)
    _assert_records(got, want)
    assert got[0][0] == 0.0 and got[1][0] == 0 and got[2][0] == 0              # itself: distance 0 at shift 0
    assert got[3][0] == ref.BITS - int((descs[0][1] > 0).sum())


def test_fully_masked_pair_is_nan(det, clouds):
    a = clouds[0]
    far = np.array([[100.0, 0.3, 0.2]], np.float32)        # one point beyond 80 m: only image row 79 is live
    assert not ref.image(a)[79].any()                      # the query has nothing there: every bit is masked
    assert det.add_keyframe(0, [0, 0, 0], far)
    assert det.add_keyframe(1, [0, 0, 0], a)
    want = _numpy_records(_desc(det, a), [_desc(det, far), _desc(det, a)])
    assert np.isnan(want[0][0]) and want[0][1:] == (-1, 0, 0)
    dist, bias, diff, total = det.compare_all(a)
    _assert_records((dist, bias, diff, total), want)
    assert np.isnan(dist[0]) and (bias[0], diff[0], total[0]) == (-1, 0, 0)
    assert dist[1] == 0.0


@pytest.mark.parametrize("angle", [73, -20])
def test_rotation_is_the_bias(det, clouds, angle):
    a, _, c = clouds
    turned = ref.yawed(a, angle, (0.25, -0.15, 0.0), 0.02, 5)
    det.add_keyframe(0, [0, 0, 0], turned)
    det.add_keyframe(1, [0, 0, 0], c)
    dist, bias, _, _ = det.compare_all(a)
    assert bias[0] == angle % 360
    assert dist[0] < dist[1]


# ---------------------------------------------------------------------------------------------------- detect
def _fill(det, clouds):
    a, b, c = clouds
    entries = [(0, [1.0, 0.0, 0.0], c), (10, [2.0, 1.0, 0.0], b), (20, [30.0, 0.0, 0.0], a),
               (70, [0.5, 0.5, 0.0], a), (30, [3.0, -2.0, 0.5], ref.scene(3))]
    for kid, pos, p in entries:
        assert det.add_keyframe(kid, pos, p)
    return [e[0] for e in entries], np.array([e[1] for e in entries], np.float32)


def test_detect_equals_the_selection_rule(det, clouds):
    from lidar_odometry_amd import LoopClosureConfig
    ids, pos = _fill(det, clouds)
    a = clouds[0]
    cur_id, cur_pos = 100, [0.0, 0.0, 0.0]
    dist = det.compare_all(a)[0]
    assert dist[2] == 0.0 and dist[3] == 0.0                # the scene itself, twice
    cases = [LoopClosureConfig(),                           # entry 2 is 30 m away, entry 3 has gap 30: entry 1 is left
             LoopClosureConfig(0.3, 30, 10.0),              # gap 30 admits entry 3
             LoopClosureConfig(0.3, 50, 40.0),              # 40 m admits entry 2
             LoopClosureConfig(0.3, 30, 40.0),              # both: a tie at 0, the lower index wins
             LoopClosureConfig(0.1, 50, 10.0),              # nothing under the threshold
             LoopClosureConfig(0.3, 95, 10.0)]              # the gap leaves entry 0 only (unrelated scene)
    picks = []
    for cfg in cases:
        want = ref.select(cfg.similarity_threshold, cfg.min_keyframe_gap, cfg.max_search_distance, cur_id, cur_pos,
                          ids, pos, dist)
        cand = det.detect(cur_id, cur_pos, a, cfg)
        picks.append(want)
        if want < 0:
            assert cand is None
        else:
            bias = det.compare_all(a)[1]
            assert (cand.query_keyframe_id, cand.match_keyframe_id, cand.bias) == (cur_id, ids[want], int(bias[want]))
            assert _bits(cand.similarity_score) == _bits(dist[want])
    assert picks == [1, 3, 2, 2, -1, -1]
    assert len(det) == 5                                    # detect adds nothing


def test_capacity_and_clear(icp, clouds):
    from lidar_odometry_amd import IrisLoopDetector
    a, b, c = clouds
    d = IrisLoopDetector(icp, capacity=2)
    try:
        assert d.capacity == 2
        assert d.add_keyframe(0, [0, 0, 0], a) and d.add_keyframe(1, [0, 0, 0], b)
        pos = (C.c_float * 3)(0, 0, 0)
        assert _lib.lib().lo_iris_add_keyframe(d._h, 2, pos, c.ctypes.data, len(c), 0) == _lib.LO_ERR_CAPACITY
        assert len(d) == 2
        with pytest.raises(RuntimeError):
            d.add_keyframe(2, [0, 0, 0], c)
        d.clear()
        assert len(d) == 0
        assert len(d.compare_all(a)[0]) == 0 and d.detect(100, [0, 0, 0], a) is None
        assert d.add_keyframe(7, [0, 0, 0], c)
        assert d.compare_all(c)[0][0] == 0.0
    finally:
        d.close()


def test_add_from_scan_equals_the_host_copy(icp, det, clouds):
    m, _, Ti, _ = _data.kitti_case(17)
    icp.set_surfels(*_data.surfels(m))
    icp.optimize_raw(None, _data.kitti_scan(17), Ti, stride=8, voxel_size=0.5)
    assert det.add_from_scan(0, [0, 0, 0])
    host = icp.filtered_points()
    assert len(host) > 1000
    assert det.add_keyframe(1, [0, 0, 0], host)
    for q in (host, clouds[0]):
        rec = det.compare_all(q)
        for k in range(4):
            assert rec[k][0:1].view(np.uint32) == rec[k][1:2].view(np.uint32)
    assert det.compare_all(host)[0][0] == 0.0


# ---------------------------------------------------------------------------------------------------- end to end
def test_loop_pair_end_to_end(icp, det):
    """The detector finds loop_case's matched keyframe among unrelated ones, and neither the loop ICP on that pair
    nor the context's map and next optimize notice that it ran."""
    m, pts, Ti, _ = _data.kitti_case(11)
    icp.set_surfels(*_data.surfels(m))
    _, A = icp.optimize(None, pts, Ti)
    cur, Tc, mat, Tm, _ = _data.loop_case(2, 6)
    loop_before = icp.optimize_loop(cur, Tc, mat, Tm)

    far = np.array([3.0, 3.0, 0.0], np.float32)
    assert det.add_keyframe(3, far, ref.scene(5))
    assert det.add_keyframe(5, np.asarray(Tm)[3::4], mat)
    assert det.add_keyframe(8, far, ref.scene(6))
    cand = det.detect(60, np.asarray(Tc)[3::4], cur)
    assert cand is not None and (cand.query_keyframe_id, cand.match_keyframe_id) == (60, 5)
    dist = det.compare_all(cur)[0]
    assert dist[1] < dist[0] and dist[1] < dist[2] and cand.similarity_score == dist[1]

    loop_after = icp.optimize_loop(cur, Tc, mat, Tm)
    assert loop_after[0] == loop_before[0] and loop_after[0]
    np.testing.assert_array_equal(np.asarray(loop_after[1]), np.asarray(loop_before[1]))
    assert loop_after[2] == loop_before[2]
    _, B = icp.optimize(None, pts, Ti)
    np.testing.assert_array_equal(np.asarray(A), np.asarray(B))
