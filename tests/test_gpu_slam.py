"""Loop closure in the frame loop (lo_odom_enable_loop_closure, include/lo_odometry.h) on the GPU.

The sequence revisits itself: frames 0..K of kitti_seq(40), then K-1..0 -- the sensor retraces its path, so a returning
keyframe sees the very scan an outbound one saw.  K, the keyframe gap and the cooldown are chosen so that the
ASSEMBLED-BY-HAND run (tests/_slam_ref.py: the same frames through the public pieces, host keyframe clouds) closes at
least one loop; that is asserted on the reference run, not on the code under test.

Composition equality: lo_odom with loop closure must equal that run BIT FOR BIT -- every frame's pose, the keyframe
flags, the loop events, the corrected keyframe poses and the built map.  Every SE3f product of the bookkeeping is
reproduced through the oracle's restatement of the reference's SE3f algebra (oracle.se3_compose / se3_inverse), so no
quantity needs the 1e-6 allowance.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests import _data

pytestmark = pytest.mark.gpu

K = 16
MAP_VOXEL = 0.4
MAX_POINTS = 1 << 15


def _cfg(**kw):
    from lidar_odometry_amd.odometry import LoopConfig
    base = dict(min_keyframe_gap=6, cooldown_keyframes=6, max_search_distance=10.0, max_keyframes=64,
                max_points=1 << 18)
    base.update(kw)
    return LoopConfig(**base)


@pytest.fixture(scope="module")
def scans():
    order = list(range(K + 1)) + list(range(K - 1, -1, -1))
    return [_data.kitti_scan(i, 40) for i in order]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _odom_run(scans, cfg, kdtree=False, after=None):
    """The frames through LidarOdometry -> (poses, status, keyframe flags, events per keyframe, loop count, kf poses, map)."""
    from lidar_odometry_amd.odometry import LidarOdometry
    o = LidarOdometry(max_points=MAX_POINTS, use_surfel_correspondence=not kdtree)
    try:
        if cfg is not None:
            o.enable_loop_closure(cfg)
        poses, status, flags, events, guesses, edges = [], [], [], [], [], []
        for raw in scans:
            T, info = o.process(raw)
            poses.append(T.reshape(12).copy())
            status.append(info.status)
            flags.append(info.keyframe)
            guesses.append(info.guess)
            if info.keyframe and cfg is not None:
                e = o.last_loop
                edges.append(e.odom_edge)
                events.append((e.keyframe_id, e.queried, e.candidate_id, np.float32(e.candidate_distance),
                               e.candidate_bias, np.float32(e.inlier_ratio), e.accepted))
        o.flush()
        out = {"poses": poses, "status": status, "flags": flags, "events": events, "guesses": guesses, "edges": edges}
        if cfg is not None:
            out["loops"] = o.loop_count
            out["kf_ids"], out["kf_poses"] = o.keyframe_poses()
            out["map"] = o.build_map(MAP_VOXEL)
            out["surfels"] = o.map_surfels
        if after is not None:
            after(o, out)
        return out
    finally:
        o.close()


@pytest.fixture(scope="module")
def ref_run(scans):
    from tests import _slam_ref
    return _slam_ref.run(scans, _cfg(), MAP_VOXEL, max_points=MAX_POINTS)


@pytest.fixture(scope="module")
def odom_run(scans):
    return _odom_run(scans, _cfg())


def test_the_reference_run_closes_a_loop(ref_run):
    """The choice of K, gap and threshold, verified on the run assembled by hand."""
    assert ref_run.loops >= 1
    assert any(e[6] for e in ref_run.events)
    assert all(s == _lib.LO_OK for s in ref_run.status)


def test_composition_equality(ref_run, odom_run):
    """lo_odom with loop closure == the same public calls made by hand, bit for bit."""
    assert odom_run["flags"] == ref_run.keyframe
    assert odom_run["status"] == ref_run.status
    for k, (a, b) in enumerate(zip(odom_run["poses"], ref_run.poses)):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"frame {k}")
    assert len(odom_run["events"]) == len(ref_run.events)
    for a, b in zip(odom_run["events"], ref_run.events):
        assert a[:3] == b[:3] and a[4] == b[4] and a[6] == b[6], (a, b)
        assert _bits(a[3]) == _bits(b[3]) and _bits(a[5]) == _bits(b[5]), (a, b)
    assert odom_run["loops"] == ref_run.loops >= 1
    assert list(odom_run["kf_ids"]) == list(range(len(ref_run.kf_poses)))
    np.testing.assert_array_equal(_bits(odom_run["kf_poses"]), _bits(np.stack(ref_run.kf_poses)))
    np.testing.assert_array_equal(_bits(odom_run["map"]), _bits(ref_run.map))
    assert len(ref_run.map) > 1000


def test_odometry_edges_and_guesses_equal_the_frame_model(ref_run, odom_run):
    """What lo_odom hands to lo_pgo as the odometry edge of every keyframe (lo_loop_event.odom_edge) is the frame-object
    model's normalised relative pose (Estimator.cpp:385-390), bit for bit, and every frame -- the three after the first
    accepted correction in particular -- starts from the model's guess (lo_odom_frame.guess): the previous frame read
    through get_pose(), i.e. through the corrected keyframe."""
    assert ref_run.loops >= 1                                   # (conditions on the model's run)
    first_kf = next(e[0] for e in ref_run.events if e[6])
    f = [k for k, kf in enumerate(ref_run.keyframe) if kf][first_kf]
    assert f + 3 < len(ref_run.poses)
    assert any(not kf for kf in ref_run.keyframe[f + 1:f + 4])  # a non-keyframe hangs off the corrected keyframe
    assert ref_run.odom_edges[0] is None and len(ref_run.odom_edges) == len(odom_run["edges"]) >= 3
    np.testing.assert_array_equal(_bits(odom_run["edges"][0]), _bits(np.eye(3, 4)))
    for j in range(1, len(ref_run.odom_edges)):
        np.testing.assert_array_equal(_bits(odom_run["edges"][j]), _bits(ref_run.odom_edges[j]), err_msg=f"keyframe {j}")
    assert ref_run.guesses[0] is None
    for k in list(range(f + 1, f + 4)) + list(range(1, len(ref_run.guesses))):
        np.testing.assert_array_equal(_bits(odom_run["guesses"][k]), _bits(ref_run.guesses[k]), err_msg=f"frame {k}")
    # the guess behind frame f + 1 starts from the CORRECTED keyframe pose, which the frame's returned pose is not
    assert not np.array_equal(_bits(odom_run["kf_poses"][first_kf]), _bits(odom_run["poses"][f])) or ref_run.loops > 1


def test_loop_closure_off_is_the_plain_frame_loop(scans, odom_run):
    """Not enabled: no allocation beyond a plain LidarOdometry's, and -- up to the first closed loop, after which the
    corrected run legitimately departs -- the same poses as the run with loop closure on."""
    from lidar_odometry_amd.odometry import LidarOdometry
    L = _lib.lib()
    base = L.lo_debug_live_bytes()
    sub = scans[:6]
    grown = []

    def run_plain():
        o = LidarOdometry(max_points=MAX_POINTS)
        try:
            poses = [o.process(raw)[0].reshape(12).copy() for raw in sub]
            grown.append(L.lo_debug_live_bytes() - base)
            assert o.loop_count == 0 and len(o.keyframe_poses()[0]) == 0
            with pytest.raises(RuntimeError):
                o.last_loop
            return poses
        finally:
            o.close()

    a, b = run_plain(), run_plain()
    assert grown[0] == grown[1] and L.lo_debug_live_bytes() == base
    for x, y, z in zip(a, b, odom_run["poses"]):
        np.testing.assert_array_equal(_bits(x), _bits(y))
        np.testing.assert_array_equal(_bits(x), _bits(z))      # before the first loop: enabling changes no pose
    # enabling is what allocates (detector, keyframe store)
    o = LidarOdometry(max_points=MAX_POINTS)
    try:
        before = L.lo_debug_live_bytes()
        o.enable_loop_closure(_cfg())
        assert L.lo_debug_live_bytes() > before
    finally:
        o.close()
    assert L.lo_debug_live_bytes() == base


def test_first_accepted_loop_is_after_the_frames_compared_above(odom_run):
    first = next(e[0] for e in odom_run["events"] if e[6])
    kf_frames = [k for k, f in enumerate(odom_run["flags"]) if f]
    assert kf_frames[first] >= 6


def test_after_a_closed_loop_tracking_goes_on(odom_run):
    assert odom_run["loops"] >= 1 and odom_run["surfels"] > 0
    first = next(e[0] for e in odom_run["events"] if e[6])
    kf_frames = [k for k, f in enumerate(odom_run["flags"]) if f]
    later = odom_run["status"][kf_frames[first] + 1:]
    assert len(later) > 0 and all(s == _lib.LO_OK for s in later)


def test_kdtree_mode_closes_a_loop_too(scans):
    out = _odom_run(scans, _cfg(), kdtree=True)
    assert out["loops"] >= 1 and len(out["map"]) > 1000
    assert all(s == _lib.LO_OK for s in out["status"])


def test_cooldown(odom_run):
    cfg = _cfg()
    last = -1
    for kid, queried, cand, _, _, _, accepted in odom_run["events"]:
        assert queried == (kid - last >= cfg.cooldown_keyframes), (kid, last)
        if not queried:
            assert cand == -1 and not accepted
        if accepted:
            last = kid
    assert last >= 0


def test_capacity_error_at_the_third_keyframe(scans):
    from lidar_odometry_amd.odometry import LidarOdometry
    o = LidarOdometry(max_points=MAX_POINTS)
    try:
        o.enable_loop_closure(_cfg(max_keyframes=2))
        T = np.zeros(12, np.float32)
        info = _lib.LoOdomFrame()
        fp = C.POINTER(C.c_float)
        rcs = []
        for raw in scans[:8]:
            raw = np.ascontiguousarray(raw, np.float32)
            rc = _lib.lib().lo_odom_process(o._o, raw.ctypes.data_as(fp), len(raw), T.ctypes.data_as(fp), C.byref(info))
            rcs.append(rc)
            if rc < 0:
                break
        assert rcs[-1] == _lib.LO_ERR_CAPACITY and all(r >= 0 for r in rcs[:-1])
        assert o.keyframes == 3
        assert b"capacity" in _lib.lib().lo_odom_last_error(o._o)
    finally:
        o.close()


def test_lifecycle(scans):
    from lidar_odometry_amd.odometry import LidarOdometry
    L = _lib.lib()
    base = L.lo_debug_live_bytes()
    o = LidarOdometry(max_points=MAX_POINTS)
    try:
        o.process(scans[0])
        c = _cfg().to_c()
        assert L.lo_odom_enable_loop_closure(o._o, C.byref(c)) == _lib.LO_ERR_STATE
    finally:
        o.close()
    o = LidarOdometry(max_points=MAX_POINTS)
    try:
        c = _cfg().to_c()
        assert L.lo_odom_enable_loop_closure(o._o, C.byref(c)) == _lib.LO_OK
        assert L.lo_odom_enable_loop_closure(o._o, C.byref(c)) == _lib.LO_ERR_STATE      # once
        bad = _cfg(min_keyframe_gap=0).to_c()
        assert L.lo_odom_enable_loop_closure(o._o, C.byref(bad)) == _lib.LO_ERR_ARG
        for raw in scans[:3]:
            o.process(raw)
    finally:
        o.close()
    assert L.lo_debug_live_bytes() == base


def test_ply_export(scans, tmp_path):
    def after(o, out):
        path = tmp_path / "map.ply"
        o.save_map_ply(path, MAP_VOXEL)
        back = np.zeros((len(out["map"]) + 8, 3), np.float32)
        n = _lib.lib().lo_load_ply(str(path).encode(), back.ctypes.data_as(C.POINTER(C.c_float)), len(back))
        assert n == len(out["map"])
        np.testing.assert_array_equal(_bits(back[:n]), _bits(out["map"]))
    out = _odom_run(scans[:9], _cfg(), after=after)
    assert len(out["map"]) > 100
