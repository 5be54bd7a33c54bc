"""The frame loop for B sequences (lo_odom_batch_*, BatchLidarOdometry): every sequence's poses, keyframe flags,
iteration counts, filtered counts and guesses equal, bit for bit, a LidarOdometry fed that sequence alone with the same
mode -- in reference-exact and in fast mode -- and the loop's edges: an empty first scan, a KDTree config, an
overflowing map."""
import functools

import numpy as np
import pytest

from lidar_odometry_amd import synth

pytestmark = pytest.mark.gpu

N_FRAMES = 12
MAXP = 1 << 15
MAX_L0 = 1 << 18
SEEDS = (7, 9, 11)


@functools.lru_cache(maxsize=None)
def sequences():
    """Three sequences (raw scans, initial pose); the third starts from a non-identity pose.  Built once."""
    out = []
    for s in SEEDS:
        # from rest to ~0.6 m per frame within five frames: a keyframe (1 m) every other frame or so afterwards
        seq = synth.KittiLikeSequence(seed=s, n_frames=N_FRAMES, ramp_s=0.5)
        raws = [seq.scan(k, device="cuda") for k in range(N_FRAMES)]     # (raycast on the GPU: seconds saved)
        for r in raws:
            r.setflags(write=False)
        out.append((raws, seq.poses[0]))
    raws, _ = out[2]
    out[2] = (raws, synth.se3(synth.rot_z(0.3), [5.0, -2.0, 0.5]))
    return tuple(out)


def solo(raws, T0, exact):
    import os
    from lidar_odometry_amd.odometry import LidarOdometry
    os.environ["LO_DEVMAP_MAX_L0"] = str(MAX_L0)          # the solo loop's map capacity (read by lo_odom_create)
    try:
        od = LidarOdometry(max_points=MAXP, initial_pose=T0, exact=exact)
    finally:
        del os.environ["LO_DEVMAP_MAX_L0"]
    try:
        return [od.process(r) for r in raws]
    finally:
        od.close()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
def test_every_sequence_equals_its_solo_frame_loop(exact):
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    seqs = sequences()
    bo = BatchLidarOdometry(len(seqs), max_points=MAXP, initial_poses=[T0 for _, T0 in seqs], exact=exact,
                            max_l0=MAX_L0)
    try:
        got = [bo.process([raws[k] for raws, _ in seqs]) for k in range(N_FRAMES)]
        bo.flush()
        kfs = [bo.keyframes(j) for j in range(len(seqs))]
    finally:
        bo.close()
    for j, (raws, T0) in enumerate(seqs):
        ref = solo(raws, T0, exact)
        flags = [i.keyframe for _, i in ref]
        assert sum(flags) >= 3 and not all(flags[1:]), flags            # several keyframes, some frames without
        assert kfs[j] == sum(flags)
        for k, (T, info) in enumerate(ref):
            Tb, ib = got[k][0][j], got[k][1][j]
            msg = f"sequence {j} frame {k}"
            np.testing.assert_array_equal(bits(Tb), bits(T), err_msg=msg)
            np.testing.assert_array_equal(bits(ib.guess), bits(info.guess), err_msg=msg)
            assert (ib.keyframe, ib.icp_iterations, ib.n_filtered, ib.status) == \
                   (info.keyframe, info.icp_iterations, info.n_filtered, info.status), msg


def test_empty_first_scan_takes_the_early_return_while_the_others_track():
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    (raws_a, Ta), (raws_b, Tb), _ = sequences()
    empty = np.full((16, 3), np.nan, np.float32)
    n = 5
    feed = [[raws_a[k], empty if k == 0 else raws_b[k]] for k in range(n)]
    bo = BatchLidarOdometry(2, max_points=MAXP, initial_poses=[Ta, Tb], max_l0=MAX_L0)
    try:
        got = [bo.process(f) for f in feed]
        assert bo.keyframes(1) == 0 and bo.keyframes(0) >= 1
    finally:
        bo.close()
    for j, T0 in ((0, Ta), (1, Tb)):
        ref = solo([f[j] for f in feed], T0, True)
        for k, (T, info) in enumerate(ref):
            Tg, ig = got[k][0][j], got[k][1][j]
            np.testing.assert_array_equal(bits(Tg), bits(T), err_msg=f"sequence {j} frame {k}")
            np.testing.assert_array_equal(bits(ig.guess), bits(info.guess), err_msg=f"sequence {j} frame {k}")
            assert (ig.keyframe, ig.icp_iterations, ig.n_filtered, ig.status) == \
                   (info.keyframe, info.icp_iterations, info.n_filtered, info.status)
    assert all(not got[k][1][1].keyframe and got[k][1][1].icp_iterations == 0 for k in range(n))


def test_kdtree_config_is_refused():
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    with pytest.raises(ValueError, match="surfel mode only.*-1"):
        BatchLidarOdometry(2, max_points=MAXP, use_surfel_correspondence=False)


def test_flush_reports_an_overflowing_map():
    """max_l0 = 64: the first keyframes overflow every map; flush() reads the error bits at once, and so does the
    call after the keyframe."""
    from lidar_odometry_amd.odometry import BatchLidarOdometry
    (raws_a, Ta), (raws_b, Tb), _ = sequences()
    bo = BatchLidarOdometry(2, max_points=MAXP, initial_poses=[Ta, Tb], max_l0=64)
    try:
        bo.process([raws_a[0], raws_b[0]])
        with pytest.raises(RuntimeError, match="-3"):
            bo.flush()
    finally:
        bo.close()
    bo = BatchLidarOdometry(2, max_points=MAXP, initial_poses=[Ta, Tb], max_l0=64)
    try:
        bo.process([raws_a[0], raws_b[0]])
        with pytest.raises(RuntimeError, match="-3"):
            bo.process([raws_a[1], raws_b[1]])
    finally:
        bo.close()
