"""CPU tests of the global-map builder's boundary (include/lo_gmap.h, lo_save_ply in include/lo_io.h): the library
exports the entry points, the package exports the Python class, the one-core voxel grid (lo_gmap_voxelgrid_host)
equals the numpy restatement of VoxelGrid::filter (tests/_gmap_ref.py) bit for bit, and lo_save_ply writes
save_point_cloud_ply's bytes.  No GPU call happens here."""
import ctypes as C
import os

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests import _gmap_ref as ref

GMAP_SYMBOLS = ("lo_gmap_create", "lo_gmap_destroy", "lo_gmap_clear", "lo_gmap_keyframes", "lo_gmap_points",
                "lo_gmap_last_error", "lo_gmap_add_keyframe", "lo_gmap_add_from_scan", "lo_gmap_build",
                "lo_gmap_download", "lo_gmap_device_points", "lo_gmap_save_ply", "lo_gmap_bench_build",
                "lo_gmap_voxelgrid_host", "lo_save_ply")
HEADER = (b"ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
          b"property float z\nend_header\n")


def _host(points, leaf):
    from lidar_odometry_amd.gmap import voxelgrid_host
    return voxelgrid_host(points, leaf)


def _both(points, leaf):
    want, order = ref.voxel_grid(points, leaf)
    got = _host(points, leaf)
    ref.assert_bits_equal(got, want)
    return got, order


def _one_voxel(seed, n=300):
    """n points inside voxel (3, -2, 0) of leaf 0.5."""
    rng = np.random.default_rng(seed)
    return (np.array([1.5, -1.0, 0.0]) + rng.uniform(0.01, 0.49, (n, 3))).astype(np.float32)


def test_symbols_and_class_are_exported():
    import lidar_odometry_amd
    L = C.CDLL(_lib.LIB_PATH)
    for name in GMAP_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(L, name), name
    assert "GlobalMapBuilder" in lidar_odometry_amd.__all__
    assert callable(lidar_odometry_amd.GlobalMapBuilder)


@pytest.mark.parametrize("leaf", [0.5, 0.2, 0.4])
def test_voxelgrid_host_random_cloud(leaf):
    rng = np.random.default_rng(5)
    pts = rng.uniform(-20.0, 20.0, (3000, 3)).astype(np.float32)
    pts[:, 2] *= 0.1                                       # a flat slab: many voxels hold several points
    got, order = _both(pts, leaf)
    assert 500 < len(got) < len(pts)
    assert order == sorted(order) and min(k[0] for k in order) < 0 < max(k[0] for k in order)


def test_voxelgrid_host_negative_coordinates():
    rng = np.random.default_rng(6)
    pts = -rng.uniform(0.0, 8.0, (800, 3)).astype(np.float32)
    got, order = _both(pts, 0.5)
    assert all(k[0] < 0 and k[1] < 0 and k[2] < 0 for k in order)


def test_voxelgrid_host_points_on_the_voxel_faces_and_negative_zero():
    k = np.arange(-6, 7)
    g = np.stack(np.meshgrid(k, k, k[:3], indexing="ij"), -1).reshape(-1, 3)
    for leaf in (0.5, 0.2, 0.4):
        pts = (g.astype(np.float32) * np.float32(leaf)).astype(np.float32)     # exactly k * leaf in fp32
        pts = np.concatenate([pts, np.array([[-0.0, -0.0, -0.0], [-0.0, 0.3 * leaf, 0.0]], np.float32)])
        got, order = _both(pts, leaf)
        assert (0, 0, 0) in order
    # -0.0 alone is copied as it is: voxel (0, 0, 0), sign bit kept
    got, order = _both(np.array([[-0.0, -0.0, -0.0]], np.float32), 0.5)
    assert order == [(0, 0, 0)] and (ref.bits(got) == 0x80000000).all()


def test_voxelgrid_host_long_run_and_its_order_dependence():
    pts = _one_voxel(0)
    got, order = _both(pts, 0.5)
    assert order == [(3, -2, 0)] and len(got) == 1
    # the running average depends on the order of its inputs: the same points reversed give other bits, so an
    # implementation that visits a voxel's points in another order cannot pass the comparisons above
    rev, _ = ref.voxel_grid(pts[::-1], 0.5)
    assert (ref.bits(rev) != ref.bits(got)).any()
    ref.assert_bits_equal(_host(pts[::-1], 0.5), rev)


def test_voxelgrid_host_empty_and_unfiltered():
    assert len(_host(np.zeros((0, 3), np.float32), 0.5)) == 0
    assert len(_host(np.ones((4, 3), np.float32), 0.0)) == 0            # filter() clears its output for leaf <= 0
    L = _lib.lib()
    p = np.ones((4, 3), np.float32)
    fp = C.POINTER(C.c_float)
    assert L.lo_gmap_voxelgrid_host(p.ctypes.data_as(fp), 4, 0.5, None, 0) == 1          # NULL sizes


def test_voxelgrid_host_refuses_points_outside_the_key_range():
    L = _lib.lib()
    fp = C.POINTER(C.c_float)
    out = np.zeros((2, 3), np.float32)
    for bad in (3e6, np.nan, np.inf):
        p = np.array([[1.0, 2.0, 3.0], [0.0, bad, 0.0]], np.float32)
        assert L.lo_gmap_voxelgrid_host(p.ctypes.data_as(fp), 2, 0.5, out.ctypes.data_as(fp), 2) == _lib.LO_ERR_ARG
    edge = np.array([[-524288.0, 524287.75, 0.0]], np.float32)         # keys -2^20 and 2^20 - 1: the last ones inside
    assert L.lo_gmap_voxelgrid_host(edge.ctypes.data_as(fp), 1, 0.5, out.ctypes.data_as(fp), 2) == 1


# ---------------------------------------------------------------------------------------------------- lo_save_ply
def _load_ply(path):
    L = _lib.lib()
    n = L.lo_load_ply(str(path).encode(), None, 0)
    out = np.zeros((max(n, 1), 3), np.float32)
    k = L.lo_load_ply(str(path).encode(), out.ctypes.data_as(C.POINTER(C.c_float)), n)
    return out[:k]


def test_save_ply_bytes_and_round_trip(tmp_path):
    from lidar_odometry_amd.gmap import save_ply
    rng = np.random.default_rng(9)
    pts = rng.uniform(-50.0, 50.0, (257, 3)).astype(np.float32)
    pts[0] = (-0.0, np.float32(1e-30), np.float32(3.4e38))
    path = tmp_path / "map.ply"
    save_ply(path, pts)
    blob = path.read_bytes()
    head = HEADER % len(pts)
    assert blob[:len(head)] == head
    assert len(blob) == len(head) + 12 * len(pts)
    assert blob[len(head):] == pts.tobytes()
    ref.assert_bits_equal(_load_ply(path), pts)


def test_save_ply_creates_missing_parent_directories(tmp_path):
    from lidar_odometry_amd.gmap import save_ply
    path = tmp_path / "a" / "b" / "map.ply"
    save_ply(path, np.ones((3, 3), np.float32))
    assert path.stat().st_size == len(HEADER % 3) + 36


def test_save_ply_refuses_an_empty_cloud(tmp_path):
    from lidar_odometry_amd.gmap import save_ply
    path = tmp_path / "sub" / "empty.ply"
    p = np.zeros((1, 3), np.float32)
    rc = _lib.lib().lo_save_ply(str(path).encode(), p.ctypes.data_as(C.POINTER(C.c_float)), 0)
    assert rc == -1                                                     # LO_IO_ERR_ARG
    with pytest.raises(ValueError):
        save_ply(path, np.zeros((0, 3), np.float32))
    assert not os.path.exists(path) and not os.path.exists(path.parent)
