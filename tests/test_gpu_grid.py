"""The device grid builder (csrc/lo_grid.hip: grid_from_device and the k_grid_* kernels) against the host builder
(grid_build) on the same points.

The batched and the single-context device forms are two shells of one set of kernel bodies, so comparing them with each
other (tests/test_gpu_batch_kdtree_loop.py) no longer compares independent programs; the host builder is the independent
one.  a. a context's grid built from a device map's L0 centroids (lo_devmap_sync_points) against lo_map_set_points on
the same centroids in the same order.  b. the loop-closure ICP's local map with the occupancy rule
(lo_icp_optimize_loop_dev against lo_icp_optimize_loop), read through lo_debug_loop_grid.  Every word as uint32, no
tolerance.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests.test_gpu_batch_kdtree import _kd
from tests.test_gpu_batch_kdtree_loop import grid, same_grid, sorted_by_cell
from tests.test_gpu_loop_dev import _assert_equal, _call

pytestmark = pytest.mark.gpu

VOXEL = 0.5
K_MAX_CELLS = 1 << 26
K_KNN_ALL_MAX = 8192
K_LOOP_MIN_PER_CELL = 4


def _centres(idx):
    """Voxel centres of integer voxel indices: a map's centroid of one such point is the point."""
    return np.ascontiguousarray(np.asarray(idx, np.float64) * VOXEL + VOXEL / 2, dtype=np.float32)


def _distinct(rng, dims, n):
    """n distinct voxels of a dims[0] x dims[1] x dims[2] block, in random order."""
    flat = rng.choice(int(np.prod(dims)), n, replace=False)
    return np.stack(np.unravel_index(flat, dims), 1)


def _clouds():
    rng = np.random.default_rng(21)
    out = {"empty": np.zeros((0, 3), np.float32), "one": _centres([[3, -4, 1]]),
           "three": _centres([[0, 0, 0], [6, -4, 1], [-5, 1, 10]]),
           # more than one 1024-thread pass and more than one 256-thread block, no multiple of either
           "dense": _centres(_distinct(rng, (80, 80, 10), 3001))}
    # ncell + 1 beyond one scan chunk (2048 words); 13^3 + 1 = 2198 leaves a tail of 2 words for the clear,
    # 15 * 15 * 11 + 1 = 2476 is a multiple of 4
    for name, cells in (("chunks_tail", (13, 13, 13)), ("chunks_mult4", (15, 15, 11))):
        vox = _distinct(rng, tuple(2 * c for c in cells), 600)
        vox[0], vox[1] = (0, 0, 0), tuple(2 * c - 1 for c in cells)
        vox = np.unique(vox, axis=0)
        out[name] = _centres(vox[rng.permutation(len(vox))])
    # 300 voxels over a 500 m cube (500^3 cells of 1 m exceed 2^26: the edge doubles to 2 m), and 4 x 4 x 3 adjacent
    # voxels inside one 2 m cell, in descending order in the middle of the cloud
    far = rng.integers(-500, 500, size=(300, 3))
    far[0], far[1] = (-500, -500, -500), (499, 499, 499)
    blk = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3) + 200
    far = far[~np.all((far >= 200) & (far < 204), axis=1)]
    out["wide"] = _centres(np.concatenate([far[:150], blk[::-1], far[150:]]))
    # the 8 voxels of one 1 m cell at indices spread over the whole cloud
    vox = _distinct(rng, (60, 60, 8), 4000)
    vox = vox[~np.all(vox // 2 == (7, 9, 1), axis=1)]
    mates = np.stack(np.meshgrid([14, 15], [18, 19], [2, 3], indexing="ij"), -1).reshape(-1, 3)
    where = np.linspace(0, len(vox) - 1, 8).astype(int)
    vox = np.insert(vox, where, mates, axis=0)
    out["far_apart_mates"] = _centres(vox)
    return out


CLOUDS = _clouds()


@pytest.fixture(scope="module")
def host():
    o = _kd(1 << 14)
    yield o
    o.close()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_device_built_grid_equals_the_host_built_grid(host, name):
    from lidar_odometry_amd.voxelmap import DeviceVoxelMap
    cloud = CLOUDS[name]
    dev = _kd(1 << 14)
    dm = DeviceVoxelMap(dev, VOXEL, 3, 0.1, max_l0=1 << 14, max_points=1 << 14)
    try:
        if len(cloud):
            dm.update(cloud, np.zeros(3), 1e4, True)
        l0 = np.ascontiguousarray(dm.l0()[1])               # the map's L0 centroids in its own order
        assert len(l0) == len(cloud)
        np.testing.assert_array_equal(np.sort(l0.view(np.uint32), axis=0), np.sort(cloud.view(np.uint32), axis=0))
        dm.sync_points()
        first = grid(dev)
        dm.sync_points()                                    # again on the same context: the same grid
        second = grid(dev)
        host.set_map_points(l0)
        want = grid(host)
        same_grid(first, want, name)
        same_grid(second, want, name + " (second build)")
        sorted_by_cell(first)
        g = first
        ncell = g["dim"][0] * g["dim"][1] * g["dim"][2]
        one, two = (np.float32(x).view(np.uint32) for x in (1.0, 2.0))
        assert g["m"] == len(cloud) and ncell <= K_MAX_CELLS
        assert g["h"] == (two if name == "wide" else one)
        per_cell = np.diff(g["start"].astype(np.int64))
        if name == "empty":
            assert g["dim"] == (1, 1, 1) and g["start"].tolist() == [0, 0]
        if name == "dense":
            assert g["m"] > 1024 and g["m"] % 256 != 0
        if name == "chunks_tail":
            assert g["dim"] == (13, 13, 13) and ncell + 1 > 2048 and (ncell + 1) % 4 == 2
        if name == "chunks_mult4":
            assert g["dim"] == (15, 15, 11) and ncell + 1 > 2048 and (ncell + 1) % 4 == 0
        if name == "wide":
            assert 500 ** 3 > K_MAX_CELLS and g["dim"] == (250, 250, 250)
            assert per_cell.max() >= 48                     # place's rank loop over many entries
        if name == "far_apart_mates":
            cell = (7 - g["org"][0]) + g["dim"][0] * ((9 - g["org"][1]) + g["dim"][1] * (1 - g["org"][2]))
            idx = g["pts"][g["start"][cell]:g["start"][cell + 1], 3].astype(np.int64)
            # its 8 points come from 8 different workgroups: the atomics' arrival order is not the index order
            assert len(idx) == 8 and idx[-1] - idx[0] > 3000 and np.all(np.diff(idx) > 256)
    finally:
        dm.close()
        dev.close()


# ---------------------------------------------------------------- b. the loop grid and the occupancy rule
def _loop_grid(icp):
    """lo_debug_loop_grid: the matched cloud's local map as the last loop call left it."""
    L = _lib.lib()
    h, m = C.c_float(0), C.c_int(0)
    org, dim = (C.c_int * 3)(), (C.c_int * 3)()
    assert L.lo_debug_loop_grid(icp.ctx, C.byref(h), org, dim, C.byref(m), None, 0, None, 0) == _lib.LO_OK
    start = np.zeros(dim[0] * dim[1] * dim[2] + 1, np.uint32)
    pts = np.zeros((max(m.value, 1), 4), np.float32)
    assert L.lo_debug_loop_grid(icp.ctx, C.byref(h), org, dim, C.byref(m), start.ctypes.data_as(C.POINTER(C.c_uint32)),
                                len(start), pts.ctypes.data_as(C.POINTER(C.c_float)), len(pts)) == _lib.LO_OK
    return dict(h=np.float32(h.value).view(np.uint32), org=tuple(org), dim=tuple(dim), m=m.value, start=start,
                pts=pts[:m.value].view(np.uint32))


def _occupied(p, h):
    """Occupied cells of edge h: float32 division and floor, as the builders."""
    return len(np.unique(np.floor(p / np.float32(h)).astype(np.int64), axis=0))


@pytest.fixture(scope="module")
def icp():
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    o = IterativeClosestPointOptimizer(max_points=1 << 14)
    yield o
    o.close()


# box (m), the doublings the rule asks for; the last is still asking after three and is cut off there
@pytest.mark.parametrize("box,widens", [((40.0, 40.0, 2.0), 1), ((80.0, 80.0, 4.0), 2), ((400.0, 400.0, 40.0), 3)])
def test_loop_grid_with_the_occupancy_rule_equals_the_host_entry(icp, box, widens):
    L = _lib.lib()
    rng = np.random.default_rng(int(box[0]))
    m = K_KNN_ALL_MAX + 808                                 # just over kKnnAllMax: the grid path
    mat = np.ascontiguousarray(rng.uniform(0.0, box, size=(m, 3)), dtype=np.float32)
    cur = np.ascontiguousarray(mat[:300] + np.array([0.03, -0.02, 0.01], np.float32), dtype=np.float32)
    I = np.eye(3, 4, dtype=np.float32).reshape(12)
    # the reference alone says what the rule does here: the edge starts at 2 x voxel = 1 m, fits 2^26 cells as it is,
    # and doubles while occupied * min_per_cell > m, three times at most
    assert np.prod(np.ceil(np.asarray(box))) <= K_MAX_CELLS
    asks = [_occupied(mat, 2.0 ** k) * K_LOOP_MIN_PER_CELL > m for k in range(4)]
    assert asks[:widens] == [True] * widens
    assert asks[widens] == (widens == 3)
    want_h = np.float32(2.0 ** widens).view(np.uint32)

    before = L.lo_loop_reruns(icp.ctx)
    h = _call(icp, False, cur, I, mat, I)
    gh = _loop_grid(icp)
    d = _call(icp, True, cur, I, mat, I)
    gd = _loop_grid(icp)
    assert L.lo_loop_reruns(icp.ctx) == before              # no tie rebuilt either grid on the host
    assert gh["h"] == want_h and gd["h"] == want_h
    assert gh["m"] == m
    same_grid(gd, gh, f"loop grid, box {box}")
    sorted_by_cell(gd)
    _assert_equal(d, h)
