"""Numpy fp32 restatement of the map export's definitions (include/lo_gmap.h), the reference of test_gmap_host.py and
test_gpu_gmap.py.  Nothing here calls the library: a Python dict keyed by (kx, ky, kz), np.float32 scalar operations
in the stated order (each one separately rounded), sorted keys."""
import numpy as np

F = np.float32


def transform(T, pts):
    """Matrix4f * (x, y, z, 1) in transform_points' order: a = T0 x; a = T1 y + a; a = T2 z + a; a = T3 1 + a."""
    T = np.asarray(T, np.float32).reshape(-1)[:12]
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.empty_like(p)
    for r in range(3):
        a = T[4 * r] * x
        a = T[4 * r + 1] * y + a
        a = T[4 * r + 2] * z + a
        a = T[4 * r + 3] * F(1.0) + a
        out[:, r] = a
    return out


def world_cloud(clouds, poses):
    """The transformed concatenation in input order (empty keyframes contribute nothing)."""
    parts = [transform(T, c) for c, T in zip(clouds, poses) if len(c)]
    return np.concatenate(parts) if parts else np.zeros((0, 3), np.float32)


def keys(pts, leaf):
    """(int)floorf(p / leaf) per axis, the division in fp32."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    return np.floor(p / F(leaf)).astype(np.int64)


def voxel_grid(pts, leaf):
    """VoxelGrid::filter -> ((M, 3) float32 centroids in sorted key order, the sorted keys)."""
    p = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    if len(p) == 0 or not leaf > 0:
        return np.zeros((0, 3), np.float32), []
    k = keys(p, leaf)
    vox = {}
    one = F(1.0)
    for i in range(len(p)):
        key = (int(k[i, 0]), int(k[i, 1]), int(k[i, 2]))
        px, py, pz = p[i, 0], p[i, 1], p[i, 2]
        c = vox.get(key)
        if c is None:
            vox[key] = [px, py, pz, one]
            continue
        w = c[3]
        tw = F(w + one)
        a = F(w / tw)
        b = F(one / tw)
        c[0] = F(F(a * c[0]) + F(b * px))
        c[1] = F(F(a * c[1]) + F(b * py))
        c[2] = F(F(a * c[2]) + F(b * pz))
        c[3] = tw
    order = sorted(vox)
    out = np.array([vox[key][:3] for key in order], np.float32).reshape(-1, 3)
    return out, order


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_bits_equal(got, want):
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    np.testing.assert_array_equal(bits(got), bits(want))
