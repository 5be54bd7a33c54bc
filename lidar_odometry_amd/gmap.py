"""Host-side mirror of the reference's map export over the HIP C ABI (``include/lo_gmap.h``).

``GlobalMapBuilder`` keeps the meaning of ``Estimator::save_map_to_ply`` (src/processing/Estimator.cpp:1248-1305):
the keyframes' feature clouds are stored as they are added, ``build`` transforms each by its keyframe's pose,
concatenates them and downsamples with ``util::VoxelGrid`` (src/util/PointCloudUtils.h:462-557), ``save_ply`` writes
``util::save_point_cloud_ply``'s file.  The clouds stay on the GPU, so after a loop closure the map is rebuilt at
the optimised poses (``lo_pgo``) by one more ``build``.  Transform, sort and centroids run on the GPU through
``liblo_icp.so`` and reproduce the reference's fp32 results bit for bit; there is no CPU fallback.  The one stated
limit -- voxel keys within +-2^20 per axis, finite points -- is described in ``include/lo_gmap.h``.

Point clouds are (N, 3) float32: numpy arrays (host), or device tensors exposing ``data_ptr()`` and ``is_cuda``
(torch tensors on the builder's device), which are read in place.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import LO_GMAP_STAGES, LO_INSUFFICIENT, lib
from .iris import _cloud, _fptr


def voxelgrid_host(points, voxel_size: float) -> np.ndarray:
    """lo_gmap_voxelgrid_host: util::VoxelGrid::filter on one core (no GPU) -> (M, 3) float32 in key order."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((max(len(p), 1), 3), np.float32)
    k = int(lib().lo_gmap_voxelgrid_host(_fptr(p), len(p), float(voxel_size), _fptr(out), len(p)))
    if k < 0:
        raise ValueError(f"lo_gmap_voxelgrid_host error {k}: a point is non-finite or its voxel key is out of range")
    return out[:k]


def save_ply(path, points) -> None:
    """lo_save_ply: util::save_point_cloud_ply's binary little-endian x/y/z file; an empty cloud is refused."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    rc = int(lib().lo_save_ply(str(path).encode(), _fptr(p), len(p)))
    if rc != 0:
        raise (ValueError if rc == -1 else OSError)(f"lo_save_ply({path!r}, {len(p)} points) failed (code {rc})")


def _poses(poses) -> np.ndarray:
    """(K, 3, 4), (K, 4, 4) or (K, 12) -> contiguous (K, 12) float32, row-major 3x4."""
    a = np.asarray(poses, dtype=np.float32)
    if a.size == 0:
        return np.zeros((0, 12), np.float32)
    if a.ndim == 3 and a.shape[1:] in ((3, 4), (4, 4)):
        a = a[:, :3, :]
    elif not (a.ndim == 2 and a.shape[1] == 12):
        raise ValueError("poses must be (K, 3, 4), (K, 4, 4) or (K, 12)")
    return np.ascontiguousarray(a.reshape(len(a), 12))


class GlobalMapBuilder:
    """GPU global-map builder bound to an ICP context (its device and stream)."""

    def __init__(self, optimizer, max_points: int = 1 << 22, max_keyframes: int = 4096):
        """optimizer: an ``IterativeClosestPointOptimizer`` (or a raw ``lo_ctx`` handle); max_points: stored points
        over all keyframes; max_keyframes: keyframes.  All device memory is taken here."""
        self._L = lib()
        self._owner = optimizer                      # the context must outlive the builder
        ctx = getattr(optimizer, "ctx", optimizer)
        err = C.c_int(0)
        self._h = self._L.lo_gmap_create(ctx, int(max_points), int(max_keyframes), C.byref(err))
        if not self._h:
            raise RuntimeError(f"lo_gmap_create failed (code {err.value})")

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._L.lo_gmap_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError(f"liblo_icp error {rc}: {self._L.lo_gmap_last_error(self._h).decode()}")
        return rc

    def __len__(self) -> int:
        """Keyframes added."""
        return int(self._L.lo_gmap_keyframes(self._h))

    @property
    def points(self) -> int:
        """Stored points over all keyframes."""
        return int(self._L.lo_gmap_points(self._h))

    def clear(self):
        self._check(self._L.lo_gmap_clear(self._h))

    def add_keyframe(self, keyframe_id: int, points) -> None:
        """Append a keyframe's feature cloud (sensor frame); an empty cloud keeps the keyframe without points."""
        keep, ptr, n, dev = _cloud(points)
        self._check(self._L.lo_gmap_add_keyframe(self._h, int(keyframe_id), ptr, n, dev))
        del keep

    def add_from_scan(self, keyframe_id: int) -> None:
        """The context's last device-filtered scan (optimize_raw / voxel_filter) as the keyframe's cloud."""
        self._check(self._L.lo_gmap_add_from_scan(self._h, int(keyframe_id)))

    def keyframe_points(self, index: int):
        """(keyframe id, device pointer as int, count) of keyframe ``index`` (insertion order) inside the arena; no
        copy, valid until clear / close.  IndexError past the end."""
        kid, p, n = C.c_int64(0), C.c_void_p(0), C.c_size_t(0)
        if not 0 <= int(index) < len(self):
            raise IndexError(f"keyframe index {index} out of range ({len(self)} keyframes)")
        self._check(self._L.lo_gmap_keyframe_points(self._h, int(index), C.byref(kid), C.byref(p), C.byref(n)))
        return int(kid.value), int(p.value or 0), int(n.value)

    def build(self, poses, voxel_size: float) -> np.ndarray:
        """The map at these keyframe poses (one per keyframe, insertion order) -> (M, 3) float32; voxel_size <= 0:
        the transformed concatenation.  An empty builder gives a (0, 3) array (the reference's ``false``)."""
        P = _poses(poses)
        n = C.c_size_t(0)
        rc = self._check(self._L.lo_gmap_build(self._h, _fptr(P), len(P), float(voxel_size), C.byref(n)))
        if rc == LO_INSUFFICIENT:
            return np.zeros((0, 3), np.float32)
        out = np.zeros((max(n.value, 1), 3), np.float32)
        k = self._check(self._L.lo_gmap_download(self._h, _fptr(out), n.value))
        return out[:k]

    def device_points(self):
        """(device pointer as int, count) of the last build's result, valid until the next build / clear."""
        p, n = C.c_void_p(0), C.c_size_t(0)
        self._check(self._L.lo_gmap_device_points(self._h, C.byref(p), C.byref(n)))
        return int(p.value or 0), int(n.value)

    def save_ply(self, path) -> None:
        """Write the last build's result as util::save_point_cloud_ply does."""
        self._check(self._L.lo_gmap_save_ply(self._h, str(path).encode()))

    def bench_build(self, poses, voxel_size: float, reps: int = 20):
        """(average device ms of one build, per-stage ms: transform + key, sort, heads + gather + scan, centroids)."""
        P = _poses(poses)
        ms = C.c_float(0.0)
        self._check(self._L.lo_gmap_bench_build(self._h, _fptr(P), len(P), float(voxel_size), int(reps), C.byref(ms)))
        st = np.zeros(LO_GMAP_STAGES, np.float32)
        self._check(self._L.lo_gmap_stage_ms(self._h, _fptr(st)))
        return float(ms.value), [float(v) for v in st]
