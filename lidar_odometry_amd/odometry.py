"""Frame loop around the ICP step (Estimator::process_frame; loop closure / PGO opt-in through
``enable_loop_closure``), C++ in liblo_icp.so (lo_odometry.cpp, include/lo_odometry.h): device voxel filter + device
GN ICP per frame, SE3f bookkeeping, keyframe map updates."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._lib import LO_INSUFFICIENT, LoLoopConfig, LoLoopEvent, LoOdomConfig, LoOdomFrame, lib


@dataclass
class FrameInfo:
    status: int
    keyframe: bool
    icp_iterations: int
    n_filtered: int
    n_corr: int
    device_ms: float
    map_ms: float
    _guess: object = None                        # lo_odom_frame.guess as it came back (converted on demand)

    @property
    def guess(self) -> np.ndarray:
        """(12,) float32: the guess this frame started from (debug output of lo_odom_process)."""
        return np.array(self._guess[:], np.float32)


@dataclass
class LoopConfig:
    """lo_loop_config (defaults: the reference's ConfigUtils.h:117-134)."""
    similarity_threshold: float = 0.3
    min_keyframe_gap: int = 50
    max_search_distance: float = 10.0
    cooldown_keyframes: int = 50
    min_inlier_ratio: float = 0.3
    odom_trans_noise: float = 0.5
    odom_rot_noise: float = 0.5
    loop_trans_noise: float = 1.0
    loop_rot_noise: float = 1.0
    max_keyframes: int = 4096
    max_points: int = 1 << 22

    def to_c(self) -> LoLoopConfig:
        c = LoLoopConfig()
        lib().lo_loop_config_default(C.byref(c))
        c.iris.similarity_threshold = float(self.similarity_threshold)
        c.iris.min_keyframe_gap = int(self.min_keyframe_gap)
        c.iris.max_search_distance = float(self.max_search_distance)
        c.cooldown_keyframes = int(self.cooldown_keyframes)
        c.min_inlier_ratio = float(self.min_inlier_ratio)
        c.odom_trans_noise, c.odom_rot_noise = float(self.odom_trans_noise), float(self.odom_rot_noise)
        c.loop_trans_noise, c.loop_rot_noise = float(self.loop_trans_noise), float(self.loop_rot_noise)
        c.max_keyframes, c.max_points = int(self.max_keyframes), int(self.max_points)
        return c


@dataclass
class LoopEvent:
    """lo_loop_event: the last keyframe's loop attempt."""
    keyframe_id: int
    queried: bool
    candidate_id: int
    candidate_distance: float
    candidate_bias: int
    icp_status: int
    icp_iterations: int
    inlier_ratio: float
    accepted: bool
    pgo_converged: bool
    pgo_iterations: int
    correction_translation: float
    correction_angle: float
    ms: dict = field(default_factory=dict)       # detect / icp / pgo / map, host wall time
    odom_edge: np.ndarray | None = None          # (12,) float32: the odometry edge handed to the pose graph (debug)


class LidarOdometry:
    """One sensor stream on one GPU: process(raw_points) -> 3x4 world pose (config/kitti.yaml defaults)."""

    def __init__(self, device: int = 0, max_points: int = 1 << 17, use_surfel_correspondence: bool = True,
                 point_stride: int = 8, voxel_size: float = 0.5, map_voxel_size: float = 0.5, max_range: float = 100.0,
                 keyframe_distance: float = 1.0, keyframe_rotation: float = 0.3, initial_pose=None,
                 exact: bool = True):
        cfg = LoOdomConfig()
        lib().lo_odom_config_default_kitti(C.byref(cfg))
        cfg.icp.max_points = int(max_points)
        cfg.icp.use_surfel_correspondence = int(bool(use_surfel_correspondence))
        cfg.icp.voxel_size = float(map_voxel_size)
        cfg.point_stride = int(point_stride)
        cfg.filter_voxel_size = float(voxel_size)
        cfg.max_range = float(max_range)
        cfg.keyframe_distance = float(keyframe_distance)
        cfg.keyframe_rotation = float(keyframe_rotation)
        err = C.c_int(0)
        self._L = lib()
        self._o = self._L.lo_odom_create(C.byref(cfg), int(device), C.byref(err))
        if not self._o:
            raise RuntimeError(f"lo_odom_create failed (code {err.value}); is a HIP device present?")
        if initial_pose is not None:
            T = np.ascontiguousarray(np.asarray(initial_pose, np.float32)[:3, :4].reshape(12))
            lib().lo_odom_set_initial_pose(self._o, T.ctypes.data_as(C.POINTER(C.c_float)))
        # the ICP arithmetic mode: reference-exact (the library default, lo_set_exact) or the opt-in fast mode
        lib().lo_odom_set_exact(self._o, 1 if exact else 0)

    def close(self):
        h = getattr(self, "_o", None)
        if h:
            self._o = None
            self._L.lo_odom_destroy(h)

    def __del__(self):
        # at interpreter teardown module globals (lib, os) may already be None: the handle keeps its own
        # reference to the loaded library, and a destructor never raises
        try:
            self.close()
        except Exception:
            pass

    def process(self, raw_points):
        p = np.ascontiguousarray(raw_points, dtype=np.float32).reshape(-1, 3)
        T = np.zeros(12, np.float32)
        info = LoOdomFrame()
        rc = lib().lo_odom_process(self._o, p.ctypes.data_as(C.POINTER(C.c_float)), len(p),
                                   T.ctypes.data_as(C.POINTER(C.c_float)), C.byref(info))
        if rc < 0:
            raise RuntimeError(f"lo_odom_process error {rc}: {lib().lo_odom_last_error(self._o).decode()}")
        return T.reshape(3, 4), FrameInfo(info.status, bool(info.keyframe), info.icp_iterations, info.n_filtered,
                                          info.n_corr, info.device_ms, info.map_ms,
                                          info.guess)

    def _checked(self, rc):
        if rc < 0:
            raise RuntimeError(f"lo_odom error {rc}: {lib().lo_odom_last_error(self._o).decode()}")
        return rc

    def enable_loop_closure(self, config: LoopConfig | None = None) -> None:
        """Close loops inside ``process`` (lo_odom_enable_loop_closure); before the first frame."""
        c = (config or LoopConfig()).to_c()
        self._checked(lib().lo_odom_enable_loop_closure(self._o, C.byref(c)))

    @property
    def last_loop(self) -> LoopEvent:
        e = LoLoopEvent()
        self._checked(lib().lo_odom_last_loop(self._o, C.byref(e)))
        return LoopEvent(e.keyframe_id, bool(e.queried), e.candidate_id, e.candidate_distance, e.candidate_bias,
                         e.icp_status, e.icp_iterations, e.inlier_ratio, bool(e.accepted), bool(e.pgo_converged),
                         e.pgo_iterations, e.correction_translation, e.correction_angle,
                         {"detect": e.detect_ms, "icp": e.icp_ms, "pgo": e.pgo_ms, "map": e.map_ms},
                         np.array(e.odom_edge[:], np.float32))

    @property
    def loop_count(self) -> int:
        return int(lib().lo_odom_loop_count(self._o))

    def keyframe_poses(self):
        """(ids (K,) int32, current -- loop-corrected -- keyframe poses (K, 3, 4) float32)."""
        n = int(lib().lo_odom_keyframe_poses(self._o, None, None, 0))
        ids = np.zeros(max(n, 1), np.int32)
        P = np.zeros((max(n, 1), 12), np.float32)
        lib().lo_odom_keyframe_poses(self._o, ids.ctypes.data_as(C.POINTER(C.c_int)),
                                     P.ctypes.data_as(C.POINTER(C.c_float)), n)
        return ids[:n], P[:n].reshape(n, 3, 4)

    def build_map(self, voxel_size: float) -> np.ndarray:
        """The stored keyframe clouds at the current keyframe poses, voxel-grid filtered (lo_gmap_build) -> (M, 3)."""
        n = C.c_size_t(0)
        rc = self._checked(lib().lo_odom_build_map(self._o, float(voxel_size), C.byref(n)))
        if rc == LO_INSUFFICIENT:
            return np.zeros((0, 3), np.float32)
        out = np.zeros((max(n.value, 1), 3), np.float32)
        k = self._checked(lib().lo_odom_map_points(self._o, out.ctypes.data_as(C.POINTER(C.c_float)), n.value))
        return out[:k]

    def save_map_ply(self, path, voxel_size: float) -> None:
        """Estimator::save_map_to_ply: build_map, then the PLY file."""
        self._checked(lib().lo_odom_save_map_ply(self._o, str(path).encode(), float(voxel_size)))

    def flush(self):
        """Wait for the last keyframe's map update; raise if it overflowed the device map (lo_odom_flush)."""
        rc = lib().lo_odom_flush(self._o)
        if rc < 0:
            raise RuntimeError(f"lo_odom_flush error {rc}: {lib().lo_odom_last_error(self._o).decode()}")

    @property
    def keyframes(self) -> int:
        return int(lib().lo_odom_keyframe_count(self._o))

    @property
    def kd_reruns(self) -> int:
        """Scans run again with the kd visit order after a deciding distance tie (lo_kd_reruns; KDTree mode)."""
        return int(lib().lo_odom_kd_reruns(self._o))

    @property
    def map_surfels(self) -> int:
        return int(lib().lo_odom_map_surfels(self._o))


class BatchLidarOdometry:
    """B sensor streams on one GPU in lockstep (lo_odom_batch_*): ``process(raws)`` takes one raw scan per sequence
    and returns one 3x4 world pose and one FrameInfo per sequence.  Each sequence's poses, keyframes, iteration counts
    and guesses equal a ``LidarOdometry`` fed that sequence alone with the same settings.  The constructor is surfel
    mode only (``use_surfel_correspondence=False`` raises); ``BatchLidarOdometry.kdtree(count, ...)`` is the same loop
    for KDTree-mode sequences (lo_odom_batch_create_kdtree).  No loop closure.  ``max_l0``: every sequence's
    device-map capacity."""

    _create = "lo_odom_batch_create"

    @classmethod
    def kdtree(cls, count: int, **kwargs):
        """The frame loop for ``count`` KDTree-mode sequences (``use_surfel_correspondence = 0``): the same keywords as
        the constructor minus ``use_surfel_correspondence``; every keyframe's grids are rebuilt in one batched call
        (lo_batch_sync_points) after the batched map update."""
        if "use_surfel_correspondence" in kwargs:
            raise TypeError("BatchLidarOdometry.kdtree() takes no use_surfel_correspondence")
        return _KdtreeBatchLidarOdometry(count, use_surfel_correspondence=False, **kwargs)

    def __init__(self, count: int, device: int = 0, max_points: int = 1 << 17, use_surfel_correspondence: bool = True,
                 point_stride: int = 8, voxel_size: float = 0.5, map_voxel_size: float = 0.5, max_range: float = 100.0,
                 keyframe_distance: float = 1.0, keyframe_rotation: float = 0.3, initial_poses=None,
                 exact: bool = True, max_l0: int = 1 << 21):
        cfg = LoOdomConfig()
        lib().lo_odom_config_default_kitti(C.byref(cfg))
        cfg.icp.max_points = int(max_points)
        cfg.icp.use_surfel_correspondence = int(bool(use_surfel_correspondence))
        cfg.icp.voxel_size = float(map_voxel_size)
        cfg.point_stride = int(point_stride)
        cfg.filter_voxel_size = float(voxel_size)
        cfg.max_range = float(max_range)
        cfg.keyframe_distance = float(keyframe_distance)
        cfg.keyframe_rotation = float(keyframe_rotation)
        err = C.c_int(0)
        self._L = lib()
        self.count = int(count)
        self._o = getattr(self._L, self._create)(C.byref(cfg), self.count, int(device), int(max_l0), C.byref(err))
        if not self._o:
            why = self._L.lo_odom_batch_last_error(None).decode()
            if err.value == _lib.LO_ERR_ARG:
                raise ValueError(f"{self._create}: {why} (code {err.value})")
            raise RuntimeError(f"{self._create} failed (code {err.value}): {why}")
        if initial_poses is not None:
            for j, P in enumerate(initial_poses):
                if P is None:
                    continue
                T = np.ascontiguousarray(np.asarray(P, np.float32)[:3, :4].reshape(12))
                self._checked(self._L.lo_odom_batch_set_initial_pose(self._o, j, T.ctypes.data_as(C.POINTER(C.c_float))))
        self._checked(self._L.lo_odom_batch_set_exact(self._o, 1 if exact else 0))

    def close(self):
        h = getattr(self, "_o", None)
        if h:
            self._o = None
            self._L.lo_odom_batch_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _checked(self, rc):
        if rc < 0:
            raise RuntimeError(f"lo_odom_batch error {rc}: {self._L.lo_odom_batch_last_error(self._o).decode()}")
        return rc

    def process(self, raws):
        """One raw scan per sequence -> (poses (B, 3, 4) float32, [FrameInfo] * B)."""
        B = self.count
        pts = [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, 3) for r in raws]
        if len(pts) != B:
            raise ValueError(f"need {B} raw scans")
        ptrs = (C.c_void_p * B)(*[p.ctypes.data if len(p) else None for p in pts])
        ns = (C.c_size_t * B)(*[len(p) for p in pts])
        T = np.zeros((B, 12), np.float32)
        info = (LoOdomFrame * B)()
        self._checked(self._L.lo_odom_batch_process(self._o, ptrs, ns, T.ctypes.data_as(C.POINTER(C.c_float)), info))
        return T.reshape(B, 3, 4), [FrameInfo(f.status, bool(f.keyframe), f.icp_iterations, f.n_filtered, f.n_corr,
                                              f.device_ms, f.map_ms, f.guess) for f in info]

    def flush(self):
        """Wait for the last keyframes' map updates; raise if one overflowed its device map (lo_odom_batch_flush)."""
        self._checked(self._L.lo_odom_batch_flush(self._o))

    def keyframes(self, job: int) -> int:
        return int(self._L.lo_odom_batch_keyframe_count(self._o, int(job)))

    def kd_reruns(self, job: int) -> int:
        """Scans of sequence ``job`` run again with the kd visit order after a deciding distance tie (lo_kd_reruns)."""
        return int(self._L.lo_odom_batch_kd_reruns(self._o, int(job)))


class _KdtreeBatchLidarOdometry(BatchLidarOdometry):
    """What ``BatchLidarOdometry.kdtree`` returns: the same object created through lo_odom_batch_create_kdtree."""
    _create = "lo_odom_batch_create_kdtree"


__all__ = ["LidarOdometry", "BatchLidarOdometry", "FrameInfo", "LoopConfig", "LoopEvent", "_lib"]
