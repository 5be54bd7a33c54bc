"""Host-side mirror of the reference's loop-closure detector over the HIP C ABI (``include/lo_iris.h``).

``IrisLoopDetector`` keeps the meaning of ``LoopClosureDetector`` (src/processing/LoopClosureDetector.cpp:44-202):
``add_keyframe`` stores a keyframe's LiDAR-Iris descriptor with its id and position, ``detect`` compares the current
keyframe's descriptor against the database and returns the best candidate under the gap / distance / threshold rule,
or ``None``.  Image, encode and match run on the GPU through ``liblo_icp.so``; there is no CPU fallback.  The one
departure from the reference -- all 360 column shifts are evaluated instead of +-2 around a Fourier-Mellin
estimate -- is described in ``include/lo_iris.h`` and DESIGN.md.

Point clouds are (N, 3) float32: numpy arrays (host), or device tensors exposing ``data_ptr()`` and ``is_cuda``
(torch tensors on the detector's device), which are read in place.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from ._lib import LO_INSUFFICIENT, LO_OK, LoIrisCandidate, LoIrisConfig, lib

ROWS, COLS, FEAT_ROWS = 80, 360, 640


@dataclass
class LoopClosureConfig:
    """LoopClosureConfig as the frame loop uses it (lo_iris_config_default)."""
    similarity_threshold: float = 0.3
    min_keyframe_gap: int = 50
    max_search_distance: float = 10.0

    def to_c(self) -> LoIrisConfig:
        return LoIrisConfig(float(self.similarity_threshold), int(self.min_keyframe_gap),
                            float(self.max_search_distance))


@dataclass
class LoopCandidate:
    query_keyframe_id: int
    match_keyframe_id: int
    similarity_score: float
    bias: int


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _position(p) -> np.ndarray:
    p = np.ascontiguousarray(np.asarray(p, dtype=np.float32).reshape(-1))
    if p.shape != (3,):
        raise ValueError("position must have 3 components")
    return p


def _cloud(points):
    """-> (keepalive, pointer as int, n, on_device)."""
    if hasattr(points, "data_ptr") and getattr(points, "is_cuda", False):
        t = points
        if t.dim() != 2 or t.shape[1] != 3 or str(t.dtype) != "torch.float32":
            raise ValueError("device points must be an (N, 3) float32 tensor")
        t = t.contiguous()
        return t, int(t.data_ptr()), int(t.shape[0]), 1
    if hasattr(points, "detach"):
        points = points.detach().cpu().numpy()
    p = np.ascontiguousarray(points, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be an (N, 3) float32 array (Point3D AoS)")
    return p, p.ctypes.data, len(p), 0


def select_host(config: LoopClosureConfig, current_id: int, current_position, ids, positions, distances) -> int:
    """lo_iris_select_host: the candidate selection rule alone (no GPU).  Returns the database index or -1."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(distances, dtype=np.float32)
    if not (len(ids) == len(pos) == len(d)):
        raise ValueError("ids/positions/distances length mismatch")
    cfg = config.to_c()
    cur = _position(current_position)
    return int(lib().lo_iris_select_host(C.byref(cfg), int(current_id), _fptr(cur),
                                         ids.ctypes.data_as(C.POINTER(C.c_int64)), _fptr(pos), _fptr(d), len(ids)))


class IrisLoopDetector:
    """GPU LiDAR-Iris loop-closure detector bound to an ICP context (its device and stream)."""

    def __init__(self, optimizer, capacity: int = 4096, config: LoopClosureConfig | None = None):
        """optimizer: an ``IterativeClosestPointOptimizer`` (or a raw ``lo_ctx`` handle); capacity: database entries."""
        self.config = config or LoopClosureConfig()
        self._L = lib()
        self._owner = optimizer                      # the context must outlive the detector
        ctx = getattr(optimizer, "ctx", optimizer)
        err = C.c_int(0)
        self._h = self._L.lo_iris_create(ctx, int(capacity), C.byref(err))
        if not self._h:
            raise RuntimeError(f"lo_iris_create failed (code {err.value})")

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._L.lo_iris_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise RuntimeError(f"liblo_icp error {rc}: {self._L.lo_iris_last_error(self._h).decode()}")
        return rc

    def __len__(self) -> int:
        return int(self._L.lo_iris_size(self._h))

    @property
    def capacity(self) -> int:
        return int(self._L.lo_iris_capacity(self._h))

    def clear(self):
        self._check(self._L.lo_iris_clear(self._h))

    # ------------------------------------------------------------------ parity entry points
    def image(self, points) -> np.ndarray:
        """LidarIris::GetIris: the 80 x 360 uint8 iris image of a host cloud."""
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((ROWS, COLS), np.uint8)
        self._check(self._L.lo_iris_image(self._h, _fptr(p), len(p), out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def encode(self, image):
        """LoGFeatureEncode: (T, M), 640 x 360 uint8 each (0 / 255)."""
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.shape != (ROWS, COLS):
            raise ValueError("image must be 80 x 360 uint8")
        T = np.zeros((FEAT_ROWS, COLS), np.uint8)
        M = np.zeros((FEAT_ROWS, COLS), np.uint8)
        u8 = C.POINTER(C.c_uint8)
        self._check(self._L.lo_iris_encode(self._h, img.ctypes.data_as(u8), T.ctypes.data_as(u8), M.ctypes.data_as(u8)))
        return T, M

    # ------------------------------------------------------------------ database
    def add_keyframe(self, keyframe_id: int, position, points) -> bool:
        """LoopClosureDetector::add_keyframe: False (nothing added) for an empty cloud."""
        keep, ptr, n, dev = _cloud(points)
        pos = _position(position)
        rc = self._check(self._L.lo_iris_add_keyframe(self._h, int(keyframe_id), _fptr(pos), ptr, n, dev))
        del keep
        return rc == LO_OK

    def add_from_scan(self, keyframe_id: int, position) -> bool:
        """The context's last device-filtered scan (optimize_raw) as the keyframe's cloud, read on the device."""
        pos = _position(position)
        return self._check(self._L.lo_iris_add_from_scan(self._h, int(keyframe_id), _fptr(pos))) == LO_OK

    # ------------------------------------------------------------------ matching
    def compare_all(self, points):
        """The query cloud against every entry: (distance float32, bias, diff, total int32 arrays), or None for an
        empty query cloud."""
        keep, ptr, n, dev = _cloud(points)
        k = len(self)
        dist = np.zeros(k, np.float32)
        bias = np.zeros(k, np.int32)
        diff = np.zeros(k, np.int32)
        total = np.zeros(k, np.int32)
        ip = C.POINTER(C.c_int32)
        rc = self._check(self._L.lo_iris_compare_all(self._h, ptr, n, dev, _fptr(dist), bias.ctypes.data_as(ip),
                                                     diff.ctypes.data_as(ip), total.ctypes.data_as(ip)))
        del keep
        if rc == LO_INSUFFICIENT:
            return None
        return dist, bias, diff, total

    def detect(self, keyframe_id: int, position, points, config: LoopClosureConfig | None = None):
        """detect_loop_closures for the current keyframe (not added): a ``LoopCandidate`` or None."""
        keep, ptr, n, dev = _cloud(points)
        pos = _position(position)
        cfg = (config or self.config).to_c()
        cand = LoIrisCandidate()
        rc = self._check(self._L.lo_iris_detect(self._h, C.byref(cfg), int(keyframe_id), _fptr(pos), ptr, n, dev,
                                                C.byref(cand)))
        del keep
        if rc != LO_OK:
            return None
        return LoopCandidate(int(cand.query_keyframe_id), int(cand.match_keyframe_id), float(cand.distance),
                             int(cand.bias))

    def bench_match(self, reps: int = 20) -> float:
        """Average device milliseconds of one match launch (last query against the current database)."""
        ms = C.c_float(0.0)
        self._check(self._L.lo_iris_bench_match(self._h, int(reps), C.byref(ms)))
        return float(ms.value)


class BatchIrisDetector:
    """One LiDAR-Iris database per job of a ``BatchOptimizer`` behind one handle (``include/lo_iris_batch.h``).

    The keyframes of any subset of jobs are added, and the queries of any subset of jobs are answered, in one set of
    launches on the batch stream.  Per job every result equals an ``IrisLoopDetector`` on that job's context, bit for
    bit.  ``jobs`` lists distinct job indices; ``ids``, ``positions`` and ``clouds`` follow the list's order.  The
    clouds of one call are all numpy arrays or all device tensors."""

    def __init__(self, batch_optimizer, capacity: int, config: LoopClosureConfig | None = None):
        self.config = config or LoopClosureConfig()
        self._L = lib()
        self._owner = batch_optimizer                # the batch must outlive the detector
        err = C.c_int(0)
        self._h = self._L.lo_iris_batch_create(getattr(batch_optimizer, "_b", batch_optimizer), int(capacity),
                                               C.byref(err))
        if not self._h:
            raise RuntimeError(f"lo_iris_batch_create failed (code {err.value})")

    def close(self):
        h = getattr(self, "_h", None)
        if h:
            self._h = None
            self._L.lo_iris_batch_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, statuses=()):
        # a negative code that no job reports is the whole call's
        if rc < 0 and rc not in statuses:
            raise RuntimeError(f"liblo_icp error {rc}: {self._L.lo_iris_batch_last_error(self._h).decode()}")
        return rc

    @property
    def capacity(self) -> int:
        return int(self._L.lo_iris_batch_capacity(self._h))

    def size(self, job: int) -> int:
        return int(self._L.lo_iris_batch_size(self._h, int(job)))

    def clear(self, job: int | None = None):
        self._check(self._L.lo_iris_batch_clear(self._h, -1 if job is None else int(job)))

    @staticmethod
    def _jobs(jobs):
        j = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1)
        return j, j.ctypes.data_as(C.POINTER(C.c_int))

    @staticmethod
    def _keys(k, ids, positions):
        i = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        p = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
        if len(i) != k or len(p) != k:
            raise ValueError(f"need {k} ids and positions")
        return i, p

    @staticmethod
    def _clouds(k, clouds):
        """-> (keepalive, pointer array, count array, on_device)."""
        if len(clouds) != k:
            raise ValueError(f"need {k} clouds")
        c = [_cloud(p) for p in clouds]
        dev = {x[3] for x in c if x[2] > 0}
        if len(dev) > 1:
            raise ValueError("the clouds of one call are all host arrays or all device tensors")
        ptrs = (C.c_void_p * max(k, 1))(*[x[1] if x[2] > 0 else None for x in c])
        ns = (C.c_size_t * max(k, 1))(*[x[2] for x in c])
        return c, ptrs, ns, (dev.pop() if dev else 0)

    # ------------------------------------------------------------------ database
    def add(self, jobs, ids, positions, clouds):
        """lo_iris_batch_add: one status per listed job -- LO_OK, LO_INSUFFICIENT (an empty cloud: nothing added) or
        LO_ERR_CAPACITY (that job's database is full)."""
        j, jp = self._jobs(jobs)
        i, p = self._keys(len(j), ids, positions)
        keep, ptrs, ns, dev = self._clouds(len(j), clouds)
        st = np.zeros(max(len(j), 1), np.int32)
        rc = self._L.lo_iris_batch_add(self._h, jp, len(j), i.ctypes.data_as(C.POINTER(C.c_int64)), _fptr(p), ptrs, ns,
                                       dev, st.ctypes.data_as(C.POINTER(C.c_int)))
        del keep
        st = [int(s) for s in st[:len(j)]]
        self._check(rc, st)
        return st

    def add_from_scans(self, jobs, ids, positions):
        """lo_iris_batch_add_from_scans: the listed jobs' device-filtered scans (``BatchOptimizer.filter_raw``) as
        their keyframes' clouds; statuses as ``add``."""
        j, jp = self._jobs(jobs)
        i, p = self._keys(len(j), ids, positions)
        st = np.zeros(max(len(j), 1), np.int32)
        rc = self._L.lo_iris_batch_add_from_scans(self._h, jp, len(j), i.ctypes.data_as(C.POINTER(C.c_int64)),
                                                  _fptr(p), st.ctypes.data_as(C.POINTER(C.c_int)))
        st = [int(s) for s in st[:len(j)]]
        self._check(rc, st)
        return st

    # ------------------------------------------------------------------ matching
    def detect(self, jobs, ids, positions, clouds=None, config: LoopClosureConfig | None = None):
        """lo_iris_batch_detect: a ``LoopCandidate`` or None per listed job (the keyframes are not added).
        clouds=None: the jobs' device-filtered scans."""
        j, jp = self._jobs(jobs)
        i, p = self._keys(len(j), ids, positions)
        keep, ptrs, ns, dev = (None, None, None, 1) if clouds is None else self._clouds(len(j), clouds)
        cfg = (config or self.config).to_c()
        cand = (LoIrisCandidate * max(len(j), 1))()
        st = np.full(max(len(j), 1), LO_INSUFFICIENT, np.int32)
        rc = self._L.lo_iris_batch_detect(self._h, C.byref(cfg), jp, len(j), i.ctypes.data_as(C.POINTER(C.c_int64)),
                                          _fptr(p), ptrs, ns, dev, cand, st.ctypes.data_as(C.POINTER(C.c_int)))
        del keep
        self._check(rc)
        return [LoopCandidate(int(c.query_keyframe_id), int(c.match_keyframe_id), float(c.distance), int(c.bias))
                if s == LO_OK else None for c, s in zip(cand, st[:len(j)])]

    def compare_all(self, jobs, clouds):
        """lo_iris_batch_compare_all, ungated: per listed job (distance float32, bias, diff, total int32 arrays) over
        its database in insertion order; empty arrays for an empty query cloud."""
        j, jp = self._jobs(jobs)
        keep, ptrs, ns, dev = self._clouds(len(j), clouds)
        cap = sum(self.size(x) for x in j)
        off = np.zeros(len(j) + 1, np.uintp)
        dist = np.zeros(max(cap, 1), np.float32)
        bias, diff, total = (np.zeros(max(cap, 1), np.int32) for _ in range(3))
        ip = C.POINTER(C.c_int32)
        self._check(self._L.lo_iris_batch_compare_all(self._h, jp, len(j), ptrs, ns, dev,
                                                      off.ctypes.data_as(C.POINTER(C.c_size_t)), _fptr(dist),
                                                      bias.ctypes.data_as(ip), diff.ctypes.data_as(ip),
                                                      total.ctypes.data_as(ip), cap))
        del keep
        self.last_offsets = [int(o) for o in off]
        return [tuple(a[int(off[x]):int(off[x + 1])].copy() for a in (dist, bias, diff, total)) for x in range(len(j))]
