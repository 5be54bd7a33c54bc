"""The batched LiDAR-Iris detector (include/lo_iris_batch.h, csrc/lo_iris_batch.hip) against one solo
``IrisLoopDetector`` per job on the same context, fed the same calls in the same order.  The solo detector is itself
pinned to numpy by tests/test_gpu_iris.py.  Everything is compared bit for bit: distances as uint32 patterns (NaN
against NaN), bias / diff / total as integers, candidates field for field.
"""
import ctypes as C

import numpy as np
import pytest

from lidar_odometry_amd import _lib
from tests import _iris_ref as ref

pytestmark = pytest.mark.gpu

B, CAP = 3, 8
ZERO = [0.0, 0.0, 0.0]
EMPTY = np.zeros((0, 3), np.float32)


class Rig:
    """B contexts, their batch, the batched detector, and one solo detector per context."""

    def __init__(self, capacity=CAP):
        from lidar_odometry_amd import (BatchIrisDetector, BatchOptimizer, IrisLoopDetector,
                                        IterativeClosestPointOptimizer)
        self.ctxs = [IterativeClosestPointOptimizer(max_points=1 << 17) for _ in range(B)]
        self.b = BatchOptimizer(self.ctxs)
        self.ib = BatchIrisDetector(self.b, capacity)
        self.solo = [IrisLoopDetector(c, capacity) for c in self.ctxs]

    def close(self):
        for d in self.solo:
            d.close()
        self.ib.close()
        self.b.close()
        for c in self.ctxs:
            c.close()

    def clear(self):
        self.ib.clear()
        for d in self.solo:
            d.clear()

    def add(self, jobs, ids, positions, clouds):
        """The same keyframes to both sides; returns the batched statuses."""
        st = self.ib.add(jobs, ids, positions, clouds)
        for j, i, p, c, s in zip(jobs, ids, positions, clouds, st):
            assert self.solo[j].add_keyframe(i, p, c) == (s == _lib.LO_OK)
        return st

    def sizes(self):
        got = [self.ib.size(j) for j in range(B)]
        assert got == [len(d) for d in self.solo]
        return got

    def same_records(self, jobs, queries):
        """compare_all of both sides, bit for bit; returns the batched records."""
        got = self.ib.compare_all(jobs, queries)
        assert len(got) == len(jobs)
        for x, (j, q) in enumerate(zip(jobs, queries)):
            want = self.solo[j].compare_all(q)
            if want is None:                                # an empty query cloud: zero records
                want = tuple(np.zeros(0, t) for t in (np.float32, np.int32, np.int32, np.int32))
            _same(got[x], want, (x, j))
        return got

    def same_candidates(self, jobs, ids, positions, queries, cfg):
        got = self.ib.detect(jobs, ids, positions, queries, cfg)
        want = [self.solo[j].detect(i, p, q, cfg) for j, i, p, q in zip(jobs, ids, positions, queries)]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert (g is None) == (w is None), (got, want)
            if g is not None:
                assert (g.query_keyframe_id, g.match_keyframe_id, g.bias) == \
                    (w.query_keyframe_id, w.match_keyframe_id, w.bias)
                assert _bits(g.similarity_score) == _bits(w.similarity_score)
        return got


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _same(got, want, what=""):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=str(what))


@pytest.fixture(scope="module")
def rig_module():
    r = Rig()
    yield r
    r.close()


@pytest.fixture()
def rig(rig_module):
    rig_module.clear()
    return rig_module


@pytest.fixture(scope="module")
def clouds():
    """The query scene, a copy turned by +73 degrees (shifted and noisy), two unrelated scenes."""
    a = ref.scene(1)
    return a, ref.yawed(a, 73, (0.3, -0.2, 0.0), 0.02, 3), ref.scene(2), ref.scene(3)


# ---------------------------------------------------------------------------------------------------- add
def test_add_subsets_and_an_empty_cloud(rig, clouds):
    import torch
    a, b, c, d = clouds
    dev = [torch.from_numpy(x).cuda() for x in (a, b)]
    assert rig.add([0, 1], [0, 0], [ZERO, ZERO], [a, b]) == [_lib.LO_OK] * 2
    assert rig.add([0], [1], [ZERO], [c]) == [_lib.LO_OK]
    assert rig.add([0], [2], [ZERO], [d]) == [_lib.LO_OK]
    assert rig.sizes() == [3, 1, 0]
    # an empty cloud: LO_INSUFFICIENT, nothing added for that job
    assert rig.add([1], [5], [ZERO], [EMPTY]) == [_lib.LO_INSUFFICIENT]
    assert rig.sizes() == [3, 1, 0]
    for q in (a, c):
        rig.same_records([0, 1, 2], [q, q, q])
    # ... also beside a real one
    assert rig.add([1, 2], [5, 0], [ZERO, ZERO], [EMPTY, d]) == [_lib.LO_INSUFFICIENT, _lib.LO_OK]
    assert rig.sizes() == [3, 1, 1]
    rig.same_records([2, 1], [d, a])
    rig.solo[2].clear()
    # device clouds give the host clouds' descriptors: jobs 0 and 1 hold [a, ...] and [b]; job 2 gets both from the
    # device, and a device query gives the host query's records
    rig.ib.clear(2)
    assert rig.ib.add([2], [0], [ZERO], [dev[0]]) == [_lib.LO_OK]
    assert rig.ib.add([2], [1], [ZERO], [dev[1]]) == [_lib.LO_OK]
    host = rig.ib.compare_all([0, 1, 2], [c, c, c])
    devq = rig.ib.compare_all([0, 1, 2], [torch.from_numpy(c).cuda()] * 3)
    for h, g in zip(host, devq):
        _same(g, h)
    for k in range(4):
        assert host[2][k][0:1].view(np.uint32) == host[0][k][0:1].view(np.uint32)      # a: device = host
        assert host[2][k][1:2].view(np.uint32) == host[1][k][0:1].view(np.uint32)      # b


# ---------------------------------------------------------------------------------------------------- compare_all
def _fill_015(rig, clouds):
    a, b, c, d = clouds
    five = [c, b, a, d, ref.scene(4)]
    rig.add([1], [0], [ZERO], [b])
    for k, p in enumerate(five):
        rig.add([2], [k], [ZERO], [p])
    assert rig.sizes() == [0, 1, 5]


def test_compare_all_sizes_0_1_5_and_list_order(rig, clouds):
    a = clouds[0]
    _fill_015(rig, clouds)
    fwd = rig.same_records([0, 1, 2], [a, a, a])
    assert rig.ib.last_offsets == [0, 0, 1, 6]
    assert [len(r[0]) for r in fwd] == [0, 1, 5]
    assert fwd[2][0][2] == 0.0 and fwd[2][1][2] == 0            # job 2's entry 2 is the query itself
    assert fwd[1][1][0] == 73                                   # the turned copy
    rev = rig.same_records([2, 1, 0], [a, a, a])
    assert rig.ib.last_offsets == [0, 5, 6, 6]
    for x in range(3):
        _same(rev[x], fwd[2 - x])
    # different queries per job, and an empty query cloud among them
    got = rig.same_records([2, 0, 1], [clouds[2], a, EMPTY])
    assert rig.ib.last_offsets == [0, 5, 5, 5]
    assert got[0][0][0] == 0.0                                  # job 2's entry 0 is clouds[2]


def test_compare_all_capacity(rig, clouds):
    a = clouds[0]
    _fill_015(rig, clouds)
    L = _lib.lib()
    jobs = (C.c_int * 3)(0, 1, 2)
    ptrs = (C.c_void_p * 3)(*[a.ctypes.data] * 3)
    ns = (C.c_size_t * 3)(*[len(a)] * 3)
    off = (C.c_size_t * 4)()
    dist = np.full(6, -1.0, np.float32)
    fp = dist.ctypes.data_as(C.POINTER(C.c_float))
    assert L.lo_iris_batch_compare_all(rig.ib._h, jobs, 3, ptrs, ns, 0, off, fp, None, None, None, 5) == \
        _lib.LO_ERR_CAPACITY
    assert (dist == -1.0).all() and list(off) == [0, 0, 1, 6]
    # every output array may be NULL, offsets included
    assert L.lo_iris_batch_compare_all(rig.ib._h, jobs, 3, ptrs, ns, 0, None, fp, None, None, None, 6) == _lib.LO_OK
    _same([dist[1:]], [rig.solo[2].compare_all(a)[0]])


# ---------------------------------------------------------------------------------------------------- NaN
def test_fully_masked_pair_is_nan_and_leaves_its_neighbours(rig, clouds):
    a, b, c, _ = clouds
    far = np.array([[100.0, 0.3, 0.2]], np.float32)        # one point beyond 80 m: only image row 79 is live
    assert not ref.image(a)[79].any()                      # the query has nothing there: every bit is masked
    rig.add([0, 1], [0, 0], [ZERO, ZERO], [b, far])
    rig.add([0, 1], [1, 1], [ZERO, ZERO], [c, a])
    rig.add([0], [2], [ZERO], [a])
    got = rig.same_records([0, 1], [a, a])
    dist, bias, diff, total = got[1]
    assert np.isnan(dist[0]) and (bias[0], diff[0], total[0]) == (-1, 0, 0)
    assert dist[1] == 0.0 and bias[1] == 0 and total[1] > 0
    assert not np.isnan(got[0][0]).any() and got[0][0][2] == 0.0


# ---------------------------------------------------------------------------------------------------- detect
def _detect_case(rig, clouds):
    """Job 0: the turned copy, eligible.  Job 1: the turned copy too young, an unrelated scene eligible.  Job 2: the
    turned copy too far, an unrelated scene eligible."""
    a, b, c, d = clouds
    rig.add([0, 1, 2], [10, 80, 10], [[1.0, 1.0, 0.0], [1.0, 0.0, 0.0], [30.0, 0.0, 0.0]], [b, b, b])
    rig.add([0, 1, 2], [20, 5, 20], [[2.0, 0.0, 0.0], [0.5, 0.5, 0.0], [3.0, -2.0, 0.5]], [c, c, c])
    rig.add([0], [90], [[0.2, 0.0, 0.0]], [a])             # job 0: the scene itself, but only 10 keyframes ago
    return a


def test_detect_equals_solo_detect(rig, clouds):
    from lidar_odometry_amd import LoopClosureConfig
    a = _detect_case(rig, clouds)
    jobs, ids, pos, qs = [0, 1, 2], [100, 100, 100], [ZERO] * 3, [a, a, a]
    cfg = LoopClosureConfig()
    got = rig.same_candidates(jobs, ids, pos, qs, cfg)
    assert got[0] is not None and got[1] is None and got[2] is None
    solo_rec = rig.solo[0].compare_all(a)
    assert (got[0].query_keyframe_id, got[0].match_keyframe_id, got[0].bias) == (100, 10, 73)
    assert _bits(got[0].similarity_score) == _bits(solo_rec[0][0]) and got[0].bias == solo_rec[1][0]
    # the gated-out copies would have matched: ungated, jobs 1 and 2 see them under the threshold
    rec = rig.ib.compare_all([1, 2], [a, a])
    assert rec[0][0][0] <= cfg.similarity_threshold < rec[0][0][1]
    assert rec[1][0][0] <= cfg.similarity_threshold < rec[1][0][1]
    # everything eligible: the scene itself wins in job 0, the copies in jobs 1 and 2
    wide = LoopClosureConfig(0.3, 1, 1e6)
    got = rig.same_candidates(jobs, ids, pos, qs, wide)
    assert [g.match_keyframe_id for g in got] == [90, 80, 10]
    # a subset in another order, different ids and positions per job
    rig.same_candidates([2, 0], [100, 140], [[29.0, 0.0, 0.0], ZERO], [a, a], cfg)
    assert rig.sizes() == [3, 2, 2]                         # detect adds nothing


def test_detect_with_an_empty_database_and_an_empty_cloud(rig, clouds):
    from lidar_odometry_amd import LoopClosureConfig
    a, b, _, _ = clouds
    rig.add([0, 1], [10, 10], [ZERO, ZERO], [b, b])
    wide = LoopClosureConfig(0.3, 1, 1e6)
    got = rig.same_candidates([0, 1, 2], [100] * 3, [ZERO] * 3, [a, EMPTY, a], wide)
    assert got[0] is not None and got[1] is None and got[2] is None
    # no job has an eligible entry: nothing to launch, every job answers None
    assert rig.same_candidates([0, 1, 2], [11] * 3, [ZERO] * 3, [a, a, a], LoopClosureConfig()) == [None] * 3


def test_tie_goes_to_the_lower_index(rig, clouds):
    from lidar_odometry_amd import LoopClosureConfig
    a, b, c, _ = clouds
    rig.add([1], [3], [ZERO], [c])
    rig.add([1], [7], [[1.0, 0.0, 0.0]], [b])
    rig.add([1], [9], [[0.0, 1.0, 0.0]], [b])
    got = rig.same_candidates([1], [100], [ZERO], [a], LoopClosureConfig())
    assert got[0] is not None and got[0].match_keyframe_id == 7
    rec = rig.ib.compare_all([1], [a])[0]
    assert _bits(rec[0][1]) == _bits(rec[0][2])


# ---------------------------------------------------------------------------------------------------- scans
def _raw(seed, n=20000):
    rng = np.random.default_rng(seed)
    p = ref.scene(seed)
    return np.ascontiguousarray(np.concatenate([p, p + rng.normal(0, 0.05, p.shape).astype(np.float32)] * 2)[:n])


def test_add_from_scans_equals_add_from_scan(rig, clouds):
    a = clouds[0]
    raws = [_raw(21), np.zeros((0, 3), np.float32), _raw(22)]
    counts = rig.b.filter_raw(raws, stride=2, voxel_size=0.5)
    assert counts[0] > 1000 and counts[1] == 0 and counts[2] > 1000
    st = rig.ib.add_from_scans([0, 1, 2], [4, 5, 6], [ZERO] * 3)
    assert st == [_lib.LO_OK, _lib.LO_INSUFFICIENT, _lib.LO_OK]
    for j in range(B):
        assert rig.solo[j].add_from_scan(4 + j, ZERO) == (st[j] == _lib.LO_OK)
    assert rig.sizes() == [1, 0, 1]
    rig.same_records([0, 1, 2], [a, a, a])
    # a query of the scans themselves (clouds=None) finds what was just added, as the solo detector given the host copy
    from lidar_odometry_amd import LoopClosureConfig
    wide = LoopClosureConfig(0.3, 1, 1e6)
    got = rig.ib.detect([0, 1, 2], [50] * 3, [ZERO] * 3, None, wide)
    want = [rig.solo[j].detect(50, ZERO, rig.ctxs[j].filtered_points(), wide) for j in range(B)]
    assert got[1] is None and want[1] is None
    for j in (0, 2):
        assert (got[j].match_keyframe_id, got[j].bias) == (4 + j, 0) == (want[j].match_keyframe_id, want[j].bias)
        assert _bits(got[j].similarity_score) == _bits(want[j].similarity_score) == 0
    # scans whose counts only the device knows (each context's own filter): one readback fetches them all
    for j, r in enumerate((_raw(23), _raw(24), _raw(25))):
        assert len(rig.ctxs[j].voxel_filter(r, 0.5, 2)) > 1000
    assert rig.ib.add_from_scans([2, 0, 1], [7, 8, 9], [ZERO] * 3) == [_lib.LO_OK] * 3
    for j in range(B):
        assert rig.solo[j].add_from_scan(7, ZERO)
    assert rig.sizes() == [2, 1, 2]
    rig.same_records([0, 1, 2], [a, a, a])


# ---------------------------------------------------------------------------------------------------- errors
def _raw_add(rig, jobs, cloud):
    L = _lib.lib()
    k = len(jobs)
    ja = (C.c_int * k)(*jobs)
    ids = (C.c_int64 * k)(*range(k))
    pos = (C.c_float * (3 * k))()
    ptrs = (C.c_void_p * k)(*[cloud.ctypes.data] * k)
    ns = (C.c_size_t * k)(*[len(cloud)] * k)
    st = (C.c_int * k)(*[77] * k)
    return L.lo_iris_batch_add(rig.ib._h, ja, k, ids, pos, ptrs, ns, 0, st), list(st)


def test_bad_job_lists_add_nothing(rig, clouds):
    a = clouds[0]
    for jobs in ([0, 1, 0], [1, 1], [0, B], [-1], [2, 0, 7]):
        rc, st = _raw_add(rig, jobs, a)
        assert rc == _lib.LO_ERR_ARG and st == [77] * len(jobs), jobs
        assert rig.ib.size(0) == rig.ib.size(1) == rig.ib.size(2) == 0
        with pytest.raises(RuntimeError):
            rig.ib.add(jobs, list(range(len(jobs))), [ZERO] * len(jobs), [a] * len(jobs))
        with pytest.raises(RuntimeError):
            rig.ib.detect(jobs, list(range(len(jobs))), [ZERO] * len(jobs), [a] * len(jobs))
        with pytest.raises(RuntimeError):
            rig.ib.compare_all(jobs, [a] * len(jobs))
    assert rig.ib.compare_all([], []) == []


def test_capacity_is_per_job_and_clear_empties_one_job(clouds):
    a, b, c, _ = clouds
    r = Rig(capacity=2)
    try:
        assert r.ib.capacity == 2
        r.add([0, 1], [0, 0], [ZERO, ZERO], [a, b])
        r.add([0], [1], [ZERO], [b])
        st = r.ib.add([0, 1, 2], [2, 1, 0], [ZERO] * 3, [c, c, c])
        assert st == [_lib.LO_ERR_CAPACITY, _lib.LO_OK, _lib.LO_OK]
        r.solo[1].add_keyframe(1, ZERO, c)
        r.solo[2].add_keyframe(0, ZERO, c)
        assert r.sizes() == [2, 2, 1]
        rc, st = _raw_add(r, [0, 2], a)
        assert rc == _lib.LO_ERR_CAPACITY and st == [_lib.LO_ERR_CAPACITY, _lib.LO_OK]
        r.solo[2].add_keyframe(1, ZERO, a)
        assert r.sizes() == [2, 2, 2]
        r.same_records([0, 1, 2], [a, a, a])
        r.ib.clear(1)
        r.solo[1].clear()
        assert r.sizes() == [2, 0, 2]
        r.add([1], [4], [ZERO], [a])
        got = r.same_records([0, 1, 2], [a, a, a])
        assert got[1][0][0] == 0.0
        r.ib.clear()
        assert [r.ib.size(j) for j in range(B)] == [0, 0, 0]
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------------- interleaving
def test_batched_calls_leave_the_solo_detectors_alone_and_repeat(rig, clouds):
    from lidar_odometry_amd import LoopClosureConfig
    a = _detect_case(rig, clouds)
    wide = LoopClosureConfig(0.3, 1, 1e6)
    before = [rig.solo[j].compare_all(a) for j in range(B)]
    cand_before = [rig.solo[j].detect(100, ZERO, a, wide) for j in range(B)]
    first = rig.ib.detect([0, 1, 2], [100] * 3, [ZERO] * 3, [a] * 3, wide)
    rec_first = rig.ib.compare_all([0, 1, 2], [a] * 3)
    # a batched add of other keyframes, a batched query of another cloud
    assert rig.ib.add([0, 1, 2], [95, 96, 97], [ZERO] * 3, [clouds[3]] * 3) == [_lib.LO_OK] * 3
    rig.ib.detect([2, 1], [200, 200], [ZERO] * 2, [clouds[2]] * 2, wide)
    for j in range(B):
        _same(rig.solo[j].compare_all(a), before[j], j)
        assert rig.solo[j].detect(100, ZERO, a, wide) == cand_before[j]
    # the earlier entries answer as before, and a second detect gives the first one's bits
    rec_again = rig.ib.compare_all([0, 1, 2], [a] * 3)
    for j in range(B):
        _same([x[:len(before[j][0])] for x in rec_again[j]], rec_first[j], j)
    gap = LoopClosureConfig(0.3, 6, 1e6)                    # the three new keyframes are too young for it
    again = rig.ib.detect([0, 1, 2], [100] * 3, [ZERO] * 3, [a] * 3, gap)
    third = rig.ib.detect([0, 1, 2], [100] * 3, [ZERO] * 3, [a] * 3, gap)
    for f, g, h in zip(first, again, third):
        assert f is not None and f == g == h
        assert _bits(f.similarity_score) == _bits(g.similarity_score) == _bits(h.similarity_score)
