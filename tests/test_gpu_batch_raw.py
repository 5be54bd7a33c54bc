"""GPU tests of the raw-scan batch (lo_batch_filter_raw*, lo_batch_optimize_raw): Estimator::preprocess_frame's
FastVoxelFilter (Estimator.cpp:561-588, VoxelMap.h:73-104) for B contexts in one set of batched launches, then the
batched optimize on the filtered clouds.

Bar: every job's filtered cloud equals the oracle restatement and the same context's single-scan voxel_filter in
order, bits and count; every optimize record equals the same context's own optimize on the filtered cloud bit for
bit.  Every equality is on bits (.view(np.uint32)).  The inputs' voxel populations are asserted, so a changed
generator cannot silently skip one of the device's summation paths (<= 16, 17..64, 65..1024, > 1024 members).
"""
import functools

import numpy as np
import pytest

import oracle
from lidar_odometry_amd._lib import LO_ERR_ARG, LO_ERR_CAPACITY, LO_ERR_STATE
from tests import _data

pytestmark = pytest.mark.gpu

MAXP = 1 << 16


# ---------------------------------------------------------------- inputs (CPU; built once, never modified)
def populations(raw, voxel, stride):
    """Members per voxel of the sampled, finite points (computeMortonKey's cells, VoxelMap.h:123-135)."""
    p = np.asarray(raw, np.float32)[::stride]
    p = p[np.isfinite(p).all(axis=1)]
    if len(p) == 0:
        return np.zeros(0, np.int64)
    inv = np.float32(1.0) / np.float32(voxel)
    f = np.floor(p * inv)
    cell = np.where(np.abs(f) >= 9.2233720e18, 0.0, np.clip(f + 2.0 ** 20, 0.0, 2.0 ** 21 - 1)).astype(np.int64)
    key = cell[:, 0] | (cell[:, 1] << 21) | (cell[:, 2] << 42)
    return np.unique(key, return_counts=True)[1]


def density_mix():
    """The cloud of test_voxel_filter_density_mix_and_signed_zero: voxels of 1..16, 17..64 and > 64 members."""
    rng = np.random.default_rng(11)
    centers = rng.integers(-40, 40, size=(600, 3)).astype(np.float32) * 0.5 + 0.25
    counts = np.concatenate([rng.integers(1, 17, 300), rng.integers(17, 65, 200), rng.integers(65, 300, 100)])
    pts = np.concatenate([c + rng.uniform(-0.2, 0.2, size=(k, 3)).astype(np.float32) for c, k in zip(centers, counts)])
    pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(np.concatenate([pts, np.array([[-0.0, 100.0, -0.0]], np.float32)]))


def one_voxel(n=3000, seed=21):
    return np.random.default_rng(seed).uniform(0.0, 0.49, size=(n, 3)).astype(np.float32)


def edge_cases():
    """The cloud of test_voxel_filter_edge_cases (shorter): NaN, inf, +-1e30 and +-6e5 among ordinary points."""
    raw = np.random.default_rng(9).normal(scale=20.0, size=(6000, 3)).astype(np.float32)
    raw[5] = [np.nan, 0, 0]
    raw[13] = [0, np.inf, 0]
    raw[21] = [1e30, 2.0, 3.0]
    raw[29] = [-1e30, 2.0, 3.0]
    raw[37] = [6e5, -6e5, 1.0]
    raw[45] = [-6e5, 6e5, 1.0]
    return raw


def random_cloud(n, seed, scale=6.0):
    return np.random.default_rng(seed).normal(scale=scale, size=(n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mixed_jobs():
    return (density_mix(), one_voxel(), edge_cases(), np.full((100, 3), np.nan, np.float32),
            np.zeros((0, 3), np.float32), random_cloud(1025, 31))


@functools.lru_cache(maxsize=None)
def ref_filter(key, stride, voxel=0.5):
    """oracle.voxel_filter of a named input, computed once and shared."""
    kind, i = key
    raw = mixed_jobs()[i] if kind == "mixed" else _data.kitti_scan(i)
    out = oracle.voxel_filter(raw, voxel, stride)
    out.setflags(write=False)
    return out


def assert_bits(got, ref, msg=""):
    assert got.shape == ref.shape, f"{msg}: count {got.shape} vs {ref.shape}"
    np.testing.assert_array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32),
                                  err_msg=msg)


# ---------------------------------------------------------------- contexts and batches
def _ctxs(count, max_points=MAXP):
    from lidar_odometry_amd import IterativeClosestPointOptimizer
    return [IterativeClosestPointOptimizer(max_points=max_points) for _ in range(count)]


class _Batch:
    """count contexts and their batch, closed together."""

    def __init__(self, count, max_points=MAXP):
        from lidar_odometry_amd import BatchOptimizer
        self.ctxs = _ctxs(count, max_points)
        self.b = BatchOptimizer(self.ctxs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.b.close()
        for o in self.ctxs:
            o.close()


@pytest.fixture(scope="module")
def six():
    with _Batch(6) as s:
        yield s


def _check_filter(s, raws, refs, stride, voxel=0.5, msg=""):
    counts = s.b.filter_raw(raws, stride=stride, voxel_size=voxel)
    assert counts == [len(r) for r in refs], f"{msg}: counts {counts}"
    for j, (o, ref) in enumerate(zip(s.ctxs, refs)):
        assert_bits(o.filtered_points(), ref, f"{msg} job {j}")


# ---------------------------------------------------------------- 1. filter parity, mixed jobs
def test_mixed_job_populations():
    """The inputs reach every summation path of the device filter (checked on the CPU oracle's side)."""
    jobs = mixed_jobs()
    for stride in (1, 3):
        for i, raw in enumerate(jobs):
            assert len(ref_filter(("mixed", i), stride)) == len(populations(raw, 0.5, stride)), (i, stride)
        mix = populations(jobs[0], 0.5, stride)
        assert (mix <= 16).any() and ((mix > 16) & (mix <= 64)).any() and (mix > 64).any(), stride
    assert ((populations(jobs[0], 0.5, 1) > 64) & (populations(jobs[0], 0.5, 1) <= 1024)).any()
    assert populations(jobs[1], 0.5, 1).max() > 1024                   # beyond the 1024-member LDS sort
    assert 64 < populations(jobs[1], 0.5, 3).max() <= 1024             # stride 3: the LDS sort itself
    assert np.isfinite(jobs[2]).all(axis=1).sum() == len(jobs[2]) - 2 and len(ref_filter(("mixed", 2), 1)) > 1000
    assert len(ref_filter(("mixed", 3), 1)) == 0 and len(ref_filter(("mixed", 4), 1)) == 0
    assert len(jobs[5]) == 1025 and len(ref_filter(("mixed", 5), 1)) > 256


@pytest.mark.parametrize("stride", [1, 3])
def test_filter_mixed_jobs_bitwise(six, stride):
    jobs = mixed_jobs()
    refs = [ref_filter(("mixed", i), stride) for i in range(6)]
    _check_filter(six, jobs, refs, stride, msg=f"stride {stride}")
    for j, (o, raw, ref) in enumerate(zip(six.ctxs, jobs, refs)):      # and the same context's single-scan filter
        assert_bits(o.voxel_filter(raw, 0.5, stride), ref, f"single job {j}")


# ---------------------------------------------------------------- 2. KITTI scans
def test_filter_kitti_scans_bitwise():
    frames = (3, 11, 20)
    raws = [_data.kitti_scan(f) for f in frames]
    assert len({len(r) for r in raws}) == 3
    refs = [ref_filter(("kitti", f), 8) for f in frames]
    assert all(len(r) > 1000 for r in refs)
    with _Batch(3) as s:
        _check_filter(s, raws, refs, 8, msg="kitti")


# ---------------------------------------------------------------- 3. reuse and interleaving
def test_filter_reuse_and_interleaving(six):
    """The slot resets leave clean tables in both directions: batch, batch with the inputs moved to other contexts,
    a single-context filter, batch again."""
    jobs = mixed_jobs()
    refs = [ref_filter(("mixed", i), 1) for i in range(6)]
    perm = [3, 0, 5, 1, 2, 4]
    _check_filter(six, jobs, refs, 1, msg="first")
    _check_filter(six, [jobs[i] for i in perm], [refs[i] for i in perm], 1, msg="permuted")
    assert_bits(six.ctxs[1].voxel_filter(jobs[2], 0.5, 1), refs[2], "single on context 1")
    _check_filter(six, jobs, refs, 1, msg="after single")


# ---------------------------------------------------------------- 4. growth
def test_filter_buffers_grow():
    small = [random_cloud(2000, 40 + j) for j in range(3)]
    large = [random_cloud(40000, 50 + j, scale=12.0) for j in range(3)]
    with _Batch(3) as s:
        _check_filter(s, small, [oracle.voxel_filter(r, 0.5, 1) for r in small], 1, msg="2k")
        refs = [oracle.voxel_filter(r, 0.5, 1) for r in large]
        assert all(len(r) > 4096 for r in refs)                        # past the buffers' first size
        _check_filter(s, large, refs, 1, msg="40k")
        _check_filter(s, small, [oracle.voxel_filter(r, 0.5, 1) for r in small], 1, msg="2k again")


# ---------------------------------------------------------------- 5. many tiny jobs, a batch of one
def test_filter_many_tiny_jobs_and_batch_of_one():
    rng = np.random.default_rng(77)
    sizes = rng.integers(50, 301, 70)
    raws = [random_cloud(int(n), 100 + j, scale=2.0) for j, n in enumerate(sizes)]
    refs = [oracle.voxel_filter(r, 0.5, 1) for r in raws]
    assert len(raws) > 64 and all(0 < len(r) for r in refs)
    with _Batch(70) as s:
        _check_filter(s, raws, refs, 1, msg="tiny")
    with _Batch(1) as s:
        _check_filter(s, [mixed_jobs()[0]], [ref_filter(("mixed", 0), 1)], 1, msg="one")


# ---------------------------------------------------------------- 6. pinned input
def test_filter_pinned_input(six):
    from lidar_odometry_amd import pinned_empty
    jobs = list(mixed_jobs())
    refs = [ref_filter(("mixed", i), 3) for i in range(6)]
    pr = pinned_empty(jobs[0].shape)
    pr[:] = jobs[0]
    jobs[0] = pr
    _check_filter(six, jobs, refs, 3, msg="pinned")
    del jobs, pr


# ---------------------------------------------------------------- 7-9. optimize
FRAMES = (11, 17, 19, 25)


@functools.lru_cache(maxsize=None)
def opt_cases():
    return tuple(_data.kitti_case(f) for f in FRAMES)


@pytest.fixture(scope="module")
def four():
    """Four contexts with their cases' maps (reference-exact mode, the default) and their batch."""
    with _Batch(4) as s:
        for o, (m, _, _, _) in zip(s.ctxs, opt_cases()):
            k, n, c = _data.surfels(m)
            o.set_surfels(k, n, c)
        yield s


def _single_records(ctxs):
    """Each context's own optimize on the filtered cloud: (ok, pose12, iterations, n_corr, costs, alpha)."""
    out = []
    for o, (_, pts, Ti, _) in zip(ctxs, opt_cases()):
        ok, To = o.optimize(None, pts, Ti)
        st = o.get_last_stats()
        out.append((ok, To.reshape(12).copy(), st.num_iterations, st.num_correspondences,
                    np.float32(st.initial_cost), np.float32(st.final_cost), st.iterations[-1]["alpha"]))
    return out


def _check_records(res, singles, msg=""):
    for j, (r, s) in enumerate(zip(res, singles)):
        ok, To, it, nc, c0, c1, alpha = s
        assert r.success == ok, f"{msg} job {j}: success"
        assert_bits(r.pose.reshape(12), To, f"{msg} job {j} pose")
        assert (r.iterations, r.n_corr) == (it, nc), f"{msg} job {j}: {r.iterations, r.n_corr} vs {it, nc}"
        assert np.float32(r.initial_cost).view(np.uint32) == c0.view(np.uint32), f"{msg} job {j}: initial cost"
        assert np.float32(r.final_cost).view(np.uint32) == c1.view(np.uint32), f"{msg} job {j}: final cost"
        assert np.float64(r.alpha).view(np.uint64) == np.float64(alpha).view(np.uint64), f"{msg} job {j}: alpha"


def _raws():
    return [_data.kitti_scan(f) for f in FRAMES]


def test_optimize_raw_exact_bitwise(four):
    cases = opt_cases()
    singles = _single_records(four.ctxs)
    assert all(s[0] for s in singles)
    res = four.b.optimize_raw(None, _raws(), [c[2] for c in cases], stride=8, voxel_size=0.5)
    assert four.b.last_counts == [len(c[1]) for c in cases]
    _check_records(res, singles, "exact")
    for j, (o, c) in enumerate(zip(four.ctxs, cases)):
        assert_bits(o.filtered_points(), c[1], f"filtered job {j}")
        assert_bits(c[1], ref_filter(("kitti", FRAMES[j]), 8), f"oracle job {j}")
    for j, (o, c, raw) in enumerate(zip(four.ctxs, cases, _raws())):   # the single raw path's pose
        ok, To = o.optimize_raw(None, raw, c[2], stride=8, voxel_size=0.5)
        assert ok == res[j].success
        assert_bits(To.reshape(12), res[j].pose.reshape(12), f"single raw job {j}")


@pytest.mark.parametrize("fast", [(0, 1, 2, 3), (1, 2)], ids=["fast", "mixed"])
def test_optimize_raw_fast_and_mixed_bitwise(four, fast):
    cases = opt_cases()
    try:
        for j, o in enumerate(four.ctxs):
            o.set_exact(j not in fast)
        singles = _single_records(four.ctxs)
        res = four.b.optimize_raw(None, _raws(), [c[2] for c in cases], stride=8, voxel_size=0.5)
        _check_records(res, singles, "fast" if len(fast) == 4 else "mixed")
        for j, (o, c) in enumerate(zip(four.ctxs, cases)):
            assert_bits(o.filtered_points(), c[1], f"filtered job {j}")
    finally:
        for o in four.ctxs:
            o.set_exact(True)


def test_two_phase_filter_then_optimize(four):
    cases = opt_cases()
    singles = _single_records(four.ctxs)
    T = [c[2] for c in cases]
    counts = four.b.filter_raw(_raws(), stride=8, voxel_size=0.5)
    assert counts == [len(c[1]) for c in cases]
    four.b.optimize_async([0] * 4, counts, T)
    _check_records(four.b.result(), singles, "two-phase")
    # a job whose filter count is 0: LO_INSUFFICIENT with pose = T_init
    raws = _raws()
    raws[2] = np.full((500, 3), np.nan, np.float32)
    counts = four.b.filter_raw(raws, stride=8, voxel_size=0.5)
    assert counts[2] == 0 and counts[0] == len(cases[0][1])
    four.b.optimize_async([0] * 4, counts, T)
    res = four.b.result()
    assert not res[2].success
    assert_bits(res[2].pose.reshape(12), np.asarray(T[2], np.float32), "empty job pose")
    _check_records([res[0], res[1], res[3]], [singles[0], singles[1], singles[3]], "beside an empty job")
    res = four.b.optimize_raw(None, raws, T, stride=8, voxel_size=0.5)
    assert not res[2].success and four.b.last_counts[2] == 0
    assert_bits(res[2].pose.reshape(12), np.asarray(T[2], np.float32), "empty job pose (optimize_raw)")


# ---------------------------------------------------------------- 10. errors
def _rc(b, call):
    """The error code of a refused call (BatchOptimizer raises 'liblo_icp batch error <rc>: ...')."""
    with pytest.raises(RuntimeError) as e:
        call()
    return int(str(e.value).split("error")[1].split(":")[0])


def test_errors_refuse_and_leave_the_batch_usable():
    import ctypes as C
    from lidar_odometry_amd import _lib
    raws = [random_cloud(900, 61), random_cloud(700, 62)]
    refs = [oracle.voxel_filter(r, 0.5, 1) for r in raws]
    T = [np.eye(3, 4, dtype=np.float32)] * 2
    with _Batch(2, max_points=1024) as s:
        def valid(msg):
            _check_filter(s, raws, refs, 1, msg=msg)
        valid("before")
        assert _rc(s.b, lambda: s.b.filter_raw(raws, stride=0)) == LO_ERR_ARG
        valid("after stride 0")
        assert _rc(s.b, lambda: s.b.filter_raw(raws, voxel_size=0.0)) == LO_ERR_ARG
        assert _rc(s.b, lambda: s.b.optimize_raw(None, raws, T, stride=0)) == LO_ERR_ARG
        assert _rc(s.b, lambda: s.b.optimize_raw(None, raws, T, voxel_size=0.0)) == LO_ERR_ARG
        valid("after voxel 0")
        big = [raws[0], random_cloud(2000, 63)]
        assert _rc(s.b, lambda: s.b.filter_raw(big, stride=1)) == LO_ERR_CAPACITY
        assert _rc(s.b, lambda: s.b.optimize_raw(None, big, T, stride=1)) == LO_ERR_CAPACITY
        valid("after capacity")
        assert s.b.filter_raw(big, stride=2) == [len(oracle.voxel_filter(r, 0.5, 2)) for r in big]   # m = 1000 fits
        # null arrays and a null scan with points, through the C ABI itself
        L, B = _lib.lib(), 2
        ptrs = (C.c_void_p * B)(raws[0].ctypes.data, None)
        ns = (C.c_size_t * B)(len(raws[0]), 5)
        out = (C.c_size_t * B)()
        assert L.lo_batch_filter_raw(s.b._b, ptrs, ns, 1, 0.5, out) == LO_ERR_ARG
        assert L.lo_batch_filter_raw(s.b._b, None, ns, 1, 0.5, out) == LO_ERR_ARG
        assert L.lo_batch_filter_raw(s.b._b, ptrs, None, 1, 0.5, out) == LO_ERR_ARG
        assert L.lo_batch_filter_raw(s.b._b, ptrs, ns, 1, 0.5, None) == LO_ERR_ARG
        valid("after null arguments")
        # a batch in flight
        counts = s.b.filter_raw(raws, stride=1)
        s.b.optimize_async([0] * B, counts, T)
        assert _rc(s.b, lambda: s.b.filter_raw(raws, stride=1)) == LO_ERR_STATE
        assert _rc(s.b, lambda: s.b.optimize_raw(None, raws, T, stride=1)) == LO_ERR_STATE
        s.b.result()
        valid("after state")


# ---------------------------------------------------------------- 11. buffers
def test_raw_batch_returns_its_memory():
    from lidar_odometry_amd import lib
    raws = [random_cloud(3000, 71), random_cloud(9000, 72)]
    T = [np.eye(3, 4, dtype=np.float32)] * 2

    def live():
        return int(lib().lo_debug_live_bytes())

    for _ in range(2):                      # the second pass would show a leak that a first-use allocation hides
        base = live()
        with _Batch(2, max_points=1 << 14) as s:
            with_batch = live()
            assert with_batch > base
            s.b.filter_raw(raws, stride=1)              # pageable staging + the filter's buffers, one grown past 4096
            assert live() > with_batch
            s.b.optimize_raw(None, raws, T, stride=2)
        assert live() == base
