"""The batched loop-closure ICP's C ABI (lo_batch_optimize_loop_dev) as the Python side binds it: the export, the
binding, the two struct mirrors against the header's field list, and the null-batch argument check.  No GPU call."""
import ctypes as C

from lidar_odometry_amd import _lib
from lidar_odometry_amd.icp import BatchOptimizer


def _layout(fields):
    """sizeof of a C struct from (size, alignment) per field, by the C layout rules."""
    off, amax = 0, 1
    for size, align in fields:
        off = (off + align - 1) // align * align + size
        amax = max(amax, align)
    return (off + amax - 1) // amax * amax


def test_symbol_is_exported_and_bound():
    L = _lib.lib()
    assert "lo_batch_optimize_loop_dev" in _lib.EXPORTED_SYMBOLS
    f = L.lo_batch_optimize_loop_dev
    assert f.restype is C.c_int
    assert len(f.argtypes) == 6


def test_struct_mirrors_match_the_header_layout():
    p, sz = C.sizeof(C.c_void_p), C.sizeof(C.c_size_t)
    # lo_loop_job: int job | const float* d_curr | size_t n_curr | float T_curr[12] | const float* d_matched |
    #              size_t n_matched | float T_matched[12]
    job = _layout([(4, 4), (p, p), (sz, sz)] + [(4, 4)] * 12 + [(p, p), (sz, sz)] + [(4, 4)] * 12)
    assert job == 8 + 2 * p + 2 * sz + 24 * 4            # the 4-byte int padded to 8, two pointers, two size_t, 24 floats
    assert C.sizeof(_lib.LoLoopJob) == job
    assert _lib.LoLoopJob.d_curr.offset == 8 and _lib.LoLoopJob.T_matched.offset == job - 48
    # lo_loop_rec: int status, converged, iterations, n_corr | float T_rel[12] | float inlier_ratio, initial_cost,
    #              final_cost | int rerun
    rec = _layout([(4, 4)] * (4 + 12 + 3 + 1))
    assert rec == 80
    assert C.sizeof(_lib.LoLoopRec) == rec
    assert _lib.LoLoopRec.T_rel.offset == 16 and _lib.LoLoopRec.rerun.offset == 76


def test_null_batch_is_an_argument_error():
    L = _lib.lib()
    jobs = (_lib.LoLoopJob * 1)()
    recs = (_lib.LoLoopRec * 1)()
    assert L.lo_batch_optimize_loop_dev(None, jobs, 1, recs, None, None) == _lib.LO_ERR_ARG
    assert L.lo_batch_optimize_loop_dev(None, None, 0, None, None, None) == _lib.LO_ERR_ARG


def test_python_entry_exists():
    assert callable(BatchOptimizer.optimize_loop_dev)
