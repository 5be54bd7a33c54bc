"""grid_fit and grid_widen (csrc/lo_grid_geom.h), the point grid's geometry, on the host alone.

A stand-alone C++ program includes the header (no HIP) and answers one query per input line; the expected values come
from a numpy model here -- float32 division and np.floor, the header's own statement of a coordinate's cell -- and,
where the issue fixes the answer, from the literal figures.  Floats cross the pipe as their uint32 bits.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_odometry_amd", "csrc")
K_MAX_CELLS = 1 << 26
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

SOURCE = r"""
#include "lo_grid_geom.h"

#include <cstdio>
#include <cstring>

static float f32(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

int main() {
    static_assert(lo::kKdMaxCells == (size_t(1) << 26), "kKdMaxCells");
    char what[8];
    while (std::scanf("%7s", what) == 1) {
        if (what[0] == 'f') {          // fit m h b0 .. b5
            unsigned long long m;
            unsigned u[7];
            if (std::scanf("%llu %u %u %u %u %u %u %u", &m, &u[0], &u[1], &u[2], &u[3], &u[4], &u[5], &u[6]) != 8) return 2;
            float h = f32(u[0]), b[6];
            for (int a = 0; a < 6; ++a) b[a] = f32(u[1 + a]);
            int org[3] = {7, 7, 7}, dim[3] = {7, 7, 7};
            const size_t ncell = lo::grid_fit(b, static_cast<size_t>(m), h, org, dim);
            std::printf("%u %d %d %d %d %d %d %llu\n", bits(h), org[0], org[1], org[2], dim[0], dim[1], dim[2],
                        static_cast<unsigned long long>(ncell));
        } else {                        // widen min_per_cell grow m occupied
            int mpc, grow;
            unsigned long long m, occ;
            if (std::scanf("%d %d %llu %llu", &mpc, &grow, &m, &occ) != 4) return 2;
            std::printf("%d\n", lo::grid_widen(mpc, grow, static_cast<size_t>(m), static_cast<size_t>(occ)) ? 1 : 0);
        }
    }
    return 0;
}
"""


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def model_fit(bounds, m, h):
    """grid_fit in numpy: (h, org, dim, ncell)."""
    h = np.float32(h)
    b = np.asarray(bounds, np.float32)
    while True:
        if m:
            lo = [int(np.floor(b[a] / h)) for a in range(3)]
            hi = [int(np.floor(b[3 + a] / h)) for a in range(3)]
        else:
            lo, hi = [0, 0, 0], [0, 0, 0]
        ok, ncell = True, 1
        for a in range(3):
            d = hi[a] - lo[a] + 1
            if d > K_MAX_CELLS or lo[a] < -(-I32_MIN // 2) or hi[a] > I32_MAX // 2:
                ok = False
                break
            ncell *= d
            if ncell > K_MAX_CELLS:
                ok = False
                break
        if ok:
            return h, lo, [hi[a] - lo[a] + 1 for a in range(3)], ncell
        h = np.float32(h * np.float32(2.0))


def model_widen(mpc, grow, m, occupied):
    return mpc > 0 and grow < 3 and m >= 64 and occupied * mpc > m


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    d = tmp_path_factory.mktemp("grid_geom")
    src = d / "grid_geom_test.cpp"
    src.write_text(SOURCE)
    exe = d / "grid_geom_test"
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        out = [tuple(int(x) for x in ln.split()) for ln in r.stdout.strip().splitlines()]
        assert len(out) == len(lines)
        return out
    return run


def _fit_line(m, h, bounds):
    return "fit %d %d " % (m, _bits(h)) + " ".join(str(_bits(x)) for x in bounds)


def _want(m, h, bounds):
    h, org, dim, ncell = model_fit(bounds, m, h)
    return (_bits(h), *org, *dim, ncell)


# (name, m, starting h, bounds, the literal answer where the case has one: (h, org, dim))
FIT_CASES = [
    ("empty", 0, 1.0, [np.inf] * 3 + [-np.inf] * 3, (1.0, [0, 0, 0], [1, 1, 1])),          # h = 2 x voxel 0.5
    ("empty_garbage_bounds", 0, 0.6, [5.0, -3.0, 1e9, 7.0, 2.0, 2e9], (0.6, [0, 0, 0], [1, 1, 1])),
    ("one_point", 1, 1.0, [1.3, -2.7, 0.1, 1.3, -2.7, 0.1], (1.0, [1, -3, 0], [1, 1, 1])),
    ("floor_not_truncation", 2, 1.0, [-0.25] * 3 + [0.25] * 3, (1.0, [-1, -1, -1], [2, 2, 2])),
    ("cube_500m_doubles_once", 300, 1.0, [-249.75] * 3 + [249.75] * 3, (2.0, [-125] * 3, [250] * 3)),
    ("cube_501_cells_per_axis", 300, 1.0, [-250.0] * 3 + [250.0] * 3, (2.0, [-125] * 3, [251] * 3)),
    ("one_long_axis", 2, 1.0, [0.0, 0.0, 0.0, 1e8, 0.0, 0.0], (2.0, [0, 0, 0], [50000001, 1, 1])),
    ("cell_beyond_int32_half", 1, 1.0, [3e9, 0.0, 0.0, 3e9, 0.0, 0.0], (4.0, [750000000, 0, 0], [1, 1, 1])),
    ("negative_cell_beyond_int32_half", 1, 1.0, [-3e9, 0.0, 0.0, -3e9, 0.0, 0.0], (4.0, [-750000000, 0, 0], [1, 1, 1])),
    ("product_exceeds_not_an_axis", 9, 0.6, [-300.3, -280.1, -30.3, 299.7, 319.2, 170.9], None),
    ("odd_edge", 9, 0.3, [-17.31, 2.22, -0.05, 3.07, 19.9, 4.4], None),
]


def test_grid_fit_equals_the_numpy_model(ask):
    got = ask([_fit_line(m, h, b) for _, m, h, b, _ in FIT_CASES])
    for (name, m, h, b, literal), g in zip(FIT_CASES, got):
        assert g == _want(m, h, b), name
        if literal is not None:
            lh, org, dim = literal
            assert g[:7] == (_bits(lh), *org, *dim), name
            assert g[7] == dim[0] * dim[1] * dim[2], name
        assert g[7] <= K_MAX_CELLS, name
    # the cases are what they claim: at the starting edge the 500 m cube has more than 2^26 cells, the long axis alone has
    assert 500 ** 3 > K_MAX_CELLS and 10 ** 8 + 1 > K_MAX_CELLS and 3e9 > I32_MAX // 2
    doubled = dict((c[0], g[0]) for c, g in zip(FIT_CASES, got))
    assert doubled["product_exceeds_not_an_axis"] > _bits(0.6)


def test_grid_widen(ask):
    cases = [(4, 0, 63, 63), (4, 0, 63, 16), (4, 3, 6400, 6400), (4, 4, 6400, 6400), (4, 2, 6400, 6400),
             (4, 0, 64, 16), (4, 0, 64, 17), (4, 2, 9000, 2250), (4, 2, 9000, 2251), (0, 0, 6400, 6400),
             (-1, 0, 6400, 6400), (1, 0, 6400, 6400), (2, 0, 64, 64), (4, 0, 64, 64)]
    got = ask(["widen %d %d %d %d" % c for c in cases])
    for c, (g,) in zip(cases, got):
        assert bool(g) == model_widen(*c), c
    answers = {c: bool(g) for c, (g,) in zip(cases, got)}
    assert not answers[(4, 0, 63, 63)]                      # m = 63 never widens
    assert not answers[(4, 3, 6400, 6400)] and answers[(4, 2, 6400, 6400)]      # grow = 3 never widens
    assert not answers[(4, 0, 64, 16)] and answers[(4, 0, 64, 17)]              # strict at occupied * min_per_cell == m
    assert not answers[(1, 0, 6400, 6400)]                  # occupied <= m: one point per cell is always enough
