// lo_grid_geom.h — the geometry of the KDTree variant's point grid, from numbers alone: a coordinate's cell, the grid
// that holds a set of points (grid_fit) and the loop path's occupancy rule (grid_widen).  No HIP here and no context:
// the host builder and both device forms (lo_grid.hip) call these, and tests/test_grid_geom.py runs them on a CPU.
// VoxelMap::RebuildKdTree (VoxelMap.cpp:420-438) equivalent: a dense uniform grid (cell = 2 x voxel, doubled until it
// fits kKdMaxCells) over the L0 centroids in GetPointCloud order; points sorted by cell (x fastest), index order inside
// a cell; start[cell] = first point, start[ncell] = m.
#pragma once
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace lo {
constexpr size_t kKdMaxCells = size_t(1) << 26;

// the cell of a coordinate: floor(v / h) in fp32, one statement for the host and (under HIP) the kernels
#if defined(__HIP__)
__host__ __device__
#endif
inline int64_t grid_cell(float v, float h) { return static_cast<int64_t>(std::floor(v / h)); }

// The grid of m points from their bounds (bounds[0..2] the minima, [3..5] the maxima; not read when m == 0, which
// gives one cell at the origin).  floor(v / h) is monotone in v, so the cells' extremes are the extremes' cells.
// h doubles until every axis lies within INT32 / 2 cells of zero and the grid fits kKdMaxCells; org / dim out;
// returns the cell count.
inline size_t grid_fit(const float* bounds, size_t m, float& h, int org[3], int dim[3]) {
    for (;;) {
        int64_t lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
            lo[a] = m ? grid_cell(bounds[a], h) : 0;
            hi[a] = m ? grid_cell(bounds[3 + a], h) : 0;
        }
        size_t ncell = 1;
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            const int64_t d = hi[a] - lo[a] + 1;
            if (d > static_cast<int64_t>(kKdMaxCells) || lo[a] < INT32_MIN / 2 || hi[a] > INT32_MAX / 2) { ok = false; break; }
            ncell *= static_cast<size_t>(d);
            if (ncell > kKdMaxCells) { ok = false; break; }
        }
        if (ok) {
            for (int a = 0; a < 3; ++a) { org[a] = static_cast<int>(lo[a]); dim[a] = static_cast<int>(hi[a] - lo[a] + 1); }
            return ncell;
        }
        h *= 2.0f;
    }
}

// The occupancy rule (min_per_cell > 0: the loop-closure ICP's matched keyframe cloud): after `grow` doublings, does
// the cell edge double once more?  While the occupied cells hold fewer than min_per_cell points on average, up to 3
// times -- a voxel-filtered, strided keyframe cloud is sparse at 2 x voxel_size, so most queries would need the outer
// shells or the brute-force fallback.  The kNN result does not depend on the edge (every answer is certified against
// the scanned cube); only the work per query does.  occupied <= m, so grid_widen(.., m, m) tells whether any count
// could still ask (a device builder then spends the readback of the count, or does not).
inline bool grid_widen(int min_per_cell, int grow, size_t m, size_t occupied) {
    return min_per_cell > 0 && grow < 3 && m >= 64 && occupied * static_cast<size_t>(min_per_cell) > m;
}
}  // namespace lo
