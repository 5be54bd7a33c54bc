// lo_grid.hip — the KDTree variant's point grid: built on the host (grid_build, all_pairs_upload; lo_map_set_points)
// or on the device by one builder with two shells (the k_grid_* kernels: grid_from_device for one context -- a device
// map's centroids through ctx_grid_from_device, the loop-closure ICP's device-resident matched cloud through
// loop_map_from_device -- and batch_grids_from_device for all active jobs of a KDTree batch, lo_batch_sync_points).
// The geometry all three share is lo_grid_geom.h.
#include "lo_ctx_def.h"
#include "lo_grid_geom.h"

namespace lo {
// The host builder (lo_grid_geom.h has the layout and the geometry).
// with_order: also the reference kd-tree's visit order (the tie-break of equal distances); without it the kNN
// kernels flag a deciding tie in DevState::kd_tie instead of ranking it (the loop-closure ICP then rebuilds with it).
// min_per_cell > 0 (the loop-closure ICP's matched keyframe cloud): the occupancy rule, grid_widen.
int grid_build(lo_ctx* c, PointGrid& G, const float* xyz, size_t m, bool with_order, int min_per_cell) {
    if (m > 0 && !xyz) { c->err = "null points"; return LO_ERR_ARG; }
    if (m > static_cast<size_t>(INT32_MAX / 2)) { c->err = "too many map points"; return LO_ERR_CAPACITY; }
    for (size_t i = 0; i < 3 * m; ++i)
        if (!std::isfinite(xyz[i])) { c->err = "non-finite map point"; return LO_ERR_ARG; }
    // the reference kd-tree's visit order over the same cloud (equal-distance neighbours are ranked by it): built
    // on a second host thread while this one builds the grid (nanoflann's partition passes are branch-bound,
    // ~0.3 ms for a 3.6k-point keyframe cloud, as the reference's own buildIndex per loop-closure call)
    std::vector<KdNode> nodes;
    std::vector<uint32_t> vpos;
    std::thread order_thread([&] { if (with_order) KdOrderBuilder(xyz, m).build(nodes, vpos); });
    struct Joiner { std::thread& t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{order_thread};
    float bounds[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (size_t i = 0; i < m; ++i)
        for (int a = 0; a < 3; ++a) {
            bounds[a] = std::min(bounds[a], xyz[3 * i + a]);
            bounds[3 + a] = std::max(bounds[3 + a], xyz[3 * i + a]);
        }
    float h = 2.0f * c->cfg.voxel_size;
    int org[3] = {0, 0, 0}, dim[3] = {1, 1, 1};
    std::vector<uint32_t> start, lin(m);
    size_t ncell = 1;
    for (int grow = 0;; ++grow) {
        ncell = grid_fit(bounds, m, h, org, dim);
        start.assign(ncell + 1, 0);
        size_t occupied = 0;
        for (size_t i = 0; i < m; ++i) {
            const int64_t x = grid_cell(xyz[3 * i], h) - org[0], y = grid_cell(xyz[3 * i + 1], h) - org[1],
                          z = grid_cell(xyz[3 * i + 2], h) - org[2];
            lin[i] = static_cast<uint32_t>((static_cast<size_t>(z) * dim[1] + y) * dim[0] + x);
            occupied += start[lin[i] + 1]++ == 0;
        }
        if (!grid_widen(min_per_cell, grow, m, occupied)) break;
        h *= 2.0f;
    }
    for (size_t k = 0; k < ncell; ++k) start[k + 1] += start[k];
    std::vector<float4> pts(std::max<size_t>(m, 1));
    std::vector<uint32_t> fill(start.begin(), start.end() - 1);
    for (size_t i = 0; i < m; ++i) {                     // stable: index order inside a cell
        float4 v;
        v.x = xyz[3 * i]; v.y = xyz[3 * i + 1]; v.z = xyz[3 * i + 2];
        int32_t id = static_cast<int32_t>(i);
        std::memcpy(&v.w, &id, sizeof(float));
        pts[fill[lin[i]]++] = v;
    }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    LO_HIP(c, G.d_pts.reserve(pts.size()));
    LO_HIP(c, G.d_start.reserve(start.size()));
    order_thread.join();
    if (nodes.empty()) nodes.push_back(KdNode{-1, -1, 0, 0, 0.0f, 0.0f});
    if (vpos.empty()) vpos.push_back(0);
    LO_HIP(c, G.d_vpos.reserve(vpos.size()));
    LO_HIP(c, G.d_nodes.reserve(nodes.size()));
    // one pinned staging buffer, four async copies on the context stream (the kernels that read the grid follow
    // in stream order; the next grid_build's stream sync retires the copies before the buffer is refilled)
    const size_t b_pts = pts.size() * sizeof(float4), b_start = start.size() * sizeof(uint32_t);
    const size_t b_vpos = vpos.size() * sizeof(uint32_t), b_nodes = nodes.size() * sizeof(KdNode);
    const size_t total = b_pts + b_start + b_vpos + b_nodes;
    if (total > G.h_stage.capacity()) LO_HIP(c, G.h_stage.reserve(2 * total));
    char* hs = static_cast<char*>(G.h_stage.get());
    std::memcpy(hs, pts.data(), b_pts);
    std::memcpy(hs + b_pts, start.data(), b_start);
    std::memcpy(hs + b_pts + b_start, vpos.data(), b_vpos);
    std::memcpy(hs + b_pts + b_start + b_vpos, nodes.data(), b_nodes);
    LO_HIP(c, hipMemcpyAsync(G.d_pts, hs, b_pts, hipMemcpyHostToDevice, c->stream));
    LO_HIP(c, hipMemcpyAsync(G.d_start, hs + b_pts, b_start, hipMemcpyHostToDevice, c->stream));
    LO_HIP(c, hipMemcpyAsync(G.d_vpos, hs + b_pts + b_start, b_vpos, hipMemcpyHostToDevice, c->stream));
    LO_HIP(c, hipMemcpyAsync(G.d_nodes, hs + b_pts + b_start + b_vpos, b_nodes, hipMemcpyHostToDevice, c->stream));
    G.m = static_cast<int>(m);
    G.has_order = with_order;
    G.all = false;
    G.h = h;
    for (int a = 0; a < 3; ++a) { G.org[a] = org[a]; G.dim[a] = dim[a]; }
    return LO_OK;
}

// A small point set (<= kKnnAllMax) for the all-pairs kernels (k_knn_all, k_inlier_all): the points in index order as
// float4 (x, y, z, index), no cells and no visit order; with q (nq points) also the query cloud into c->d_pts, both
// through the grid's pinned staging buffer (two async copies, no pageable-memory copy).
int all_pairs_upload(lo_ctx* c, PointGrid& G, const float* xyz, size_t m, const float* q, size_t nq) {
    if (m > static_cast<size_t>(kKnnAllMax)) { c->err = "all_pairs_upload: too many points"; return LO_ERR_CAPACITY; }
    if (m > 0 && !xyz) { c->err = "null points"; return LO_ERR_ARG; }
    for (size_t i = 0; i < 3 * m; ++i)
        if (!std::isfinite(xyz[i])) { c->err = "non-finite map point"; return LO_ERR_ARG; }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipStreamSynchronize(c->stream));          // the staging buffer's previous copy has retired
    const size_t mm = std::max<size_t>(m, 1), bytes = mm * sizeof(float4) + nq * 3 * sizeof(float);
    LO_HIP(c, G.d_pts.reserve(mm));
    if (bytes > G.h_stage.capacity()) LO_HIP(c, G.h_stage.reserve(2 * bytes));
    float4* hs = static_cast<float4*>(G.h_stage.get());
    for (size_t i = 0; i < m; ++i) {
        int32_t id = static_cast<int32_t>(i);
        float w;
        std::memcpy(&w, &id, sizeof(float));
        hs[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], w);
    }
    if (m > 0) LO_HIP(c, hipMemcpyAsync(G.d_pts, hs, m * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if (nq > 0) {
        float* hq = reinterpret_cast<float*>(hs + mm);
        std::memcpy(hq, q, nq * 3 * sizeof(float));
        LO_HIP(c, hipMemcpyAsync(c->d_pts, hq, nq * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    G.m = static_cast<int>(m);
    G.has_order = false;
    G.all = true;
    return LO_OK;
}

// ---- the same grid built on the device: one builder, a solo and a batch shell around every kernel body ----
// grid_from_device builds one grid on the context stream, its job's descriptor (GridJob) passed to the k_grid_*_1
// shells by value; batch_grids_from_device builds the grids of all active jobs on the batch stream, the k_grid_*_b
// shells reading descriptor blockIdx.y of a device array.  Either way: a bounds launch, seven words per job read back
// with the call's one synchronise, the geometry on the host (grid_fit), and seven launches (grid_emit):
//   clear       counts[0 .. ncell] = 0
//   keys        every point's cell, and its arrival number in the cell (the cell count's atomicAdd)
//   scan_sum    exclusive scan of counts into start, three launches: each workgroup sums its chunk of the job's
//   scan_top      ncell + 1 counts, one workgroup per job scans the chunk sums, each workgroup scans its chunk from
//   scan_write    its offset
//   claim       slots[start[cell] + arrival] = point index (arrival order inside a cell: arbitrary)
//   place       a point's rank in its cell = the cell's slot entries with a smaller index; the point goes to
//               start[cell] + rank -- index order inside a cell, whatever order the atomics landed in
// Every phase reads what an earlier launch wrote: no kernel fills through atomics and reads the result itself.  Every
// kernel clamps the device count to the array's capacity and to the host's copy that sized the buffers (grid_job_m):
// the host reports a corrupt or overflowing count (the bounds' seventh word) and nothing reads or writes past an array.
struct GridGeom {
    float h;
    int org[3], dim[3];
};
// point i's cell in the grid, x fastest (grid_build's lin[i])
__device__ __forceinline__ uint32_t grid_lin(const float* __restrict__ xyz, int i, const GridGeom& g) {
    const long long x = grid_cell(xyz[3 * i], g.h) - g.org[0], y = grid_cell(xyz[3 * i + 1], g.h) - g.org[1],
                    z = grid_cell(xyz[3 * i + 2], g.h) - g.org[2];
    return static_cast<uint32_t>((static_cast<unsigned long long>(z) * g.dim[1] + y) * g.dim[0] + x);
}
struct GridJob {
    const float* xyz;                // the points, 3 floats each
    const int* d_count;              //   *d_count of them on the device (clamped to cap and to m)
    int cap;
    int m;                           // the host's copy of the count (what the buffers below are sized for)
    GridGeom g;
    uint32_t n;                      // ncell + 1: the words of counts and start
    uint32_t chunk;                  // scan: words per workgroup (a multiple of kGridScanBlock)
    uint32_t* counts;                // [n]
    uint32_t* start;                 // [n]
    uint32_t* keys;                  // [m] a point's cell (kGridNoCell: none)
    uint32_t* rank;                  // [m] its arrival number in the cell
    uint32_t* slots;                 // [m] point indices grouped by cell
    uint32_t* bsum;                  // [gridDim.x of the scan] chunk sums, then their exclusive scan
    uint32_t* occ;                   // nullable: counts the occupied cells (the occupancy rule; zeroed by the host)
    float4* pts;                     // [m]
};
constexpr int kGridScanBlock = 256;
constexpr int kGridScanMaxBlocks = 1024;         // chunk sums per job: what scan_top's one workgroup scans
constexpr int kGridBatchWGs = 65536;             // workgroups per launch over all jobs
constexpr uint32_t kGridNoCell = 0xFFFFFFFFu;
__device__ __forceinline__ int grid_job_m(const GridJob& J) { return min(min(max(*J.d_count, 0), J.cap), J.m); }
// The bodies: blk of nblk workgroups work on job J.  Bounds, by one 1024-thread workgroup: out[0..2] the minima,
// [3..5] the maxima, [6] the raw count.
__device__ __forceinline__ void grid_bounds_body(const GridJob& J, float* __restrict__ out) {
    __shared__ float s[6][16];
    const float* __restrict__ xyz = J.xyz;
    const int m_raw = *J.d_count, m = min(max(m_raw, 0), J.cap), tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < m; i += 1024)
        for (int a = 0; a < 3; ++a) { const float v = xyz[3 * i + a]; lo[a] = fminf(lo[a], v); hi[a] = fmaxf(hi[a], v); }
    for (int o = 32; o > 0; o >>= 1)
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
    if (lane == 0) for (int a = 0; a < 3; ++a) { s[a][wid] = lo[a]; s[3 + a][wid] = hi[a]; }
    __syncthreads();
    if (tid < 6) {
        float r = s[tid][0];
        for (int w = 1; w < 16; ++w) r = tid < 3 ? fminf(r, s[tid][w]) : fmaxf(r, s[tid][w]);
        out[tid] = r;
    }
    if (tid == 0) out[6] = __int_as_float(m_raw);
}
__device__ __forceinline__ void grid_clear_body(const GridJob& J, uint32_t blk, uint32_t nblk) {
    const uint32_t n4 = J.n >> 2, step = nblk * 256u;
    uint4* c4 = reinterpret_cast<uint4*>(J.counts);      // (a hipMalloc'ed array: 16-byte aligned)
    for (uint32_t k = blk * 256u + threadIdx.x; k < n4; k += step) c4[k] = make_uint4(0u, 0u, 0u, 0u);
    if (blk == 0 && threadIdx.x < (J.n & 3u)) J.counts[4u * n4 + threadIdx.x] = 0u;
}
// A cell outside the grid cannot come from the points the bounds were taken of; such a point (a non-finite
// coordinate, say) is left out instead of counted.
__device__ __forceinline__ void grid_keys_body(const GridJob& J, int blk, int nblk) {
    const int m = grid_job_m(J), step = nblk * 256;
    for (int i = blk * 256 + threadIdx.x; i < m; i += step) {
        uint32_t lin = grid_lin(J.xyz, i, J.g), r = 0u;
        if (lin < J.n - 1u) {
            r = atomicAdd(&J.counts[lin], 1u);
            if (r == 0u && J.occ) atomicAdd(J.occ, 1u);      // grid_build's `occupied`
        } else {
            lin = kGridNoCell;
        }
        J.keys[i] = lin;
        J.rank[i] = r;
    }
}
// exclusive scan of one value per thread over a 64 * NW-thread workgroup; total: the workgroup's sum
template <int NW>
__device__ __forceinline__ uint32_t grid_block_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t off = 0u, tot = 0u;
    for (int k = 0; k < NW; ++k) {
        const uint32_t t = s_w[k];
        if (k < w) off += t;
        tot += t;
    }
    __syncthreads();                                     // s_w is free for the next call
    total = tot;
    return off + inc - v;
}
__device__ __forceinline__ void grid_scan_sum_body(const GridJob& J, uint32_t blk) {
    __shared__ uint32_t s_w[kGridScanBlock / 64];
    const uint64_t b0 = static_cast<uint64_t>(blk) * J.chunk;
    const uint32_t e0 = static_cast<uint32_t>(min(b0 + J.chunk, static_cast<uint64_t>(J.n)));
    uint32_t sum = 0u;
    for (uint64_t k = b0 + threadIdx.x; k < e0; k += kGridScanBlock) sum += J.counts[k];
    uint32_t total;
    (void)grid_block_scan<kGridScanBlock / 64>(sum, s_w, total);
    if (threadIdx.x == 0) J.bsum[blk] = total;
}
__device__ __forceinline__ void grid_scan_top_body(const GridJob& J, int nblk) {
    __shared__ uint32_t s_w[kGridScanMaxBlocks / 64];
    const int t = threadIdx.x;
    const uint32_t v = t < nblk ? J.bsum[t] : 0u;
    uint32_t total;
    const uint32_t ex = grid_block_scan<kGridScanMaxBlocks / 64>(v, s_w, total);
    if (t < nblk) J.bsum[t] = ex;
}
__device__ __forceinline__ void grid_scan_write_body(const GridJob& J, uint32_t blk) {
    __shared__ uint32_t s_w[kGridScanBlock / 64];
    const uint64_t b0 = static_cast<uint64_t>(blk) * J.chunk;
    if (b0 >= J.n) return;                               // (the whole workgroup: no barrier is skipped by a part of it)
    const uint32_t e0 = static_cast<uint32_t>(min(b0 + J.chunk, static_cast<uint64_t>(J.n)));
    uint32_t carry = J.bsum[blk];
    for (uint32_t base = static_cast<uint32_t>(b0); base < e0; base += kGridScanBlock) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t v = k < e0 ? J.counts[k] : 0u;
        uint32_t total;
        const uint32_t ex = grid_block_scan<kGridScanBlock / 64>(v, s_w, total);
        if (k < e0) J.start[k] = carry + ex;
        carry += total;
    }
}
__device__ __forceinline__ void grid_claim_body(const GridJob& J, int blk, int nblk) {
    const int m = grid_job_m(J), step = nblk * 256;
    for (int i = blk * 256 + threadIdx.x; i < m; i += step) {
        const uint32_t lin = J.keys[i];
        if (lin == kGridNoCell) continue;
        const uint32_t p = J.start[lin] + J.rank[i];
        if (p < static_cast<uint32_t>(m)) J.slots[p] = static_cast<uint32_t>(i);
    }
}
__device__ __forceinline__ void grid_place_body(const GridJob& J, int blk, int nblk) {
    const int m = grid_job_m(J), step = nblk * 256;
    for (int i = blk * 256 + threadIdx.x; i < m; i += step) {
        const uint32_t lin = J.keys[i];
        if (lin == kGridNoCell) continue;
        const uint32_t s = J.start[lin], e = min(J.start[lin + 1u], static_cast<uint32_t>(m));
        uint32_t p = s;
        for (uint32_t q = s; q < e; ++q) p += J.slots[q] < static_cast<uint32_t>(i) ? 1u : 0u;
        if (p < static_cast<uint32_t>(m))
            J.pts[p] = make_float4(J.xyz[3 * i], J.xyz[3 * i + 1], J.xyz[3 * i + 2], __int_as_float(i));
    }
}

// The shells.  _1: one job, by value; _b: blockIdx.y = active slot, its job's descriptor read from a device array.
__global__ __launch_bounds__(1024) void k_grid_bounds_1(GridJob J, float* __restrict__ out) { grid_bounds_body(J, out); }
__global__ __launch_bounds__(1024) void k_grid_bounds_b(const GridJob* __restrict__ jobs, float* __restrict__ out) {
    grid_bounds_body(jobs[blockIdx.y], out + 7 * blockIdx.y);
}
__global__ __launch_bounds__(256) void k_grid_clear_1(GridJob J) { grid_clear_body(J, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256)
void k_grid_clear_b(const GridJob* __restrict__ jobs) { grid_clear_body(jobs[blockIdx.y], blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void k_grid_keys_1(GridJob J) { grid_keys_body(J, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256)
void k_grid_keys_b(const GridJob* __restrict__ jobs) { grid_keys_body(jobs[blockIdx.y], blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(kGridScanBlock) void k_grid_scan_sum_1(GridJob J) { grid_scan_sum_body(J, blockIdx.x); }
__global__ __launch_bounds__(kGridScanBlock)
void k_grid_scan_sum_b(const GridJob* __restrict__ jobs) { grid_scan_sum_body(jobs[blockIdx.y], blockIdx.x); }
__global__ __launch_bounds__(kGridScanMaxBlocks) void k_grid_scan_top_1(GridJob J, int nblk) { grid_scan_top_body(J, nblk); }
__global__ __launch_bounds__(kGridScanMaxBlocks)
void k_grid_scan_top_b(const GridJob* __restrict__ jobs, int nblk) { grid_scan_top_body(jobs[blockIdx.y], nblk); }
__global__ __launch_bounds__(kGridScanBlock) void k_grid_scan_write_1(GridJob J) { grid_scan_write_body(J, blockIdx.x); }
__global__ __launch_bounds__(kGridScanBlock)
void k_grid_scan_write_b(const GridJob* __restrict__ jobs) { grid_scan_write_body(jobs[blockIdx.y], blockIdx.x); }
__global__ __launch_bounds__(256) void k_grid_claim_1(GridJob J) { grid_claim_body(J, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256)
void k_grid_claim_b(const GridJob* __restrict__ jobs) { grid_claim_body(jobs[blockIdx.y], blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256) void k_grid_place_1(GridJob J) { grid_place_body(J, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(256)
void k_grid_place_b(const GridJob* __restrict__ jobs) { grid_place_body(jobs[blockIdx.y], blockIdx.x, gridDim.x); }

// ---- the host side both forms share ----
// the scratch words behind the six bounds and the count (kGridWords floats), and the solo scan's chunk sums
int grid_scratch(lo_ctx* c) {
    LO_HIP(c, c->gscr.d_bounds.reserve(kGridWords));
    LO_HIP(c, c->gscr.h_bounds.reserve(kGridWords));
    LO_HIP(c, c->gscr.d_bsum.reserve(kGridScanMaxBlocks));
    return LO_OK;
}
// A buffer that has to grow takes half as much again (at most 4M elements more): a map gains cells and points with
// every keyframe, and a hipFree + hipMalloc per buffer per job per keyframe costs more than the eight launches (their
// cost rises with the number of live allocations: B = 1024 keyframes took 256 ms with exact sizes).
template <class T>
static hipError_t grid_grow(DevBuf<T>& buf, size_t need) {
    return need <= buf.capacity() ? hipSuccess : buf.reserve(need + std::min(need / 2, size_t(1) << 22));
}
// a job over a device point array whose count is on the device too; the count in its bounds readback (raw)
static GridJob grid_job_of(const float* xyz, const int* d_count, size_t cap) {
    GridJob J{};
    J.xyz = xyz;
    J.d_count = d_count;
    J.cap = static_cast<int>(std::min(cap, static_cast<size_t>(INT32_MAX)));
    return J;
}
static size_t grid_count(const float* hb) {
    int mi = 0;
    std::memcpy(&mi, &hb[6], sizeof(int));
    return static_cast<size_t>(std::max(mi, 0));
}
// Job J bound to grid G of m points in ncell cells: G's and the scratch's buffers grown where they have to (nothing in
// flight may read them), the descriptor's geometry and pointers, and G's host fields as the launches will leave it.
static hipError_t grid_job_bind(GridJob& J, PointGrid& G, DevGridScratch& W, size_t m, size_t ncell, const GridGeom& g) {
    const size_t mm = std::max<size_t>(m, 1);
    hipError_t e = grid_grow(G.d_pts, mm);
    if (e == hipSuccess) e = grid_grow(G.d_start, ncell + 1);
    if (e == hipSuccess) e = grid_grow(W.d_keys, 3 * mm);    // keys, rank, slots
    if (e == hipSuccess) e = grid_grow(W.d_counts, ncell + 1);
    if (e != hipSuccess) return e;
    J.m = G.m = static_cast<int>(m);
    J.g = g;
    J.n = static_cast<uint32_t>(ncell + 1);
    J.counts = W.d_counts;
    J.start = G.d_start;
    J.keys = W.d_keys;
    J.rank = J.keys + mm;
    J.slots = J.rank + mm;
    J.pts = G.d_pts;
    G.has_order = G.all = false;
    G.h = g.h;
    for (int a = 0; a < 3; ++a) { G.org[a] = g.org[a]; G.dim[a] = g.dim[a]; }
    return hipSuccess;
}
// One set of launches: over the batch's k descriptors on the device (d_jobs; the _b shells), or over one job by value
// (one; the _1 shells: no descriptor upload).
struct GridRun {
    hipStream_t stream;
    const GridJob* d_jobs;
    const GridJob* one;
    int k;
    unsigned pblk, cblk, nblk;       // workgroups per job: over the points, over the counts (clear), scan chunks
};
// launch sizes from the largest job (max_m points, max_n count words) under the workgroup budget; the scan's chunk
// count is common to all jobs
static GridRun grid_run(hipStream_t stream, const GridJob* d_jobs, const GridJob* one, int k, size_t max_m, size_t max_n) {
    const unsigned per_job = static_cast<unsigned>(std::max(1, kGridBatchWGs / k));
    auto blocks = [&](size_t items, size_t per) {
        return static_cast<unsigned>(std::max<size_t>(1, std::min<size_t>(per_job, (items + per - 1) / per)));
    };
    return GridRun{stream, d_jobs, one, k, blocks(max_m, 256), blocks(max_n, 16 * 256),
                   std::min(blocks(max_n, 8 * kGridScanBlock), static_cast<unsigned>(kGridScanMaxBlocks))};
}
// a job's chunk of the scan's nblk, and where its chunk sums go
static void grid_job_scan(GridJob& J, unsigned nblk, uint32_t* bsum) {
    const uint32_t per = (J.n + nblk - 1) / nblk;
    J.chunk = (per + kGridScanBlock - 1) / kGridScanBlock * kGridScanBlock;
    J.bsum = bsum;
}
template <class KB, class K1, class... A>
static void grid_launch(const GridRun& R, KB kb, K1 k1, unsigned blocks, unsigned threads, A... a) {
    if (R.d_jobs) hipLaunchKernelGGL(kb, dim3(blocks, R.k), dim3(threads), 0, R.stream, R.d_jobs, a...);
    else hipLaunchKernelGGL(k1, dim3(blocks), dim3(threads), 0, R.stream, *R.one, a...);
}
// The launch list.  kGridBin alone is what the occupancy rule repeats per cell edge it tries.
enum { kGridBin = 1, kGridOrder = 2 };
static void grid_emit(const GridRun& R, int phases) {
    if (phases & kGridBin) {
        grid_launch(R, k_grid_clear_b, k_grid_clear_1, R.cblk, 256);
        grid_launch(R, k_grid_keys_b, k_grid_keys_1, R.pblk, 256);
    }
    if (phases & kGridOrder) {
        grid_launch(R, k_grid_scan_sum_b, k_grid_scan_sum_1, R.nblk, kGridScanBlock);
        grid_launch(R, k_grid_scan_top_b, k_grid_scan_top_1, 1, kGridScanMaxBlocks, static_cast<int>(R.nblk));
        grid_launch(R, k_grid_scan_write_b, k_grid_scan_write_1, R.nblk, kGridScanBlock);
        grid_launch(R, k_grid_claim_b, k_grid_claim_1, R.pblk, 256);
        grid_launch(R, k_grid_place_b, k_grid_place_1, R.pblk, 256);
    }
}

// grid_build's grid of a device point array, into G, on the context stream.  min_per_cell as grid_build: while the
// rule can still ask (grid_widen), keys counts the occupied cells and the count is one more 4-byte readback.
int grid_from_device(lo_ctx* c, PointGrid& G, const float* d_xyz, const int* d_count, size_t cap, int min_per_cell) {
    DevGridScratch& S = c->gscr;
    int rc = grid_scratch(c);
    if (rc != LO_OK) return rc;
    GridJob J = grid_job_of(d_xyz, d_count, cap);
    hipLaunchKernelGGL(k_grid_bounds_1, dim3(1), dim3(1024), 0, c->stream, J, S.d_bounds.get());
    LO_HIP(c, hipMemcpyAsync(S.h_bounds, S.d_bounds, 7 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    const size_t m = grid_count(S.h_bounds);
    if (m > cap) { c->err = "ctx_grid_from_device: count beyond the array"; return LO_ERR_CAPACITY; }
    uint32_t* d_occ = reinterpret_cast<uint32_t*>(S.d_bounds.get()) + kGridOcc;
    GridGeom g{2.0f * c->cfg.voxel_size, {0, 0, 0}, {1, 1, 1}};
    GridRun R{};
    for (int grow = 0;; ++grow) {
        const size_t ncell = grid_fit(S.h_bounds, m, g.h, g.org, g.dim);
        LO_HIP(c, grid_job_bind(J, G, S, m, ncell, g));
        R = grid_run(c->stream, nullptr, &J, 1, std::max<size_t>(m, 1), ncell + 1);
        grid_job_scan(J, R.nblk, S.d_bsum);
        const bool rule = grid_widen(min_per_cell, grow, m, m);
        J.occ = rule ? d_occ : nullptr;
        if (rule) LO_HIP(c, hipMemsetAsync(d_occ, 0, sizeof(uint32_t), c->stream));
        grid_emit(R, kGridBin);
        if (!rule) break;
        LO_HIP(c, hipMemcpyAsync(S.h_bounds + kGridOcc, d_occ, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        uint32_t occupied = 0;
        std::memcpy(&occupied, &S.h_bounds[kGridOcc], sizeof(uint32_t));
        if (!grid_widen(min_per_cell, grow, m, occupied)) break;
        g.h *= 2.0f;
    }
    grid_emit(R, kGridOrder);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}

// A device cloud (sensor frame, AoS float3) in the world: transform_pt, util::transform_point_cloud's fp32 order, as
// lo::transform_points on the host.  ALL: float4 (x, y, z, index) in index order (all_pairs_upload's layout); else
// float3.  words: the grid scratch -- [kGridCount] receives n (the device count grid_from_device reads), [kGridBad]
// is raised by a non-finite world point (grid_build's LO_ERR_ARG).
template <bool ALL>
__global__ __launch_bounds__(kBlock) void k_cloud_world(const float* __restrict__ in, int n, Pose12 T,
                                                        float* __restrict__ out3, float4* __restrict__ out4,
                                                        uint32_t* __restrict__ words) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) words[kGridCount] = static_cast<uint32_t>(n);
    if (i >= n) return;
    float wx, wy, wz;
    transform_pt(T.v, in[3 * static_cast<size_t>(i)], in[3 * static_cast<size_t>(i) + 1], in[3 * static_cast<size_t>(i) + 2],
                 wx, wy, wz);
    if (!(isfinite(wx) && isfinite(wy) && isfinite(wz))) atomicOr(&words[kGridBad], 1u);
    if (ALL) {
        out4[i] = make_float4(wx, wy, wz, __int_as_float(i));
    } else {
        out3[3 * static_cast<size_t>(i)] = wx;
        out3[3 * static_cast<size_t>(i) + 1] = wy;
        out3[3 * static_cast<size_t>(i) + 2] = wz;
    }
}

// The loop-closure ICP's local map from a device cloud: d_xyz (m points, sensor frame) at pose T, into G -- the
// all-pairs layout up to kKnnAllMax points, else grid_build's grid (no visit order either way), as all_pairs_upload /
// grid_build give for the same cloud transformed on the host.
int loop_map_from_device(lo_ctx* c, PointGrid& G, const float* d_xyz, size_t m, const float T[12], int min_per_cell) {
    if (m > 0 && !d_xyz) { c->err = "null points"; return LO_ERR_ARG; }
    if (m > static_cast<size_t>(INT32_MAX / 2)) { c->err = "too many map points"; return LO_ERR_CAPACITY; }
    int rc = grid_scratch(c);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipStreamSynchronize(c->stream));          // nothing in flight reads the buffers grown below
    const bool all = m <= static_cast<size_t>(kKnnAllMax);
    const size_t mm = std::max<size_t>(m, 1);
    if (all) LO_HIP(c, G.d_pts.reserve(mm));
    else LO_HIP(c, c->d_lworld.reserve(3 * mm));
    uint32_t* words = reinterpret_cast<uint32_t*>(c->gscr.d_bounds.get());
    LO_HIP(c, hipMemsetAsync(words + kGridBad, 0, sizeof(uint32_t), c->stream));
    Pose12 P;
    std::memcpy(P.v, T, sizeof(P.v));
    const dim3 grid(static_cast<unsigned>((mm + kBlock - 1) / kBlock)), blk(kBlock);
    if (all) hipLaunchKernelGGL(k_cloud_world<true>, grid, blk, 0, c->stream, d_xyz, static_cast<int>(m), P, nullptr, G.d_pts.get(), words);
    else hipLaunchKernelGGL(k_cloud_world<false>, grid, blk, 0, c->stream, d_xyz, static_cast<int>(m), P, c->d_lworld.get(), nullptr, words);
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipMemcpyAsync(c->gscr.h_bounds + kGridBad, words + kGridBad, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t bad = 0;
    std::memcpy(&bad, &c->gscr.h_bounds[kGridBad], sizeof(uint32_t));
    if (bad) { c->err = "non-finite map point"; return LO_ERR_ARG; }
    if (all) {
        G.m = static_cast<int>(m);
        G.has_order = false;
        G.all = true;
        return LO_OK;
    }
    return grid_from_device(c, G, c->d_lworld, reinterpret_cast<const int*>(words + kGridCount), m, min_per_cell);
}

int ctx_grid_from_device(lo_ctx* c, const float* d_xyz, const int* d_count, size_t cap) {
    if (!c || !d_xyz || !d_count) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (!c->kd) { c->err = "ctx_grid_from_device: a KDTree-mode context"; return LO_ERR_STATE; }
    LO_HIP(c, hipSetDevice(c->device));
    const int rc = grid_from_device(c, c->grid, d_xyz, d_count, cap, 0);
    if (rc == LO_OK) c->grid_dev = true;
    return rc;
}

// ---- the grids of a batch (lo_batch_sync_points): ctx_grid_from_device for all active jobs in one set of launches ----
// Two host-to-device copies (the jobs' point arrays before the bounds, the grids' descriptors after the readback), one
// device-to-host copy of seven words per job with the call's one synchronise, and eight launches.
struct BatchGrids {
    int device = 0;
    DevBuf<GridJob> d_jobs;
    PinnedBuf<GridJob> h_jobs;
    DevBuf<float> d_bounds;          // 7 words per active slot
    PinnedBuf<float> h_bounds;
    DevBuf<uint32_t> d_bsum;         // the scan's chunk sums of all slots (at most kGridBatchWGs workgroups scan)
    hipEvent_t ev_up = nullptr;      // the last call's second upload has read h_jobs
    bool up_pending = false;
};
static void bg_release(void* p) {
    BatchGrids* S = static_cast<BatchGrids*>(p);
    (void)hipSetDevice(S->device);
    if (S->ev_up) (void)hipEventDestroy(S->ev_up);
    delete S;
}

int batch_grids_from_device(lo_batch* b, const GridSrc* src, int n, std::string* err, int* bad_job) {
    struct Err { std::string err, *out; ~Err() { if (out) *out = err; } } err_{{}, err}, *e = &err_;   // LO_HIP's handle
    if (bad_job) *bad_job = -1;
    const BatchView V = batch_view(b);
    LO_HIP(e, hipSetDevice(V.device));
    void** slot = batch_grid_state(b, bg_release);
    if (!*slot) {
        BatchGrids* S = new BatchGrids();
        S->device = V.device;
        *slot = S;                                           // owned by the batch from here on
    }
    BatchGrids* S = static_cast<BatchGrids*>(*slot);
    const size_t B = static_cast<size_t>(V.count);
    if (!S->ev_up) LO_HIP(e, hipEventCreateWithFlags(&S->ev_up, hipEventDisableTiming));
    LO_HIP(e, S->d_jobs.reserve(B));
    LO_HIP(e, S->h_jobs.reserve(B));
    LO_HIP(e, S->d_bounds.reserve(7 * B));
    LO_HIP(e, S->h_bounds.reserve(7 * B));
    if (S->up_pending) {                                     // the previous call's upload still reads h_jobs
        LO_HIP(e, hipEventSynchronize(S->ev_up));
        S->up_pending = false;
    }
    if (n <= 0) return LO_OK;
    hipStream_t bs = static_cast<hipStream_t>(V.stream);
    for (int a = 0; a < n; ++a) S->h_jobs[a] = grid_job_of(src[a].xyz, src[a].count, src[a].cap);
    LO_HIP(e, hipMemcpyAsync(S->d_jobs, S->h_jobs, sizeof(GridJob) * n, hipMemcpyHostToDevice, bs));
    hipLaunchKernelGGL(k_grid_bounds_b, dim3(1, n), dim3(1024), 0, bs, S->d_jobs.get(), S->d_bounds.get());
    LO_HIP(e, hipGetLastError());
    LO_HIP(e, hipMemcpyAsync(S->h_bounds, S->d_bounds, sizeof(float) * 7 * n, hipMemcpyDeviceToHost, bs));
    LO_HIP(e, hipStreamSynchronize(bs));
    // nothing is in flight on the batch stream now (and the contexts are idle, as for every batch call): each job's
    // geometry, and its buffers grown where they have to
    int rc = LO_OK, k = 0;
    size_t max_n = 1, max_m = 1;
    for (int a = 0; a < n; ++a) {
        lo_ctx* c = src[a].c;
        const float* hb = S->h_bounds + 7 * a;
        const size_t m = grid_count(hb);
        if (m > src[a].cap) {
            c->err = "ctx_grid_from_device: count beyond the array";
            if (rc == LO_OK) {
                rc = LO_ERR_CAPACITY;
                if (bad_job) *bad_job = src[a].job;
                e->err = "job " + std::to_string(src[a].job) + ": " + c->err;
            }
            continue;
        }
        GridGeom g{2.0f * c->cfg.voxel_size, {0, 0, 0}, {1, 1, 1}};
        const size_t ncell = grid_fit(hb, m, g.h, g.org, g.dim);
        GridJob J = S->h_jobs[a];
        LO_HIP(e, grid_job_bind(J, c->grid, c->gscr, m, ncell, g));
        S->h_jobs[k++] = J;                                  // (k <= a: entry a has been read)
        max_n = std::max(max_n, ncell + 1);
        max_m = std::max(max_m, m);
        c->grid_dev = true;
    }
    if (k == 0) return rc;
    const GridRun R = grid_run(bs, S->d_jobs, nullptr, k, max_m, max_n);
    LO_HIP(e, S->d_bsum.reserve(std::max(static_cast<size_t>(kGridBatchWGs), B)));      // >= nblk * k
    for (int a = 0; a < k; ++a) grid_job_scan(S->h_jobs[a], R.nblk, S->d_bsum + static_cast<size_t>(a) * R.nblk);
    LO_HIP(e, hipMemcpyAsync(S->d_jobs, S->h_jobs, sizeof(GridJob) * k, hipMemcpyHostToDevice, bs));
    LO_HIP(e, hipEventRecord(S->ev_up, bs));
    S->up_pending = true;
    grid_emit(R, kGridBin | kGridOrder);
    LO_HIP(e, hipGetLastError());
    return rc;
}

// ---- the loop grids of a batch (lo_batch_optimize_loop_dev): loop_map_from_device's grid build for all cell-grid jobs
// of a call, on the batch stream with the batch's descriptors and the same kernels.  Each job's world cloud (float3,
// its count in a device word) goes into its context's lgrid under the loop path's occupancy rule: every round bins the
// jobs that are still asking at their current cell edge (clear + keys, the occupied cells counted), one readback of
// the counts and one synchronise for all of them, and grid_widen decides per job -- at most four rounds whatever the
// number of jobs.  Then the order phases once, over every job at its final geometry.  No visit order is built.
// h_bad (nullable): n_bad host words the caller's copy on the batch stream fills before the bounds readback; a
// non-zero word ends the call with LO_ERR_ARG (*bad_slot: its index) before any grid is touched.
int batch_loop_grids_from_device(lo_batch* b, const LoopGridSrc* src, int n, int min_per_cell, const uint32_t* h_bad,
                                 int n_bad, int* bad_slot, std::string* err) {
    struct Err { std::string err, *out; ~Err() { if (out) *out = err; } } err_{{}, err}, *e = &err_;   // LO_HIP's handle
    if (bad_slot) *bad_slot = -1;
    const BatchView V = batch_view(b);
    LO_HIP(e, hipSetDevice(V.device));
    void** slot = batch_grid_state(b, bg_release);
    if (!*slot) {
        BatchGrids* S = new BatchGrids();
        S->device = V.device;
        *slot = S;                                           // owned by the batch from here on
    }
    BatchGrids* S = static_cast<BatchGrids*>(*slot);
    const size_t B = static_cast<size_t>(std::max(V.count, n));
    if (!S->ev_up) LO_HIP(e, hipEventCreateWithFlags(&S->ev_up, hipEventDisableTiming));
    LO_HIP(e, S->d_jobs.reserve(B));
    LO_HIP(e, S->h_jobs.reserve(B));
    LO_HIP(e, S->d_bounds.reserve(7 * B));
    LO_HIP(e, S->h_bounds.reserve(8 * B));                   // the bounds, then the open jobs' occupied-cell words
    hipStream_t bs = static_cast<hipStream_t>(V.stream);
    auto upload = [&](int k) -> hipError_t {                 // h_jobs[0 .. k) to the device; ev_up: the copy has read them
        hipError_t r = hipMemcpyAsync(S->d_jobs, S->h_jobs, sizeof(GridJob) * k, hipMemcpyHostToDevice, bs);
        if (r == hipSuccess) r = hipEventRecord(S->ev_up, bs);
        S->up_pending = r == hipSuccess;
        return r;
    };
    auto settle = [&]() -> hipError_t {                      // h_jobs may be rewritten
        if (!S->up_pending) return hipSuccess;
        S->up_pending = false;
        return hipEventSynchronize(S->ev_up);
    };
    LO_HIP(e, settle());
    std::vector<GridJob> fin(static_cast<size_t>(std::max(n, 0)));
    for (int a = 0; a < n; ++a) S->h_jobs[a] = fin[a] = grid_job_of(src[a].xyz, src[a].count, src[a].m);
    if (n > 0) {
        LO_HIP(e, upload(n));
        hipLaunchKernelGGL(k_grid_bounds_b, dim3(1, n), dim3(1024), 0, bs, S->d_jobs.get(), S->d_bounds.get());
        LO_HIP(e, hipGetLastError());
        LO_HIP(e, hipMemcpyAsync(S->h_bounds, S->d_bounds, sizeof(float) * 7 * n, hipMemcpyDeviceToHost, bs));
    }
    LO_HIP(e, hipStreamSynchronize(bs));
    for (int a = 0; a < n_bad; ++a)
        if (h_bad && h_bad[a]) {
            if (bad_slot) *bad_slot = a;
            e->err = "non-finite map point";
            return LO_ERR_ARG;
        }
    if (n <= 0) return LO_OK;
    std::vector<GridGeom> g(static_cast<size_t>(n));
    std::vector<char> open(static_cast<size_t>(n), 1);
    for (int a = 0; a < n; ++a) {
        g[a] = GridGeom{2.0f * src[a].c->cfg.voxel_size, {0, 0, 0}, {1, 1, 1}};
        if (grid_count(S->h_bounds + 7 * a) != src[a].m) {
            e->err = "job " + std::to_string(src[a].job) + ": loop grid: the device count is not the job's";
            return LO_ERR_STATE;
        }
    }
    uint32_t* h_occ = reinterpret_cast<uint32_t*>(S->h_bounds.get());    // (behind the 7 n bounds)
    std::vector<int> act;
    for (int grow = 0;; ++grow) {
        act.clear();
        for (int a = 0; a < n; ++a) if (open[a]) act.push_back(a);
        if (act.empty()) break;
        LO_HIP(e, settle());
        size_t max_n = 1, max_m = 1;
        bool any_rule = false;
        int k = 0;
        for (int a : act) {
            const size_t m = src[a].m;
            const size_t ncell = grid_fit(S->h_bounds + 7 * a, m, g[a].h, g[a].org, g[a].dim);
            LO_HIP(e, grid_job_bind(fin[a], src[a].c->lgrid, src[a].c->gscr, m, ncell, g[a]));
            const bool rule = grid_widen(min_per_cell, grow, m, m);
            fin[a].occ = rule ? src[a].occ : nullptr;
            if (rule) LO_HIP(e, hipMemsetAsync(src[a].occ, 0, sizeof(uint32_t), bs));
            any_rule = any_rule || rule;
            S->h_jobs[k++] = fin[a];
            max_n = std::max(max_n, ncell + 1);
            max_m = std::max(max_m, m);
        }
        LO_HIP(e, upload(k));
        grid_emit(grid_run(bs, S->d_jobs, nullptr, k, max_m, max_n), kGridBin);
        LO_HIP(e, hipGetLastError());
        if (!any_rule) break;                                // nobody can ask: every open job is at its final edge
        // the open jobs' occupied-cell words sit side by side (src[].occ = base + slot): one copy of the span
        const uint32_t* lo_occ = src[act.front()].occ;
        const uint32_t* hi_occ = lo_occ;
        for (int a : act) { lo_occ = std::min(lo_occ, static_cast<const uint32_t*>(src[a].occ)); hi_occ = std::max(hi_occ, static_cast<const uint32_t*>(src[a].occ)); }
        const size_t span = static_cast<size_t>(hi_occ - lo_occ) + 1;
        if (7 * static_cast<size_t>(n) + span > S->h_bounds.capacity()) { e->err = "loop grid: occupancy words out of range"; return LO_ERR_STATE; }
        LO_HIP(e, hipMemcpyAsync(h_occ + 7 * n, lo_occ, sizeof(uint32_t) * span, hipMemcpyDeviceToHost, bs));
        LO_HIP(e, hipStreamSynchronize(bs));
        for (int a : act) {
            const uint32_t occupied = h_occ[7 * n + (static_cast<const uint32_t*>(src[a].occ) - lo_occ)];
            if (fin[a].occ && grid_widen(min_per_cell, grow, src[a].m, occupied)) g[a].h *= 2.0f;
            else open[a] = 0;
        }
    }
    size_t max_n = 1, max_m = 1;
    for (int a = 0; a < n; ++a) { max_n = std::max<size_t>(max_n, fin[a].n); max_m = std::max(max_m, src[a].m); }
    const GridRun R = grid_run(bs, S->d_jobs, nullptr, n, max_m, max_n);
    LO_HIP(e, S->d_bsum.reserve(std::max(static_cast<size_t>(kGridBatchWGs), B)));      // >= nblk * n
    LO_HIP(e, settle());
    for (int a = 0; a < n; ++a) {
        grid_job_scan(fin[a], R.nblk, S->d_bsum + static_cast<size_t>(a) * R.nblk);
        S->h_jobs[a] = fin[a];
    }
    LO_HIP(e, upload(n));
    grid_emit(R, kGridOrder);
    LO_HIP(e, hipGetLastError());
    return LO_OK;
}

// The kd visit order for a grid whose points are on the device only (grid_from_device, all_pairs_device): its points
// back in index order (each grid point carries its index), then the host build with the order -- the same grid plus
// the order.
int grid_add_order(lo_ctx* c, PointGrid& G, int min_per_cell) {
    const size_t m = static_cast<size_t>(G.m);
    std::vector<float4> p(std::max<size_t>(m, 1));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    if (m > 0) LO_HIP(c, hipMemcpy(p.data(), G.d_pts, m * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<float> xyz(3 * std::max<size_t>(m, 1));
    for (size_t k = 0; k < m; ++k) {
        int i;
        std::memcpy(&i, &p[k].w, sizeof(int));
        if (i < 0 || static_cast<size_t>(i) >= m) { c->err = "device grid: bad point index"; return LO_ERR_STATE; }
        xyz[3 * i] = p[k].x; xyz[3 * i + 1] = p[k].y; xyz[3 * i + 2] = p[k].z;
    }
    return grid_build(c, G, xyz.data(), m, true, min_per_cell);
}
int grid_add_order(lo_ctx* c) {
    const int rc = grid_add_order(c, c->grid, 0);
    if (rc == LO_OK) c->grid_dev = true;                 // still the device map's grid (the next keyframe rebuilds it)
    return rc;
}
}  // namespace lo

extern "C" {

int lo_map_set_points(lo_ctx* c, const float* xyz, size_t m) {
    if (!c) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (!c->kd) { c->err = "lo_map_set_points needs use_surfel_correspondence = 0"; return LO_ERR_STATE; }
    c->grid_dev = false;
    return grid_build(c, c->grid, xyz, m);
}

int lo_kd_reruns(const lo_ctx* c) { return c ? c->kd_reruns : -1; }
long long lo_loop_reruns(const lo_ctx* c) { return c ? static_cast<long long>(c->loop_reruns) : -1; }

size_t lo_map_point_count(const lo_ctx* c) { return c ? static_cast<size_t>(c->grid.m) : 0; }

}  // extern "C"
