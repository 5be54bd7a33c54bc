// lo_gmap.hip — the global-map builder on the device (include/lo_gmap.h; DESIGN.md "Global map builder").
//
// The reference's VoxelGrid::filter is a sequential fp32 running average per voxel, in input order, read out of a
// std::map in (x, y, z) key order.  A STABLE sort of (voxel key, input index) puts every voxel's points side by side
// in input order and the voxels in key order; each voxel's run is then walked sequentially by one lane, so the same
// operations happen in the same order and the bits are the reference's.
//
//   k_gmap_transform   arena point -> world point (transform_pt) + packed key + range check        12 B in, 20 B out
//   hipcub radix sort  (key, input index) pairs, stable, bits 0..62
//   k_gmap_heads       run starts flagged; world points gathered into sorted order
//   hipcub scan        exclusive sum of the flags = each point's voxel number; its last entry = the voxel count
//   k_gmap_starts      voxel number -> first sorted position
//   k_gmap_centroids   one lane per voxel walks its run (three axes share the two divisions of a step)
//
// The arena is cut into chunks of at most kChunk points of ONE keyframe when the keyframe is added; a transform
// workgroup takes one chunk, so its pose is workgroup-uniform and is read through the scalar unit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/lo_gmap.h"
#include "../../include/lo_io.h"
#include "lo_buf.h"
#include "lo_ctx_internal.h"
#include "lo_device.h"

namespace lo {
namespace gmap {

constexpr int kChunk = 1024;                       // points per transform workgroup (4 per thread)
constexpr int kKeyBits = 63;                       // three 21-bit fields
constexpr uint64_t kBadKey = (1ull << kKeyBits) - 1;

struct Chunk {
    int kf;                                        // keyframe (pose index)
    int start;                                     // first arena point
    int n;                                         // 1..kChunk
    int pad;
};

// pack_key with x in the top field: unsigned order of the packed word = signed (kx, ky, kz) order
__device__ __forceinline__ uint64_t pack_key_xyz(int kx, int ky, int kz) {
    return (static_cast<uint64_t>(static_cast<uint32_t>(kx + (1 << 20))) << 42) |
           (static_cast<uint64_t>(static_cast<uint32_t>(ky + (1 << 20))) << 21) |
           static_cast<uint64_t>(static_cast<uint32_t>(kz + (1 << 20)));
}

// get_voxel_key's one axis: (int)floorf(p / leaf).  Clamped in floating point first so the cast is defined; a clamped
// value fails key_in_range.
__device__ __forceinline__ int axis_key(float p, float leaf) {
    const float f = fminf(fmaxf(floorf(p / leaf), -2097152.0f), 2097152.0f);
    return static_cast<int>(f);
}

// ------------------------------------------------------------------------------------------------ transform + key
template <bool KEYS>
__global__ void __launch_bounds__(kBlock) k_gmap_transform(const float* __restrict__ arena,
                                                           const Chunk* __restrict__ chunks,
                                                           const float* __restrict__ poses, float leaf,
                                                           float* __restrict__ world, uint64_t* __restrict__ keys,
                                                           unsigned* __restrict__ bad) {
    const Chunk ch = chunks[blockIdx.x];           // workgroup-uniform: scalar loads
    const float* Tp = poses + 12 * static_cast<size_t>(ch.kf);
    float T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tp[k];
    // all four loads first (the index clamped into the chunk, ch.n >= 1, so none needs a branch), then the arithmetic
    float p[kChunk / kBlock][3];
#pragma unroll
    for (int r = 0; r < kChunk / kBlock; ++r) {
        const int j = min(r * kBlock + static_cast<int>(threadIdx.x), ch.n - 1);
        const size_t i = static_cast<size_t>(ch.start) + j;       // < the arena's point count by construction
        p[r][0] = arena[3 * i];
        p[r][1] = arena[3 * i + 1];
        p[r][2] = arena[3 * i + 2];
    }
#pragma unroll
    for (int r = 0; r < kChunk / kBlock; ++r) {
        const int j = r * kBlock + static_cast<int>(threadIdx.x);
        if (j >= ch.n) break;
        const size_t i = static_cast<size_t>(ch.start) + j;
        float wx, wy, wz;
        transform_pt(T, p[r][0], p[r][1], p[r][2], wx, wy, wz);
        world[3 * i] = wx;
        world[3 * i + 1] = wy;
        world[3 * i + 2] = wz;
        if (KEYS) {
            const int kx = axis_key(wx, leaf), ky = axis_key(wy, leaf), kz = axis_key(wz, leaf);
            const bool ok = isfinite(wx) && isfinite(wy) && isfinite(wz) && key_in_range(kx) && key_in_range(ky) &&
                            key_in_range(kz);
            keys[i] = ok ? pack_key_xyz(kx, ky, kz) : kBadKey;
            if (!ok) atomicAdd(bad, 1u);
        }
    }
}

// ------------------------------------------------------------------------------------------------ heads + gather
// Sorted position i: flag = 1 where a voxel's run starts; the world point moved to its sorted position.  Entry n of
// the flags is 0, so the exclusive sum's entry n is the voxel count.
__global__ void __launch_bounds__(kBlock) k_gmap_heads(const uint64_t* __restrict__ skeys,
                                                       const uint32_t* __restrict__ sidx,
                                                       const float* __restrict__ world, int n,
                                                       uint32_t* __restrict__ flag, float* __restrict__ sorted) {
    const int i = blockIdx.x * kBlock + static_cast<int>(threadIdx.x);
    if (i > n) return;
    if (i == n) { flag[n] = 0u; return; }
    flag[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1u : 0u;
    const size_t s = sidx[i];                      // < n: a permutation of 0..n-1
    const size_t d = static_cast<size_t>(i);
    sorted[3 * d] = world[3 * s];
    sorted[3 * d + 1] = world[3 * s + 1];
    sorted[3 * d + 2] = world[3 * s + 2];
}

// rid = exclusive sum of flag (n + 1 entries).  starts[v] = first sorted position of voxel v, starts[M] = n;
// counts[1] = M.
__global__ void __launch_bounds__(kBlock) k_gmap_starts(const uint32_t* __restrict__ flag,
                                                        const uint32_t* __restrict__ rid, int n,
                                                        uint32_t* __restrict__ starts, unsigned* __restrict__ counts) {
    const int i = blockIdx.x * kBlock + static_cast<int>(threadIdx.x);
    if (i > n) return;
    if (i == n) {
        starts[rid[n]] = static_cast<uint32_t>(n);             // rid[n] = M <= n: starts has n + 1 entries
        counts[1] = rid[n];
    } else if (flag[i]) {
        starts[rid[i]] = static_cast<uint32_t>(i);
    }
}

// ------------------------------------------------------------------------------------------------ centroids
// WeightedCentroid::add_point over one voxel's run, in order.  w counts in fp32 as the reference's does (it stops
// growing at 2^24).  The loads of a step do not depend on the chain, so four points are fetched ahead of their steps.
__device__ __forceinline__ void add_point(float& cx, float& cy, float& cz, float& w, float px, float py, float pz) {
    const float tw = w + 1.0f;
    const float a = w / tw;
    const float b = 1.0f / tw;
    cx = a * cx + b * px;
    cy = a * cy + b * py;
    cz = a * cz + b * pz;
    w = tw;
}

__global__ void __launch_bounds__(kBlock) k_gmap_centroids(const float* __restrict__ sorted,
                                                           const uint32_t* __restrict__ starts,
                                                           const unsigned* __restrict__ counts,
                                                           float* __restrict__ out) {
    const uint32_t v = blockIdx.x * kBlock + threadIdx.x;
    if (v >= counts[1]) return;
    const uint32_t b = starts[v], e = starts[v + 1];           // b < e <= n
    const float* p = sorted + 3 * static_cast<size_t>(b);
    float cx = p[0], cy = p[1], cz = p[2], w = 1.0f;
    uint32_t left = e - b - 1;
    p += 3;
    for (; left >= 4; left -= 4, p += 12) {
        float q[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) q[k] = p[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) add_point(cx, cy, cz, w, q[3 * k], q[3 * k + 1], q[3 * k + 2]);
    }
    for (; left > 0; --left, p += 3) add_point(cx, cy, cz, w, p[0], p[1], p[2]);
    out[3 * static_cast<size_t>(v)] = cx;
    out[3 * static_cast<size_t>(v) + 1] = cy;
    out[3 * static_cast<size_t>(v) + 2] = cz;
}

__global__ void __launch_bounds__(kBlock) k_gmap_iota(uint32_t* __restrict__ v, size_t n) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) v[i] = static_cast<uint32_t>(i);
}

}  // namespace gmap
}  // namespace lo

// ================================================================================================== host side
using namespace lo;
using namespace lo::gmap;

struct lo_gmap {
    lo_ctx* ctx = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    size_t max_points = 0, max_keyframes = 0, max_chunks = 0;
    std::vector<int64_t> ids;
    std::vector<size_t> kf_start, kf_n;  // each keyframe's first arena point and count
    std::vector<Chunk> chunks;           // host mirror of d_chunks
    size_t n_points = 0;
    // device buffers, all sized at create
    DevBuf<float> d_arena;               // stored clouds, sensor frame
    DevBuf<Chunk> d_chunks;
    DevBuf<float> d_poses;               // max_keyframes x 12
    DevBuf<float> d_world;               // transformed concatenation (the voxel_size <= 0 result)
    DevBuf<uint64_t> d_keys;
    DevBuf<uint64_t> d_skeys;
    DevBuf<uint32_t> d_iota;             // 0..max_points-1, written once
    DevBuf<uint32_t> d_sidx;
    DevBuf<uint32_t> d_flag;             // max_points + 1
    DevBuf<uint32_t> d_rid;              // max_points + 1
    DevBuf<uint32_t> d_starts;           // max_points + 1
    DevBuf<float> d_sorted;
    DevBuf<float> d_out;
    DevBuf<unsigned> d_counts;           // [0] points out of range, [1] voxels
    DevBuf<void> d_tmp;                  // hipcub work space
    // last build
    const float* d_result = nullptr;
    size_t n_result = 0;
    float stage_ms[LO_GMAP_STAGES] = {0.0f, 0.0f, 0.0f, 0.0f};
    std::string err;
};

static int gm_enter(lo_gmap* m) {
    LO_HIP(m, hipSetDevice(m->device));
    m->stream = static_cast<hipStream_t>(lo_stream(m->ctx));   // lo_set_stream may have replaced it
    return LO_OK;
}

static int gm_blocks(size_t n) { return static_cast<int>((n + kBlock - 1) / kBlock); }

// The arena bookkeeping of one more keyframe of n points starting at the current end (the copy is already enqueued).
static int gm_push(lo_gmap* m, int64_t id, size_t n) {
    const size_t first = m->chunks.size();
    const int kf = static_cast<int>(m->ids.size());
    for (size_t off = 0; off < n; off += kChunk)
        m->chunks.push_back(Chunk{kf, static_cast<int>(m->n_points + off),
                                  static_cast<int>(std::min<size_t>(kChunk, n - off)), 0});
    const size_t added = m->chunks.size() - first;             // <= max_chunks in total: n / kChunk + 1 per keyframe
    if (added > 0)
        LO_HIP(m, hipMemcpyAsync(m->d_chunks + first, m->chunks.data() + first, added * sizeof(Chunk),
                                 hipMemcpyHostToDevice, m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));               // the caller's buffer is free again
    m->ids.push_back(id);
    m->kf_start.push_back(m->n_points);
    m->kf_n.push_back(n);
    m->n_points += n;
    return LO_OK;
}

static int gm_room(lo_gmap* m, size_t n) {
    if (m->ids.size() >= m->max_keyframes) { m->err = "keyframe capacity reached"; return LO_ERR_CAPACITY; }
    if (n > m->max_points - m->n_points) { m->err = "point capacity reached"; return LO_ERR_CAPACITY; }
    return LO_OK;
}

// One build's launches on the stream (no readback).  ev: nullable, LO_GMAP_STAGES + 1 events recorded around the stages.
static int gm_enqueue(lo_gmap* m, float voxel_size, hipEvent_t* ev) {
    const int n = static_cast<int>(m->n_points);
    const dim3 grid_t(static_cast<unsigned>(m->chunks.size())), blk(kBlock);
    const bool filter = voxel_size > 0.0f;
    LO_HIP(m, hipMemsetAsync(m->d_counts, 0, 2 * sizeof(unsigned), m->stream));
    if (ev) LO_HIP(m, hipEventRecord(ev[0], m->stream));
    if (!filter) {
        hipLaunchKernelGGL(k_gmap_transform<false>, grid_t, blk, 0, m->stream, m->d_arena, m->d_chunks, m->d_poses,
                           1.0f, m->d_world, m->d_keys, m->d_counts);
        LO_HIP(m, hipGetLastError());
        if (ev)
            for (int s = 1; s <= LO_GMAP_STAGES; ++s) LO_HIP(m, hipEventRecord(ev[s], m->stream));
        return LO_OK;
    }
    hipLaunchKernelGGL(k_gmap_transform<true>, grid_t, blk, 0, m->stream, m->d_arena, m->d_chunks, m->d_poses,
                       voxel_size, m->d_world, m->d_keys, m->d_counts);
    LO_HIP(m, hipGetLastError());
    if (ev) LO_HIP(m, hipEventRecord(ev[1], m->stream));
    size_t t = m->d_tmp.capacity();
    LO_HIP(m, hipcub::DeviceRadixSort::SortPairs(m->d_tmp, t, m->d_keys.get(), m->d_skeys.get(), m->d_iota.get(), m->d_sidx.get(), n, 0,
                                                 kKeyBits, m->stream));
    if (ev) LO_HIP(m, hipEventRecord(ev[2], m->stream));
    const dim3 grid_n1(gm_blocks(static_cast<size_t>(n) + 1));
    hipLaunchKernelGGL(k_gmap_heads, grid_n1, blk, 0, m->stream, m->d_skeys, m->d_sidx, m->d_world, n, m->d_flag,
                       m->d_sorted);
    LO_HIP(m, hipGetLastError());
    t = m->d_tmp.capacity();
    LO_HIP(m, hipcub::DeviceScan::ExclusiveSum(m->d_tmp, t, m->d_flag.get(), m->d_rid.get(), n + 1, m->stream));
    hipLaunchKernelGGL(k_gmap_starts, grid_n1, blk, 0, m->stream, m->d_flag, m->d_rid, n, m->d_starts, m->d_counts);
    LO_HIP(m, hipGetLastError());
    if (ev) LO_HIP(m, hipEventRecord(ev[3], m->stream));
    hipLaunchKernelGGL(k_gmap_centroids, dim3(gm_blocks(n)), blk, 0, m->stream, m->d_sorted, m->d_starts, m->d_counts,
                       m->d_out);
    LO_HIP(m, hipGetLastError());
    if (ev) LO_HIP(m, hipEventRecord(ev[4], m->stream));
    return LO_OK;
}

// Argument checks and the pose upload shared by build and bench_build.
static int gm_prepare(lo_gmap* m, const float* poses, size_t n_poses) {
    if (n_poses != m->ids.size()) { m->err = "n_poses differs from the keyframe count"; return LO_ERR_ARG; }
    if (m->n_points == 0) return LO_INSUFFICIENT;
    const int rc = gm_enter(m);
    if (rc != LO_OK) return rc;
    LO_HIP(m, hipMemcpyAsync(m->d_poses, poses, n_poses * 12 * sizeof(float), hipMemcpyHostToDevice, m->stream));
    return LO_OK;
}

extern "C" {

lo_gmap* lo_gmap_create(lo_ctx* ctx, size_t max_points, size_t max_keyframes, int* err) {
    auto fail = [&](int rc, const char* msg, lo_gmap* m) -> lo_gmap* {
        std::fprintf(stderr, "lo_gmap_create: %s\n", m && !m->err.empty() ? m->err.c_str() : msg);
        if (m) lo_gmap_destroy(m);
        if (err) *err = rc;
        return nullptr;
    };
    if (!ctx || max_points < 1 || max_points > (size_t(1) << 30) || max_keyframes < 1 ||
        max_keyframes > (size_t(1) << 24))
        return fail(LO_ERR_ARG, "bad arguments (a context, 1 <= max_points <= 2^30, 1 <= max_keyframes <= 2^24)",
                    nullptr);
    lo_gmap* m = new lo_gmap();
    m->ctx = ctx;
    m->device = lo_device(ctx);
    m->max_points = max_points;
    m->max_keyframes = max_keyframes;
    m->max_chunks = max_points / kChunk + max_keyframes;
    auto init = [&]() -> int {
        const int rc = gm_enter(m);
        if (rc != LO_OK) return rc;
        const size_t np = max_points;
        const int ni = static_cast<int>(np);
        size_t t_sort = 0, t_scan = 0;
        LO_HIP(m, hipcub::DeviceRadixSort::SortPairs(nullptr, t_sort, m->d_keys.get(), m->d_skeys.get(), m->d_iota.get(), m->d_sidx.get(), ni, 0,
                                                     kKeyBits, m->stream));
        LO_HIP(m, hipcub::DeviceScan::ExclusiveSum(nullptr, t_scan, m->d_flag.get(), m->d_rid.get(), ni + 1, m->stream));
        LO_HIP(m, m->d_arena.reserve(np * 3));
        LO_HIP(m, m->d_chunks.reserve(m->max_chunks));
        LO_HIP(m, m->d_poses.reserve(max_keyframes * 12));
        LO_HIP(m, m->d_world.reserve(np * 3));
        LO_HIP(m, m->d_keys.reserve(np));
        LO_HIP(m, m->d_skeys.reserve(np));
        LO_HIP(m, m->d_iota.reserve(np));
        LO_HIP(m, m->d_sidx.reserve(np));
        LO_HIP(m, m->d_flag.reserve(np + 1));
        LO_HIP(m, m->d_rid.reserve(np + 1));
        LO_HIP(m, m->d_starts.reserve(np + 1));
        LO_HIP(m, m->d_sorted.reserve(np * 3));
        LO_HIP(m, m->d_out.reserve(np * 3));
        LO_HIP(m, m->d_counts.reserve(2));
        LO_HIP(m, m->d_tmp.reserve(std::max<size_t>(std::max(t_sort, t_scan), 256)));
        hipLaunchKernelGGL(k_gmap_iota, dim3(gm_blocks(np)), dim3(kBlock), 0, m->stream, m->d_iota, np);
        LO_HIP(m, hipGetLastError());
        LO_HIP(m, hipStreamSynchronize(m->stream));
        return LO_OK;
    };
    const int rc = init();
    if (rc != LO_OK) return fail(rc, "allocation", m);
    m->ids.reserve(max_keyframes);
    m->chunks.reserve(m->max_chunks);
    if (err) *err = LO_OK;
    return m;
}

void lo_gmap_destroy(lo_gmap* m) {
    if (!m) return;
    if (hipSetDevice(m->device) == hipSuccess && m->stream)
        (void)hipStreamSynchronize(static_cast<hipStream_t>(lo_stream(m->ctx)));
    delete m;
}

const char* lo_gmap_last_error(const lo_gmap* m) { return m ? m->err.c_str() : "null map builder"; }
size_t lo_gmap_keyframes(const lo_gmap* m) { return m ? m->ids.size() : 0; }
size_t lo_gmap_points(const lo_gmap* m) { return m ? m->n_points : 0; }

int lo_gmap_clear(lo_gmap* m) {
    if (!m) return LO_ERR_ARG;
    m->ids.clear();
    m->kf_start.clear();
    m->kf_n.clear();
    m->chunks.clear();
    m->n_points = 0;
    m->d_result = nullptr;
    m->n_result = 0;
    return LO_OK;
}

int lo_gmap_add_keyframe(lo_gmap* m, int64_t id, const float* pts, size_t n, int on_device) {
    if (!m || (n > 0 && !pts)) return LO_ERR_ARG;
    int rc = gm_room(m, n);
    if (rc == LO_OK) rc = gm_enter(m);
    if (rc != LO_OK) return rc;
    if (n > 0)
        LO_HIP(m, hipMemcpyAsync(m->d_arena + 3 * m->n_points, pts, n * 3 * sizeof(float),
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, m->stream));
    return gm_push(m, id, n);
}

int lo_gmap_add_from_scan(lo_gmap* m, int64_t id) {
    if (!m) return LO_ERR_ARG;
    int rc = gm_room(m, 0);
    if (rc == LO_OK) rc = gm_enter(m);
    if (rc != LO_OK) return rc;
    const float* d_scan = nullptr;
    const int* d_scan_n = nullptr;
    rc = ctx_filtered_device(m->ctx, &d_scan, &d_scan_n);
    if (rc != LO_OK) { m->err = lo_last_error(m->ctx); return rc; }
    lo_config cfg;
    if (lo_get_config(m->ctx, &cfg) != LO_OK) return LO_ERR_ARG;
    int n = 0;
    LO_HIP(m, hipMemcpyAsync(&n, d_scan_n, sizeof(int), hipMemcpyDeviceToHost, m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));
    if (n < 0 || n > cfg.max_points) { m->err = "filtered count beyond max_points"; return LO_ERR_STATE; }
    rc = gm_room(m, static_cast<size_t>(n));
    if (rc != LO_OK) return rc;
    if (n > 0)
        LO_HIP(m, hipMemcpyAsync(m->d_arena + 3 * m->n_points, d_scan, static_cast<size_t>(n) * 3 * sizeof(float),
                                 hipMemcpyDeviceToDevice, m->stream));
    return gm_push(m, id, static_cast<size_t>(n));
}

int lo_gmap_keyframe_points(lo_gmap* m, size_t index, int64_t* id, const float** d_xyz, size_t* n) {
    if (!m || !d_xyz || !n) return LO_ERR_ARG;
    if (index >= m->ids.size()) { m->err = "keyframe index past the end"; return LO_ERR_ARG; }
    if (id) *id = m->ids[index];
    *d_xyz = m->d_arena + 3 * m->kf_start[index];
    *n = m->kf_n[index];
    return LO_OK;
}

int lo_gmap_build(lo_gmap* m, const float* poses, size_t n_poses, float voxel_size, size_t* out_n) {
    if (!m || (n_poses > 0 && !poses)) return LO_ERR_ARG;
    m->d_result = nullptr;
    m->n_result = 0;
    if (out_n) *out_n = 0;
    int rc = gm_prepare(m, poses, n_poses);
    if (rc == LO_OK) rc = gm_enqueue(m, voxel_size, nullptr);
    if (rc != LO_OK) return rc;
    unsigned counts[2] = {0u, 0u};
    LO_HIP(m, hipMemcpyAsync(counts, m->d_counts, sizeof(counts), hipMemcpyDeviceToHost, m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));
    if (voxel_size > 0.0f) {
        if (counts[0] != 0u) {
            m->err = std::to_string(counts[0]) + " of " + std::to_string(m->n_points) +
                     " world points are non-finite or have a voxel key outside [-2^20, 2^20)";
            return LO_ERR_ARG;
        }
        m->d_result = m->d_out;
        m->n_result = counts[1];
    } else {
        m->d_result = m->d_world;
        m->n_result = m->n_points;
    }
    if (out_n) *out_n = m->n_result;
    return LO_OK;
}

long long lo_gmap_download(lo_gmap* m, float* out, size_t cap) {
    if (!m) return LO_ERR_ARG;
    if (!m->d_result) { m->err = "no build result"; return LO_ERR_STATE; }
    if (!out) return static_cast<long long>(m->n_result);
    const size_t k = std::min(cap, m->n_result);
    const int rc = gm_enter(m);
    if (rc != LO_OK) return rc;
    if (k > 0) LO_HIP(m, hipMemcpyAsync(out, m->d_result, k * 3 * sizeof(float), hipMemcpyDeviceToHost, m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));
    return static_cast<long long>(k);
}

int lo_gmap_device_points(lo_gmap* m, const float** d_xyz, size_t* n) {
    if (!m || !d_xyz || !n) return LO_ERR_ARG;
    if (!m->d_result) { m->err = "no build result"; return LO_ERR_STATE; }
    *d_xyz = m->d_result;
    *n = m->n_result;
    return LO_OK;
}

int lo_gmap_save_ply(lo_gmap* m, const char* path) {
    if (!m || !path) return LO_ERR_ARG;
    if (!m->d_result) { m->err = "no build result"; return LO_ERR_STATE; }
    std::vector<float> h(3 * m->n_result);
    const long long k = lo_gmap_download(m, h.data(), m->n_result);
    if (k < 0) return static_cast<int>(k);
    const int rc = lo_save_ply(path, h.data(), static_cast<size_t>(k));
    if (rc != 0) {
        m->err = std::string(rc == LO_IO_ERR_OPEN ? "cannot write " : "nothing to write to ") + path;
        return LO_ERR_ARG;
    }
    return LO_OK;
}

int lo_gmap_bench_build(lo_gmap* m, const float* poses, size_t n_poses, float voxel_size, int reps, float* avg_ms) {
    if (!m || !avg_ms || reps < 1 || (n_poses > 0 && !poses)) return LO_ERR_ARG;
    int rc = gm_prepare(m, poses, n_poses);
    if (rc == LO_OK) rc = gm_enqueue(m, voxel_size, nullptr);  // warm-up
    if (rc != LO_OK) return rc;
    m->d_result = nullptr;                                     // the timed builds are not checked: no result
    m->n_result = 0;
    hipEvent_t ev[LO_GMAP_STAGES + 1];
    for (hipEvent_t& e : ev) LO_HIP(m, hipEventCreate(&e));
    auto done = [&](int r) {
        for (hipEvent_t& e : ev) (void)hipEventDestroy(e);
        return r;
    };
    auto hip = [&](hipError_t e) {
        if (e == hipSuccess) return true;
        m->err = std::string("lo_gmap_bench_build: ") + hipGetErrorString(e);
        return false;
    };
    if (!hip(hipEventRecord(ev[0], m->stream))) return done(LO_ERR_HIP);
    for (int i = 0; i < reps && rc == LO_OK; ++i) rc = gm_enqueue(m, voxel_size, nullptr);
    if (rc != LO_OK) return done(rc);
    float ms = 0.0f;
    if (!hip(hipEventRecord(ev[1], m->stream)) || !hip(hipEventSynchronize(ev[1])) ||
        !hip(hipEventElapsedTime(&ms, ev[0], ev[1])))
        return done(LO_ERR_HIP);
    *avg_ms = ms / static_cast<float>(reps);
    float acc[LO_GMAP_STAGES] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = 0; i < reps; ++i) {
        rc = gm_enqueue(m, voxel_size, ev);
        if (rc != LO_OK) return done(rc);
        if (!hip(hipEventSynchronize(ev[LO_GMAP_STAGES]))) return done(LO_ERR_HIP);
        for (int s = 0; s < LO_GMAP_STAGES; ++s) {
            if (!hip(hipEventElapsedTime(&ms, ev[s], ev[s + 1]))) return done(LO_ERR_HIP);
            acc[s] += ms;
        }
    }
    for (int s = 0; s < LO_GMAP_STAGES; ++s) m->stage_ms[s] = acc[s] / static_cast<float>(reps);
    return done(LO_OK);
}

int lo_gmap_stage_ms(const lo_gmap* m, float* out_ms) {
    if (!m || !out_ms) return LO_ERR_ARG;
    for (int s = 0; s < LO_GMAP_STAGES; ++s) out_ms[s] = m->stage_ms[s];
    return LO_OK;
}

}  // extern "C"
