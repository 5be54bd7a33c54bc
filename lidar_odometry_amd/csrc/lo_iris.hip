// lo_iris.hip — LiDAR-Iris loop-closure detector on the device (include/lo_iris.h; DESIGN.md "LiDAR-Iris loop detector").
//
// Three kernels, all with bounded loops, none waiting on another block:
//   k_iris_image   points -> the 80 x 360 uint8 iris image (32-bit atomic OR on the containing word)
//   k_iris_encode  image -> the bit-packed descriptor (fp64 circular convolution with the log-Gabor kernels)
//   k_iris_match   one query descriptor against every database entry at all 360 column shifts, in-block argmin
//
// The packed descriptor's layout and the kernels' device bodies are in lo_iris_body.h, shared with the batched
// detector (lo_iris_batch.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lo_iris.h"
#include "lo_buf.h"
#include "lo_ctx_internal.h"
#include "lo_iris_body.h"

namespace lo {
namespace iris {

__global__ void __launch_bounds__(256) k_iris_image(const float* __restrict__ pts, int n, uint32_t* __restrict__ img) {
    image_points(pts, n, img, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// image row blockIdx.x, scale blockIdx.y
__global__ void __launch_bounds__(kThreads) k_iris_encode(const uint32_t* __restrict__ img,
                                                          const double2* __restrict__ h,
                                                          uint32_t* __restrict__ desc) {
    encode_row(img, h, desc, blockIdx.x, blockIdx.y);
}

// One workgroup = database entries blockIdx.x * kEntries ... (past the end: the last one again, not written) x all
// 360 shifts.
__global__ void __launch_bounds__(kThreads) k_iris_match(const uint64_t* __restrict__ db,
                                                         const uint64_t* __restrict__ q, int n_db,
                                                         float* __restrict__ out_dist, int* __restrict__ out_bias,
                                                         int* __restrict__ out_diff, int* __restrict__ out_total) {
    const int e0 = blockIdx.x * kEntries;
    const uint64_t* ent[kEntries];
#pragma unroll
    for (int j = 0; j < kEntries; ++j) ent[j] = db + static_cast<size_t>(min(e0 + j, n_db - 1)) * kDescWords;
    match_block(q, ent, [&](int j, float dist, int bias, int diff, int total) {
        const int e = e0 + j;
        if (e >= n_db) return;
        out_dist[e] = dist;
        out_bias[e] = bias;
        out_diff[e] = diff;
        out_total[e] = total;
    });
}

}  // namespace iris
}  // namespace lo

// ================================================================================================== host side
using namespace lo;
using namespace lo::iris;

struct lo_iris {
    lo_ctx* ctx = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    size_t capacity = 0;
    std::vector<int64_t> ids;
    std::vector<float> pos;
    DevBuf<uint64_t> d_db;               // capacity + 1 descriptors; the last is the query's
    DevBuf<uint32_t> d_img;
    DevBuf<double2> d_h;
    DevBuf<float> d_pts;                 // staging of host clouds
    DevBuf<float> d_dist;                // per-entry match records
    DevBuf<int> d_rec;                   // bias, diff, total: 3 x capacity
    bool has_query = false;
    std::vector<float> h_dist;
    std::string err;
};

static int ir_enter(lo_iris* m) {
    LO_HIP(m, hipSetDevice(m->device));
    m->stream = static_cast<hipStream_t>(lo_stream(m->ctx));   // lo_set_stream may have replaced it
    return LO_OK;
}

static uint64_t* ir_slot(lo_iris* m, size_t i) { return m->d_db + i * kDescWords; }

// points (host or device) -> d_img
static int ir_image(lo_iris* m, const float* pts, size_t n, int on_device) {
    if (n > static_cast<size_t>(INT_MAX) / 3) { m->err = "too many points"; return LO_ERR_ARG; }
    const float* d = pts;
    if (!on_device && n > 0) {
        if (3 * n > m->d_pts.capacity()) LO_HIP(m, m->d_pts.reserve(3 * std::max<size_t>(2 * n, 1 << 16)));
        LO_HIP(m, hipMemcpyAsync(m->d_pts, pts, n * 3 * sizeof(float), hipMemcpyHostToDevice, m->stream));
        d = m->d_pts;
    }
    LO_HIP(m, hipMemsetAsync(m->d_img, 0, kImgWords * sizeof(uint32_t), m->stream));
    if (n > 0) {
        const int blocks = static_cast<int>(std::min<size_t>(1024, (n + 255) / 256));
        hipLaunchKernelGGL(k_iris_image, dim3(blocks), dim3(256), 0, m->stream, d, static_cast<int>(n), m->d_img);
        LO_HIP(m, hipGetLastError());
    }
    return LO_OK;
}

// d_img -> the packed descriptor in slot
static int ir_encode(lo_iris* m, uint64_t* slot) {
    LO_HIP(m, hipMemsetAsync(slot, 0, kDescWords * sizeof(uint64_t), m->stream));
    hipLaunchKernelGGL(k_iris_encode, dim3(kRows, kScales), dim3(kThreads), 0, m->stream, m->d_img, m->d_h,
                       reinterpret_cast<uint32_t*>(slot));
    LO_HIP(m, hipGetLastError());
    return LO_OK;
}

static int ir_push(lo_iris* m, int64_t id, const float position[3]) {
    m->ids.push_back(id);
    m->pos.insert(m->pos.end(), position, position + 3);
    return LO_OK;
}

static int ir_match(lo_iris* m) {
    const int n_db = static_cast<int>(m->ids.size());
    int* r = m->d_rec;
    hipLaunchKernelGGL(k_iris_match, dim3((n_db + kEntries - 1) / kEntries), dim3(kThreads), 0, m->stream, m->d_db,
                       ir_slot(m, m->capacity), n_db, m->d_dist, r, r + m->capacity, r + 2 * m->capacity);
    LO_HIP(m, hipGetLastError());
    return LO_OK;
}

extern "C" {

void lo_iris_config_default(lo_iris_config* cfg) {
    if (!cfg) return;
    cfg->similarity_threshold = 0.3f;
    cfg->min_keyframe_gap = 50;
    cfg->max_search_distance = 10.0f;
}

lo_iris* lo_iris_create(lo_ctx* ctx, size_t capacity, int* err) {
    auto fail = [&](int rc, const char* msg, lo_iris* m) -> lo_iris* {
        std::fprintf(stderr, "lo_iris_create: %s\n", m && !m->err.empty() ? m->err.c_str() : msg);
        if (m) lo_iris_destroy(m);
        if (err) *err = rc;
        return nullptr;
    };
    if (!ctx || capacity < 1 || capacity > (size_t(1) << 20))
        return fail(LO_ERR_ARG, "bad arguments (a context, 1 <= capacity <= 2^20)", nullptr);
    lo_iris* m = new lo_iris();
    m->ctx = ctx;
    m->device = lo_device(ctx);
    m->capacity = capacity;
    auto init = [&]() -> int {
        int rc = ir_enter(m);
        if (rc != LO_OK) return rc;
        LO_HIP(m, m->d_db.reserve((capacity + 1) * kDescWords));
        LO_HIP(m, m->d_img.reserve(kImgWords));
        LO_HIP(m, m->d_h.reserve(static_cast<size_t>(kScales) * kCols));
        LO_HIP(m, m->d_dist.reserve(capacity));
        LO_HIP(m, m->d_rec.reserve(3 * capacity));
        std::vector<double> h;
        build_kernels(h);
        LO_HIP(m, hipMemcpy(m->d_h, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        return LO_OK;
    };
    const int rc = init();
    if (rc != LO_OK) return fail(rc, "allocation", m);
    m->ids.reserve(capacity);
    m->pos.reserve(3 * capacity);
    if (err) *err = LO_OK;
    return m;
}

void lo_iris_destroy(lo_iris* m) {
    if (!m) return;
    if (hipSetDevice(m->device) == hipSuccess && m->stream)
        (void)hipStreamSynchronize(static_cast<hipStream_t>(lo_stream(m->ctx)));
    delete m;
}

const char* lo_iris_last_error(const lo_iris* m) { return m ? m->err.c_str() : "null detector"; }
size_t lo_iris_size(const lo_iris* m) { return m ? m->ids.size() : 0; }
size_t lo_iris_capacity(const lo_iris* m) { return m ? m->capacity : 0; }

int lo_iris_clear(lo_iris* m) {
    if (!m) return LO_ERR_ARG;
    m->ids.clear();
    m->pos.clear();
    return LO_OK;
}

int lo_iris_image(lo_iris* m, const float* pts, size_t n, uint8_t* out_img) {
    if (!m || !out_img || (n > 0 && !pts)) return LO_ERR_ARG;
    int rc = ir_enter(m);
    if (rc == LO_OK) rc = ir_image(m, pts, n, 0);
    if (rc != LO_OK) return rc;
    LO_HIP(m, hipMemcpyAsync(out_img, m->d_img, kImgWords * sizeof(uint32_t), hipMemcpyDeviceToHost, m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));
    return LO_OK;
}

int lo_iris_encode(lo_iris* m, const uint8_t* img, uint8_t* out_T, uint8_t* out_M) {
    if (!m || !img || !out_T || !out_M) return LO_ERR_ARG;
    int rc = ir_enter(m);
    if (rc != LO_OK) return rc;
    m->has_query = false;                                  // the query slot is the scratch descriptor
    LO_HIP(m, hipMemcpyAsync(m->d_img, img, kImgWords * sizeof(uint32_t), hipMemcpyHostToDevice, m->stream));
    rc = ir_encode(m, ir_slot(m, m->capacity));
    if (rc != LO_OK) return rc;
    std::vector<uint64_t> d(kDescWords);
    LO_HIP(m, hipMemcpyAsync(d.data(), ir_slot(m, m->capacity), kDescWords * sizeof(uint64_t), hipMemcpyDeviceToHost,
                             m->stream));
    LO_HIP(m, hipStreamSynchronize(m->stream));
    for (int s = 0; s < kScales; ++s)
        for (int r = 0; r < kRows; ++r)
            for (int c = 0; c < kCols; ++c) {
                const int p = r * kScales + s;
                const uint64_t* col = d.data() + static_cast<size_t>(c) * kWords + (p >> 6);
                const uint8_t re = (col[0] >> (p & 63)) & 1, im = (col[kHalfWords] >> (p & 63)) & 1;
                const uint8_t masked = !((col[2 * kHalfWords] >> (p & 63)) & 1);
                const size_t a = (static_cast<size_t>(s) * kRows + r) * kCols + c;
                const size_t b = (static_cast<size_t>(kScales + s) * kRows + r) * kCols + c;
                out_T[a] = re ? 255 : 0;
                out_T[b] = im ? 255 : 0;
                out_M[a] = out_M[b] = masked ? 255 : 0;
            }
    return LO_OK;
}

int lo_iris_add_keyframe(lo_iris* m, int64_t id, const float position[3], const float* pts, size_t n, int on_device) {
    if (!m || !position || (n > 0 && !pts)) return LO_ERR_ARG;
    if (n == 0) return LO_INSUFFICIENT;
    if (m->ids.size() >= m->capacity) { m->err = "database full"; return LO_ERR_CAPACITY; }
    int rc = ir_enter(m);
    if (rc == LO_OK) rc = ir_image(m, pts, n, on_device);
    if (rc == LO_OK) rc = ir_encode(m, ir_slot(m, m->ids.size()));
    if (rc != LO_OK) return rc;
    LO_HIP(m, hipStreamSynchronize(m->stream));           // the caller's buffer (or the staging copy) is free again
    return ir_push(m, id, position);
}

int lo_iris_add_from_scan(lo_iris* m, int64_t id, const float position[3]) {
    if (!m || !position) return LO_ERR_ARG;
    if (m->ids.size() >= m->capacity) { m->err = "database full"; return LO_ERR_CAPACITY; }
    int rc = ir_enter(m);
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
    if (n <= 0) return LO_INSUFFICIENT;
    if (n > cfg.max_points) { m->err = "filtered count beyond max_points"; return LO_ERR_STATE; }
    rc = ir_image(m, d_scan, static_cast<size_t>(n), 1);
    if (rc == LO_OK) rc = ir_encode(m, ir_slot(m, m->ids.size()));
    if (rc != LO_OK) return rc;
    LO_HIP(m, hipStreamSynchronize(m->stream));
    return ir_push(m, id, position);
}

int lo_iris_compare_all(lo_iris* m, const float* pts, size_t n, int on_device, float* out_dist, int32_t* out_bias,
                        int32_t* out_diff, int32_t* out_total) {
    if (!m || (n > 0 && !pts)) return LO_ERR_ARG;
    if (n == 0) return LO_INSUFFICIENT;
    int rc = ir_enter(m);
    if (rc == LO_OK) rc = ir_image(m, pts, n, on_device);
    if (rc == LO_OK) rc = ir_encode(m, ir_slot(m, m->capacity));
    if (rc != LO_OK) return rc;
    m->has_query = true;
    const size_t k = m->ids.size();
    if (k > 0) {
        rc = ir_match(m);
        if (rc != LO_OK) return rc;
        const int* r = m->d_rec;
        if (out_dist) LO_HIP(m, hipMemcpyAsync(out_dist, m->d_dist, k * sizeof(float), hipMemcpyDeviceToHost, m->stream));
        if (out_bias) LO_HIP(m, hipMemcpyAsync(out_bias, r, k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        if (out_diff) LO_HIP(m, hipMemcpyAsync(out_diff, r + m->capacity, k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
        if (out_total) LO_HIP(m, hipMemcpyAsync(out_total, r + 2 * m->capacity, k * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    }
    LO_HIP(m, hipStreamSynchronize(m->stream));
    return LO_OK;
}

long long lo_iris_select_host(const lo_iris_config* cfg, int64_t current_id, const float current_position[3],
                              const int64_t* ids, const float* positions, const float* dist, size_t n) {
    if (!cfg || !current_position || (n > 0 && (!ids || !positions || !dist))) return -1;
    Best best;                                             // the rule itself: lo_iris_body.h
    for (size_t i = 0; i < n; ++i)
        if (eligible(*cfg, current_id, current_position, ids[i], positions + 3 * i))
            best.offer(static_cast<long long>(i), dist[i]);
    return best.pick(*cfg);
}

int lo_iris_detect(lo_iris* m, const lo_iris_config* cfg, int64_t id, const float position[3], const float* pts,
                   size_t n, int on_device, lo_iris_candidate* cand) {
    if (!m || !cfg || !position || !cand || (n > 0 && !pts)) return LO_ERR_ARG;
    if (n == 0 || m->ids.empty()) return LO_INSUFFICIENT;
    const size_t k = m->ids.size();
    m->h_dist.resize(k);
    std::vector<int32_t> bias(k);
    const int rc = lo_iris_compare_all(m, pts, n, on_device, m->h_dist.data(), bias.data(), nullptr, nullptr);
    if (rc != LO_OK) return rc;
    const long long i = lo_iris_select_host(cfg, id, position, m->ids.data(), m->pos.data(), m->h_dist.data(), k);
    if (i < 0) return LO_INSUFFICIENT;
    cand->query_keyframe_id = id;
    cand->match_keyframe_id = m->ids[i];
    cand->distance = m->h_dist[i];
    cand->bias = bias[i];
    return LO_OK;
}

int lo_iris_bench_match(lo_iris* m, int reps, float* avg_ms) {
    if (!m || !avg_ms || reps < 1) return LO_ERR_ARG;
    if (!m->has_query || m->ids.empty()) { m->err = "no query / empty database"; return LO_ERR_STATE; }
    int rc = ir_enter(m);
    if (rc == LO_OK) rc = ir_match(m);                     // warm-up
    if (rc != LO_OK) return rc;
    hipEvent_t a, b;
    LO_HIP(m, hipEventCreate(&a));
    LO_HIP(m, hipEventCreate(&b));
    LO_HIP(m, hipEventRecord(a, m->stream));
    for (int i = 0; i < reps && rc == LO_OK; ++i) rc = ir_match(m);
    LO_HIP(m, hipEventRecord(b, m->stream));
    LO_HIP(m, hipEventSynchronize(b));
    float ms = 0.0f;
    LO_HIP(m, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *avg_ms = ms / static_cast<float>(reps);
    return rc;
}

}  // extern "C"
