// lo_iris.hip — LiDAR-Iris loop-closure detector on the device (include/lo_iris.h; DESIGN.md "LiDAR-Iris loop detector").
//
// Three kernels, all with bounded loops, none waiting on another block:
//   k_iris_image   points -> the 80 x 360 uint8 iris image (32-bit atomic OR on the containing word)
//   k_iris_encode  image -> the bit-packed descriptor (fp64 circular convolution with the log-Gabor kernels)
//   k_iris_match   one query descriptor against every database entry at all 360 column shifts, in-block argmin
//
// Packed descriptor (kDescWords 64-bit words = 43,200 B): column-major, 15 words per image column:
//   words 0..4   Re bits  (bit p = r * 4 + s of the column: range row r, scale s -- 320 bits)
//   words 5..9   Im bits  (same order)
//   words 10..14 VALID bits = ~M (same order; M's two halves are identical, so one copy serves Re and Im)
// The 640-row axis lies inside the words, so a circular column shift is an index rotation over whole 120-byte
// columns, and the row order inside a column (any fixed permutation) does not change a popcount.
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

namespace lo {
namespace iris {

constexpr int kRows = LO_IRIS_ROWS;
constexpr int kCols = LO_IRIS_COLS;
constexpr int kScales = 4;
constexpr int kHalfWords = 5;                      // 320 bits
constexpr int kWords = 3 * kHalfWords;             // per column: Re, Im, valid
constexpr int kDescWords = kCols * kWords;         // 5400 x 8 B = 43,200 B
constexpr int kImgWords = kRows * kCols / 4;       // the image as 32-bit words
constexpr int kThreads = 384;                      // >= kCols, 6 waves
constexpr int kEntries = 2;                        // database entries per match workgroup (query LDS reads shared)
static_assert(kRows * kScales == 64 * kHalfWords, "Re / Im / valid halves fill whole words");

// ---------------------------------------------------------------------------------------------------- image
// LidarIris::GetIris (LidarIris.cpp:4-19).
__global__ void __launch_bounds__(256) k_iris_image(const float* __restrict__ pts, int n, uint32_t* __restrict__ img) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        const float dis = sqrtf(x * x + y * y);
        const float yaw = static_cast<float>(static_cast<double>(atan2f(y, x) * 180.0f) / M_PI + 180.0);
        // clamped in floating point first: the reference's int casts of out-of-range values are only defined there
        const int q_dis = static_cast<int>(fminf(fmaxf(floorf(dis), 0.0f), static_cast<float>(kRows - 1)));
        const int q_arc = static_cast<int>(fminf(fmaxf(ceilf(z + 5.0f), 0.0f), 7.0f));
        const int q_yaw = static_cast<int>(fmin(fmax(floor(static_cast<double>(yaw) + 0.5), 0.0),
                                                static_cast<double>(kCols - 1)));
        const int cell = q_dis * kCols + q_yaw;            // < kRows * kCols by the clamps
        atomicOr(&img[cell >> 2], (1u << q_arc) << (8 * (cell & 3)));
    }
}

// ---------------------------------------------------------------------------------------------------- encode
// LogGaborFilter + LoGFeatureEncode (LidarIris.cpp:84-154) for image row blockIdx.x and scale blockIdx.y.
// idft(dft(x) . F_s) is the circular convolution of x with h_s = idft(F_s) (unscaled, as cv::idft without DFT_SCALE);
// h (4 x 360 complex, fp64) is built on the host, so one pass of 360 x 360 real-by-complex products per (row, scale)
// gives the response directly; zero cells (most of an iris image) are skipped, which is exact.
__global__ void __launch_bounds__(kThreads) k_iris_encode(const uint32_t* __restrict__ img,
                                                          const double2* __restrict__ h,
                                                          uint32_t* __restrict__ desc) {
    __shared__ double sx[kCols];
    __shared__ double2 sh[kCols];
    const int r = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
    if (t < kCols) {
        const int cell = r * kCols + t;
        sx[t] = static_cast<double>((img[cell >> 2] >> (8 * (cell & 3))) & 0xffu);
        sh[t] = h[s * kCols + t];
    }
    __syncthreads();
    if (t >= kCols) return;
    double re = 0.0, im = 0.0;
    int d = t;                                             // (t - m) mod 360
    for (int m = 0; m < kCols; ++m) {
        const double xm = sx[m];
        if (xm != 0.0) {                                   // block-uniform
            const double2 hv = sh[d];
            re += xm * hv.x;
            im += xm * hv.y;
        }
        d = d == 0 ? kCols - 1 : d - 1;
    }
    const int p = r * kScales + s;                         // bit inside the column's 320-bit half
    const uint32_t bit = 1u << (p & 31);
    uint32_t* col = desc + static_cast<size_t>(t) * (2 * kWords) + (p >> 5);
    if (re > 0.0) atomicOr(col, bit);
    if (im > 0.0) atomicOr(col + 2 * kHalfWords, bit);
    if (!(sqrt(re * re + im * im) < 1e-4)) atomicOr(col + 4 * kHalfWords, bit);
}

// ---------------------------------------------------------------------------------------------------- match
// LidarIris::GetHammingDistance (LidarIris.cpp:164-193) at every shift.  One workgroup = kEntries database entries x
// all 360 shifts: thread s holds shift s, walks the 360 columns, reads the query's column (c - s) mod 360 from LDS
// (word-major there: consecutive shifts read consecutive 8-byte words, no bank conflict) and the entries' column c
// through wave-uniform addresses.  total = 2 popcount(valid1 & valid2) (the mask counts for both halves); the
// block's argmin over s orders by (distance, s), NaN last.
__device__ inline int popc64(uint64_t v) { return __popcll(v); }

__global__ void __launch_bounds__(kThreads) k_iris_match(const uint64_t* __restrict__ db,
                                                         const uint64_t* __restrict__ q, int n_db,
                                                         float* __restrict__ out_dist, int* __restrict__ out_bias,
                                                         int* __restrict__ out_diff, int* __restrict__ out_total) {
    __shared__ uint64_t sq[kWords * kCols];
    __shared__ unsigned long long skey[kThreads];
    const int t = threadIdx.x;
    for (int i = t; i < kDescWords; i += kThreads) sq[(i % kWords) * kCols + i / kWords] = q[i];
    __syncthreads();
    const int e0 = blockIdx.x * kEntries;
    const uint64_t* ent[kEntries];
#pragma unroll
    for (int j = 0; j < kEntries; ++j) ent[j] = db + static_cast<size_t>(min(e0 + j, n_db - 1)) * kDescWords;
    const int s = t < kCols ? t : 0;
    int idx = s == 0 ? 0 : kCols - s;                      // (c - s) mod 360 at c = 0
    int diff[kEntries], val[kEntries];
#pragma unroll
    for (int j = 0; j < kEntries; ++j) diff[j] = val[j] = 0;
    for (int c = 0; c < kCols; ++c) {
        uint64_t qw[kWords];
#pragma unroll
        for (int w = 0; w < kWords; ++w) qw[w] = sq[w * kCols + idx];
#pragma unroll
        for (int j = 0; j < kEntries; ++j) {
            const uint64_t* d = ent[j] + c * kWords;
#pragma unroll
            for (int w = 0; w < kHalfWords; ++w) {
                const uint64_t v = qw[2 * kHalfWords + w] & d[2 * kHalfWords + w];
                val[j] += popc64(v);
                diff[j] += popc64((qw[w] ^ d[w]) & v) + popc64((qw[kHalfWords + w] ^ d[kHalfWords + w]) & v);
            }
        }
        idx = idx + 1 == kCols ? 0 : idx + 1;
    }
#pragma unroll
    for (int j = 0; j < kEntries; ++j) {
        const int total = 2 * val[j];
        const float dist = static_cast<float>(diff[j]) / static_cast<float>(total);   // total = 0: 0 / 0, unused
        // distances are >= +0, so their bit patterns order as the values do; NaN (total = 0) sorts last
        unsigned long long key = ~0ull;
        if (t < kCols)
            key = (static_cast<unsigned long long>(total ? __float_as_uint(dist) : 0xffffffffu) << 32) |
                  static_cast<unsigned>(t);
        __syncthreads();
        skey[t] = key;
        __syncthreads();
        for (int off = 256; off > 0; off >>= 1) {
            if (t < off && t + off < kThreads) skey[t] = min(skey[t], skey[t + off]);
            __syncthreads();
        }
        const unsigned long long best = skey[0];
        const int e = e0 + j;
        if (e < n_db) {
            if ((best >> 32) == 0xffffffffull) {           // every shift fully masked
                if (t == 0) {
                    out_dist[e] = __uint_as_float(0x7fc00000u);
                    out_bias[e] = -1;
                    out_diff[e] = 0;
                    out_total[e] = 0;
                }
            } else if (t == static_cast<int>(best & 0xffffffffull)) {
                out_dist[e] = dist;
                out_bias[e] = t;
                out_diff[e] = diff[j];
                out_total[e] = total;
            }
        }
    }
}

// The four log-Gabor kernels h_s = idft(F_s), unscaled: F_s[0] = 0, F_s[k] = exp(-ln^2((k / 360) / fo) / (2 ln^2 sigma))
// for k = 1..180 with fo = 1 / wavelength, F_s[181..359] = 0; wavelength 18, x mult per scale (LidarIris.cpp:95-130
// with the detector's nscale 4, minWaveLength 18, mult 2.1f, sigmaOnf 0.75f).
static void build_kernels(std::vector<double>& h) {
    h.assign(static_cast<size_t>(kScales) * kCols * 2, 0.0);
    const long double two_pi = 2.0L * acosl(-1.0L);
    const double mult = static_cast<double>(2.1f), sigma = static_cast<double>(0.75f);
    const double den = 2.0 * std::log(sigma) * std::log(sigma);
    double wavelength = 18.0;
    for (int s = 0; s < kScales; ++s) {
        const double fo = 1.0 / wavelength;
        long double F[kCols / 2 + 1];
        F[0] = 0.0L;
        for (int k = 1; k <= kCols / 2; ++k) {
            const double l = std::log((static_cast<double>(k) / kCols) / fo);
            F[k] = std::exp(-(l * l) / den);
        }
        for (int d = 0; d < kCols; ++d) {
            long double re = 0.0L, im = 0.0L;
            for (int k = 1; k <= kCols / 2; ++k) {
                const long double a = two_pi * static_cast<long double>((k * d) % kCols) / kCols;
                re += F[k] * cosl(a);
                im += F[k] * sinl(a);
            }
            h[(static_cast<size_t>(s) * kCols + d) * 2] = static_cast<double>(re);
            h[(static_cast<size_t>(s) * kCols + d) * 2 + 1] = static_cast<double>(im);
        }
        wavelength *= mult;
    }
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
    long long best = -1;
    for (size_t i = 0; i < n; ++i) {
        if (static_cast<int>(current_id) - static_cast<int>(ids[i]) < cfg->min_keyframe_gap) continue;
        const float dx = current_position[0] - positions[3 * i], dy = current_position[1] - positions[3 * i + 1],
                    dz = current_position[2] - positions[3 * i + 2];
        const float d = std::sqrt(dx * dx + dy * dy + dz * dz);
        if (d > cfg->max_search_distance) continue;
        if (std::isnan(dist[i])) continue;
        if (best < 0 || dist[i] < dist[best]) best = static_cast<long long>(i);
    }
    if (best >= 0 && dist[best] > cfg->similarity_threshold) best = -1;
    return best;
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
