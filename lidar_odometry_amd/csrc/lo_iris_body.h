// lo_iris_body.h — what the solo detector (lo_iris.hip) and the batched one (lo_iris_batch.hip) share: the descriptor
// layout, the device bodies of the image, encode and match kernels, the log-Gabor kernels and the selection rule.
// Each kernel of either file is a thin shell around one of these bodies, so the two detectors cannot drift apart.
//
// Packed descriptor (kDescWords 64-bit words = 43,200 B): column-major, 15 words per image column:
//   words 0..4   Re bits  (bit p = r * 4 + s of the column: range row r, scale s -- 320 bits)
//   words 5..9   Im bits  (same order)
//   words 10..14 VALID bits = ~M (same order; M's two halves are identical, so one copy serves Re and Im)
// The 640-row axis lies inside the words, so a circular column shift is an index rotation over whole 120-byte
// columns, and the row order inside a column (any fixed permutation) does not change a popcount.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/lo_iris.h"

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
// LidarIris::GetIris (LidarIris.cpp:4-19) for the points first, first + step, ... of pts.
__device__ inline void image_points(const float* __restrict__ pts, int n, uint32_t* __restrict__ img, int first,
                                    int step) {
    for (int i = first; i < n; i += step) {
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
// LogGaborFilter + LoGFeatureEncode (LidarIris.cpp:84-154) for image row r and scale s, by one workgroup of kThreads.
// idft(dft(x) . F_s) is the circular convolution of x with h_s = idft(F_s) (unscaled, as cv::idft without DFT_SCALE);
// h (4 x 360 complex, fp64) is built on the host, so one pass of 360 x 360 real-by-complex products per (row, scale)
// gives the response directly; zero cells (most of an iris image) are skipped, which is exact.  desc must be zero.
__device__ inline void encode_row(const uint32_t* __restrict__ img, const double2* __restrict__ h,
                                  uint32_t* __restrict__ desc, int r, int s) {
    __shared__ double sx[kCols];
    __shared__ double2 sh[kCols];
    const int t = threadIdx.x;
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
// LidarIris::GetHammingDistance (LidarIris.cpp:164-193) at every shift, by one workgroup of kThreads: the query q
// against the kEntries database entries ent[] x all 360 shifts.  Thread s holds shift s, walks the 360 columns, reads
// the query's column (c - s) mod 360 from LDS (word-major there: consecutive shifts read consecutive 8-byte words, no
// bank conflict) and the entries' column c through wave-uniform addresses.  total = 2 popcount(valid1 & valid2) (the
// mask counts for both halves); the block's argmin over s orders by (distance, s), NaN last.  For each entry j exactly
// one thread calls out(j, dist, bias, diff, total): (NaN, -1, 0, 0) when every shift is fully masked.
__device__ inline int popc64(uint64_t v) { return __popcll(v); }

template <class Out>
__device__ inline void match_block(const uint64_t* __restrict__ q, const uint64_t* const (&ent)[kEntries], Out&& out) {
    __shared__ uint64_t sq[kWords * kCols];
    __shared__ unsigned long long skey[kThreads];
    const int t = threadIdx.x;
    for (int i = t; i < kDescWords; i += kThreads) sq[(i % kWords) * kCols + i / kWords] = q[i];
    __syncthreads();
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
        if ((best >> 32) == 0xffffffffull) {               // every shift fully masked
            if (t == 0) out(j, __uint_as_float(0x7fc00000u), -1, 0, 0);
        } else if (t == static_cast<int>(best & 0xffffffffull)) {
            out(j, dist, t, diff[j], total);
        }
    }
}

// The four log-Gabor kernels h_s = idft(F_s), unscaled: F_s[0] = 0, F_s[k] = exp(-ln^2((k / 360) / fo) / (2 ln^2 sigma))
// for k = 1..180 with fo = 1 / wavelength, F_s[181..359] = 0; wavelength 18, x mult per scale (LidarIris.cpp:95-130
// with the detector's nscale 4, minWaveLength 18, mult 2.1f, sigmaOnf 0.75f).
inline void build_kernels(std::vector<double>& h) {
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

// ---------------------------------------------------------------------------------------------------- selection
// The candidate rule of LoopClosureDetector::detect_loop_closures (lo_iris_select_host, lo_iris.h), in two parts so
// that the batched detector can apply the first before it matches anything and the second to what it matched.
// eligible(): the tests that need no distance -- the keyframe gap and the fp32 position norm.
inline bool eligible(const lo_iris_config& cfg, int64_t current_id, const float current_position[3], int64_t id,
                     const float position[3]) {
    if (static_cast<int>(current_id) - static_cast<int>(id) < cfg.min_keyframe_gap) return false;
    const float dx = current_position[0] - position[0], dy = current_position[1] - position[1],
                dz = current_position[2] - position[2];
    const float d = std::sqrt(dx * dx + dy * dy + dz * dz);
    return !(d > cfg.max_search_distance);
}

// Best: the eligible entries' distances offered in index order -- NaN skipped, the lowest wins, ties to the lower
// index; pick() returns the index only if its distance is <= the threshold, else -1.
struct Best {
    long long index = -1;
    float dist = 0.0f;
    void offer(long long i, float d) {
        if (std::isnan(d)) return;
        if (index < 0 || d < dist) { index = i; dist = d; }
    }
    long long pick(const lo_iris_config& cfg) const { return index >= 0 && dist > cfg.similarity_threshold ? -1 : index; }
};

}  // namespace iris
}  // namespace lo
