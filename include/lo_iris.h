/*
 * lo_iris.h — C ABI of the MI355X-native LiDAR-Iris loop-closure detector: the producer of the loop candidates that
 * lo_icp_optimize_loop (lo_icp.h) verifies and lo_pgo.h closes.
 *
 * Replaces, for a host that keeps the reference's frame loop:
 *   LoopClosureDetector::add_keyframe / detect_loop_closures   (src/processing/LoopClosureDetector.cpp:44-202)
 *   LidarIris::GetIris / LoGFeatureEncode / GetHammingDistance  (thirdparty/LidarIris/LidarIris.cpp:4-19, :84-154, :164-193)
 * constructed as the detector constructs it: nscale 4, minWaveLength 18, mult 2.1f, sigmaOnf 0.75f, matchNum 2.
 *
 * The one departure from the reference (DESIGN.md "LiDAR-Iris loop detector"): LidarIris::Compare estimates the
 * column shift with a log-polar Fourier-Mellin registration (fftm.cpp: OpenCV remap / warpAffine / phaseCorrelate)
 * and evaluates the masked Hamming distance only at estimate-2 .. estimate+2, forward and reversed by 180 degrees.
 * Here the distance is evaluated at ALL 360 circular column shifts and the minimum is taken.  That set holds every
 * shift either direction of the reference can evaluate, so for every pair the distance reported here is <= the
 * reference's, and equal whenever the reference's estimate lies within +-2 of the best shift.
 * Everything else follows the reference's definitions; the encode is done in fp64 (the reference: OpenCV fp32 DFTs),
 * so a bit whose filter response is within rounding of its threshold can differ from an OpenCV build's.
 *
 * Conventions as lo_icp.h: an opaque handle created against a context (its device; its stream, looked up on every
 * call so lo_set_stream is followed), plain pointers and sizes, the caller owns every host buffer, LO_* return codes
 * (LO_INSUFFICIENT = "no" in the reference's bool / empty-vector sense), negative = errors with the text in
 * lo_iris_last_error.  Not thread-safe.  Every call is synchronous.  The context must outlive the handle.
 */
#ifndef LO_IRIS_H
#define LO_IRIS_H

#include <stddef.h>
#include <stdint.h>

#include "lo_icp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LO_IRIS_ROWS       80     /* range bins of the iris image (1 m each) */
#define LO_IRIS_COLS       360    /* yaw bins (1 degree each) */
#define LO_IRIS_FEAT_ROWS  640    /* rows of T and M: [Re of scales 0..3, Im of scales 0..3] x 80 */
#define LO_IRIS_BITS       230400 /* LO_IRIS_FEAT_ROWS * LO_IRIS_COLS */

/* LoopClosureConfig (LoopClosureDetector.h) as the frame loop uses it. */
typedef struct lo_iris_config {
    float similarity_threshold;   /* 0.3f: a candidate needs distance <= this */
    int   min_keyframe_gap;       /* 50: skip entries with (int)current_id - (int)entry_id < this */
    float max_search_distance;    /* 10.0f m: skip entries whose position is farther than this (fp32 norm) */
} lo_iris_config;

/* LoopCandidate. */
typedef struct lo_iris_candidate {
    int64_t query_keyframe_id;
    int64_t match_keyframe_id;
    float   distance;             /* similarity_score: masked Hamming distance at the best shift */
    int     bias;                 /* that shift, 0..359 */
} lo_iris_candidate;

typedef struct lo_iris lo_iris;

void        lo_iris_config_default(lo_iris_config* cfg);
/* capacity: database entries (keyframes), fixed; 43,200 B of device memory each. */
lo_iris*    lo_iris_create(lo_ctx* ctx, size_t capacity, int* err);
void        lo_iris_destroy(lo_iris* iris);
const char* lo_iris_last_error(const lo_iris* iris);
size_t      lo_iris_size(const lo_iris* iris);
size_t      lo_iris_capacity(const lo_iris* iris);
int         lo_iris_clear(lo_iris* iris);

/* ---- parity entry points (host in, host out) ----
 * GetIris: n AoS float3 points (sensor frame) -> the 80 x 360 uint8 image, row = range bin, column = yaw bin, bit =
 * height bin.  range bin floor(sqrtf(x*x + y*y)) clamped to 0..79; yaw bin floor(yaw + 0.5) clamped to 0..359 with
 * yaw = (float)(atan2f(y, x) * 180.0f / pi + 180) (the product in fp32, the quotient and sum in fp64, then the
 * reference's store to a float); height bit ceil(z + 5) clamped to 0..7.  Far points are clamped, not dropped.
 * n = 0 gives the all-zero image and LO_OK. */
int lo_iris_image(lo_iris* iris, const float* pts_xyz, size_t n, uint8_t* out_img /* 80*360 */);
/* LoGFeatureEncode of an 80 x 360 image: T and M, 640 x 360 uint8 each, 0 / 255 as the reference's Mat1b.
 * Row s*80 + r of T = (Re v > 0), row (4+s)*80 + r = (Im v > 0); both such rows of M = (|v| < 1e-4), where v is the
 * unscaled inverse DFT of (row r's 360-point DFT) x (the one-sided log-Gabor filter of scale s), in fp64. */
int lo_iris_encode(lo_iris* iris, const uint8_t* img, uint8_t* out_T, uint8_t* out_M);

/* ---- database ----
 * LoopClosureDetector::add_keyframe + the feature extraction detect_loop_closures does for it.  pts: host pointer,
 * or (on_device != 0) a device pointer on the context's device.  An empty cloud adds nothing and returns
 * LO_INSUFFICIENT (add_keyframe's false); LO_ERR_CAPACITY when the database is full. */
int lo_iris_add_keyframe(lo_iris* iris, int64_t keyframe_id, const float position[3], const float* pts_xyz, size_t n,
                         int on_device);
/* The same for the context's last device-filtered scan (lo_icp_optimize_raw / lo_odom_process: the keyframe's
 * feature cloud): read straight from the device buffer behind lo_filtered_points; only its 4-byte count is read
 * back.  LO_ERR_STATE when the context has no such scan. */
int lo_iris_add_from_scan(lo_iris* iris, int64_t keyframe_id, const float position[3]);

/* ---- matching ----
 * The query cloud's descriptor against every database entry i (in insertion order) at every shift s in 0..359:
 * with T1s, M1s the QUERY's T and M rolled right by s columns (circShift(., 0, s): column c of the rolled image is
 * column (c - s) mod 360 of the original) and T2, M2 the entry's,
 *   mask = M1s | M2;  total = 230400 - popcount(mask);  diff = popcount((T1s ^ T2) & ~mask);
 *   distance = diff / (float)total (one fp32 division), NaN when total = 0.
 * out_dist[i] = the minimum over s (NaN only if every shift is NaN), out_bias[i] = the smallest s that attains it
 * (-1 when every shift is NaN, as GetHammingDistance leaves it), out_diff[i] / out_total[i] = diff and total at that
 * shift (0 / 0 for NaN).  Sign: an entry whose scene is the query's scene turned by +a degrees about z as seen from
 * the sensor (its points are R_z(a) * the query's) reports bias = a mod 360.  Any output pointer may be NULL.
 * An empty query cloud returns LO_INSUFFICIENT and writes nothing. */
int lo_iris_compare_all(lo_iris* iris, const float* pts_xyz, size_t n, int on_device, float* out_dist,
                        int32_t* out_bias, int32_t* out_diff, int32_t* out_total);

/* detect_loop_closures for the current keyframe (which is NOT added: call lo_iris_add_keyframe for it afterwards,
 * as the frame loop does): lo_iris_compare_all, then lo_iris_select_host over the database's ids and positions.
 * LO_OK with *candidate filled, or LO_INSUFFICIENT for none (empty cloud, empty database, nothing passes). */
int lo_iris_detect(lo_iris* iris, const lo_iris_config* cfg, int64_t keyframe_id, const float position[3],
                   const float* pts_xyz, size_t n, int on_device, lo_iris_candidate* candidate);

/* The selection rule alone (context-free, host-only, no GPU needed).  Entry i is skipped when
 * (int)current_id - (int)ids[i] < min_keyframe_gap, when the fp32 norm of (current_position - positions[3i..]) is
 * > max_search_distance, or when dist[i] is NaN.  Among the rest the lowest dist wins, ties to the lower index; it is
 * returned only if dist <= similarity_threshold.  Returns the index, or -1 for none. */
long long lo_iris_select_host(const lo_iris_config* cfg, int64_t current_id, const float current_position[3],
                              const int64_t* ids, const float* positions, const float* dist, size_t n);

/* Timing harness (scripts/iris_bench.py): reps back-to-back launches of the match kernel, the last query against
 * the current database; average device time per launch (HIP events). */
int lo_iris_bench_match(lo_iris* iris, int reps, float* avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* LO_IRIS_H */
