// lo_kernels_decl.h — forward declarations of the kernels and launch helpers defined in lo_kernels.hip, lo_pko.hip,
// lo_exact.hip and lo_kdtree.hip, for the host translation units that launch them (through lo_ctx_def.h).
#pragma once
#include <hip/hip_runtime.h>

#include "lo_device.h"
#include "lo_seqsum.h"

namespace lo {
__global__ void k_correspond(KParams P, int with_stats);
template <int NW> __global__ void k_pko_t(KParams P, int it, int G);
__global__ void k_pko_tx(KParams P, int it, int G);
__global__ void k_pko_finish(KParams P);
__global__ void k_accumulate(KParams P, int it, int fuse);
__global__ void k_solve(KParams P, int it, int ne_only);
__global__ void k_solve_pick(KParams P, int it);
__global__ void k_solve_correspond(KParams P, int it);
__global__ void k_solve_knn(KParams P, int it);
__global__ void k_pick_knn(KParams P, int it);
__global__ void k_pick_correspond(KParams P, int it);
__global__ void k_pick(KParams P, int it);
struct Pose12 { float v[12]; };
__global__ void k_init(DevState* st, Pose12 T, double scale, double alpha);
__global__ void k_export_pose(const DevState* st, float* out);
__global__ void k_wait_seq(uint32_t* fin, uint32_t seq, DevState* st, uint32_t* hbroken, unsigned long long bound);
__global__ void k_wait_final(uint32_t* fin, uint32_t seq, DevState* st, uint32_t* hbroken, unsigned long long bound);
__global__ void k_signal_main(uint32_t* fin, uint32_t seq);
__global__ void k_knn(KParams P);
__global__ void k_knn_brute(KParams P);
__global__ void k_knn_brute_w(KParams P);
__global__ void k_knn_all(KParams P);
__global__ void k_pick_knn_all(KParams P, int it);
__global__ void k_inlier_all(KParams P);
__global__ void k_knn_reset(KParams P);
__global__ void k_plane(KParams P, int with_stats);
__global__ void k_inlier(KParams P);
__global__ void k_correspond_b(const KParams* PB, int with_stats, int init);
__global__ void k_knn_b(const KParams* PB, int init);
__global__ void k_knn_brute_b(const KParams* PB, int njobs, int per);
__global__ void k_plane_b(const KParams* PB, int with_stats);
__global__ void k_knn_all_b(const KParams* PB, int init);
__global__ void k_inlier_all_b(const KParams* PB, const int* sel);
__global__ void k_inlier_b(const KParams* PB, const int* sel);
template <int NW, bool ONE_WAVE> __global__ void k_pko_tb(const KParams* PB, int it);
__global__ void k_accumulate_b(const KParams* PB, int it);
template <bool SOLVE> __global__ void k_accumulate_b1(const KParams* PB, int it);
__global__ void k_solve_b1(const KParams* PB, int it);
__global__ void k_solve_b(const KParams* PB, int it);
__global__ void k_export_batch(const KParams* PB, lo_batch_rec* out);
__global__ void k_exact_acc_b(const KParams* PB, int it);
__global__ void k_export_group(const KParams* PB, int njobs, uint32_t* hdone, uint32_t seq);
void launch_exact_scale_cb(const KParams* PB, int njobs, int n_max, hipStream_t s);
struct MapPatchRec;
__global__ void k_map_patch(Slot* tab, uint32_t log2cap, const MapPatchRec* rec, int n);
struct FitJob {
    uint64_t key;
    int32_t off, m;
};
struct FitOut;
__global__ void k_surfel_fit(const FitJob* jobs, const float* cs, int n, float thr, Slot* tab, uint32_t log2cap,
                             FitOut* out);
void launch_exact_scale(const KParams& P, int n, double* sorted, hipStream_t s);
hipError_t exact_scale_rank_prepare();
hipError_t exact_scale_c_prepare();
void launch_exact_scale_c(const KParams& P, hipStream_t s);
void launch_seq_sum_diag(const double* x, int n, double* sort, double* out, long long* stats, hipStream_t s);
void launch_mw_sums(const float* col0, int ld, int ncol, int n_cap, const int* n_dev, const DevState* st, const MwBuf& B,
                    float* out, long long* stats, hipStream_t s, bool factored);
size_t mw_bytes(int ncol, int n_cap);
MwBuf mw_layout(void* mem, int ncol, int n_cap);
hipError_t mw_clear(const MwBuf& B, int ncol, hipStream_t s);
void launch_mwm_scale(KParams P, const double* sorted, const MwmBuf& B, hipStream_t s);
size_t mwm_bytes(int n_cap);
MwmBuf mwm_layout(void* mem, int n_cap);
__global__ void k_exact_resid(KParams P, double* out);
__global__ void k_exact_terms(KParams P);
__global__ void k_exact_solve(KParams P, int it);
__global__ void k_exact_finish(KParams P, int it);
}  // namespace lo
