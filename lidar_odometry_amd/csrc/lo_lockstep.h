// lo_lockstep.h — the launch list of a lockstep run: the first `nfast + nexl` jobs of a device KParams array advance
// through every GN iteration together, one launch per kernel per iteration for all of them (blockIdx.y = job).  One
// body, two callers: the scan-parallel batch (lo_batch.hip: B contexts, one job each) and the scan queue's groups
// (lo_scanq.hip: G queued scans of one context, each on its own set of per-scan state).
//
// Job order in the array: the fast-mode jobs, then the reference-exact ones (each at most kExactMergeMax points: their
// iteration-0 scale is k_exact_scale_cb's one workgroup per job).  Nothing here synchronises with the host, and nothing
// is speculative: k_pko_tb picks alpha, then k_exact_acc_b (exact jobs) or k_accumulate_b* / k_solve_b* (fast jobs)
// form the one set of sums the step needs.
#pragma once
#include <algorithm>

#include "lo_kernels_decl.h"

namespace lo {
// KDTree runs, the unresolved pass (k_knn_brute_b): at most this many 1024-thread workgroups over all jobs (two per
// CU), and at most kLockstepBrutePerJob of them on one job (what a single context's k_knn_brute launch gets)
constexpr int kLockstepBruteWGs = 512;
constexpr int kLockstepBrutePerJob = 64;

struct LockstepShape {
    int nfast = 0, nexl = 0;        // fast-mode jobs, then reference-exact jobs
    int max_nb = 1;                 // the largest job's k_correspond grid
    int max_knn = 1;                //   and its k_knn grid (KDTree runs)
    int max_acc = 1;                // the largest fast job's accumulate grid (KParams::nb_acc)
    int n_max_ex = 1;               // the largest exact job's point count
    bool kd = false;                // KDTree correspondence: k_knn_b + k_knn_brute_b + k_plane_b per iteration
    int pko_wgs = 1;                // PKO workgroups per job (the caller's budget / jobs, capped by the alpha grid)
    bool one_wave = false;          // one single-wave PKO workgroup per job (k_pko_tb<1, true>)
    bool split_solve = false;       // small fast jobs: k_accumulate_b1<false> + k_solve_b1 instead of the fused form
};

// The correspondence stage of one lockstep iteration: the surfel lookup, or (KDTree) the grid search, the unresolved
// queries and the plane fit, each one launch for all jobs.
inline void launch_lockstep_correspond(hipStream_t s, const KParams* d_P, const LockstepShape& L, int with_stats, int init) {
    const int nact = L.nfast + L.nexl;
    const dim3 blk(kBlock);
    if (!L.kd) {
        hipLaunchKernelGGL(k_correspond_b, dim3(L.max_nb, nact), blk, 0, s, d_P, with_stats, init);
        return;
    }
    const int per = std::max(1, std::min(kLockstepBrutePerJob, kLockstepBruteWGs / nact));
    const int wgs = static_cast<int>(std::min<long long>(kLockstepBruteWGs, static_cast<long long>(nact) * per));
    hipLaunchKernelGGL(k_knn_b, dim3(L.max_knn, nact), blk, 0, s, d_P, init);
    hipLaunchKernelGGL(k_knn_brute_b, dim3(wgs), dim3(1024), 0, s, d_P, nact, per);
    hipLaunchKernelGGL(k_plane_b, dim3(L.max_nb, nact), blk, 0, s, d_P, with_stats);
}

// Every GN iteration of the run.  Returns the first launch error (e.g. a dynamic-LDS launch whose attribute was not
// set: the caller sets those of k_pko_tb, k_exact_acc_b and the exact scale once, before its first run).
inline hipError_t launch_lockstep(hipStream_t s, const KParams* d_P, const LockstepShape& L, int max_iters) {
    const int nact = L.nfast + L.nexl;
    if (nact <= 0) return hipSuccess;
    const size_t pre_bytes = static_cast<size_t>(L.max_nb) * sizeof(int);
    const dim3 blk(kBlock);
    for (int it = 0; it < max_iters; ++it) {
        launch_lockstep_correspond(s, d_P, L, it == 0 ? 1 : 0, it == 0 ? 1 : 0);
        if (it == 0 && L.nexl > 0) {
            launch_exact_scale_cb(d_P + L.nfast, L.nexl, L.n_max_ex, s);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        if (L.one_wave)
            hipLaunchKernelGGL((k_pko_tb<1, true>), dim3(1, nact), dim3(64), pre_bytes, s, d_P, it);
        else
            hipLaunchKernelGGL((k_pko_tb<4, false>), dim3(L.pko_wgs, nact), dim3(256), pre_bytes, s, d_P, it);
        if (L.nexl > 0)
            hipLaunchKernelGGL(k_exact_acc_b, dim3(L.nexl), dim3(256), kXcLdsBytes, s, d_P + L.nfast, it);
        if (L.nfast == 0) continue;
        if (L.max_acc <= kFuseMaxBlocks) {             // small jobs: one 8-wave workgroup accumulates + solves
            if (!L.split_solve) {
                hipLaunchKernelGGL(k_accumulate_b1<true>, dim3(1, L.nfast), dim3(512), 0, s, d_P, it);
            } else {
                hipLaunchKernelGGL(k_accumulate_b1<false>, dim3(1, L.nfast), dim3(512), 0, s, d_P, it);
                hipLaunchKernelGGL(k_solve_b1, dim3(L.nfast), dim3(kBlock), 0, s, d_P, it);
            }
        } else {
            hipLaunchKernelGGL(k_accumulate_b, dim3(L.max_acc, L.nfast), blk, 0, s, d_P, it);
            hipLaunchKernelGGL(k_solve_b, dim3(L.nfast), dim3(kSolveThreads), 0, s, d_P, it);
        }
    }
    return hipGetLastError();
}

// What a lockstep caller sets once per process before its first run: the dynamic-LDS attributes of the kernels above.
inline hipError_t lockstep_prepare() {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pko_tb<4, false>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(kMaxBlocks * sizeof(int)));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pko_tb<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(kMaxBlocks * sizeof(int)));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_exact_acc_b), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(kXcLdsBytes));
    if (e != hipSuccess) return e;
    // reference-exact jobs' iteration-0 scale (k_exact_scale_cb, up to 80 KB of dynamic LDS): a process that only runs
    // lockstep must not depend on a single-context exact optimize having set the attribute first
    return exact_scale_c_prepare();
}
}  // namespace lo
