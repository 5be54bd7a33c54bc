// lo_batch_loop.hip — the batched loop-closure ICP: lo_batch_optimize_loop_dev, lo_icp_optimize_loop_dev for many jobs
// of a batch in one lockstep run (IterativeClosestPointOptimizer::optimize_loop, :40-251, once per job).
//
// The conventions are lo_batch.hip's: one KParams per lockstep job in a device array, blockIdx.y = job or
// batch_block's linearisation, a job's surplus blocks leave before touching its buffers, a finished job
// (DevState::done) leaves at once.  Slot order: fast all-pairs | fast cell-grid | exact cell-grid | exact all-pairs, so
// the fast jobs, the exact jobs and the cell-grid jobs (n_matched > kKnnAllMax) are each one contiguous range.  Per call:
//   k_cloud_world_b   every job's matched cloud into the world: float4 into its context's loop grid (all-pairs jobs),
//                     float3 into its d_lworld (cell-grid jobs); a per-job word flags a non-finite point
//   cell-grid jobs    batch_loop_grids_from_device (lo_grid.hip): the batch grid builder on each context's lgrid with
//                     the loop path's occupancy rule, one readback + synchronise per tried cell edge for all jobs
//   per GN iteration  k_knn_all_b (all-pairs jobs; the others leave), k_knn_b + k_knn_brute_b over the cell-grid range,
//                     k_plane_b, (iteration 0, exact jobs) k_exact_scale_cb, k_pko_tb, then k_exact_acc_b (exact jobs)
//                     and k_accumulate_b* / k_solve_b* (fast jobs): the lockstep forms of lo_batch_optimize_async
//   per chunk of 4    k_loop_heads: every job's head (done, status, iter, n_corr, pose, kd_tie, ...) into one array,
//                     one device-to-host copy and one synchronise for the whole batch
//   once              k_inlier_all_b / k_inlier_b over the converged jobs, k_loop_heads, k_loop_logs (the executed
//                     iterations' logs packed back to back), one copy
// T_rel and the inlier ratio are formed on the host by loop_solve's own statements.  A reference-exact job beyond
// kExactMergeMax points (no lockstep form, as in lo_batch_optimize_async) and a job that met a deciding distance tie
// run through the solo code on their own context inside the call.
#include "lo_ctx_def.h"

#include <climits>

namespace lo {
constexpr int kLoopIters = 100;                      // optimize_loop's iteration limit (:74), as loop_solve
constexpr int kLoopChunkB = 4;                       // iterations between two reads of the jobs' heads, as loop_solve
constexpr int kLoopMinCell = 4;                      // the matched cloud's grid: >= 4 points per occupied cell, as loop_solve
constexpr int kLoopPkoWGs = 256;                     // PKO workgroups per launch over all jobs (lo_batch.hip's budget)
constexpr int kLoopSplitSolveMin = 1024;             // fast jobs from which k_solve_b1 solves (lo_batch.hip)
constexpr int kLoopBruteWGs = 512, kLoopBrutePerJob = 64;   // k_knn_brute_b's grid (lo_batch.hip)

struct LoopCloud {
    const float* in;                 // the matched cloud, sensor frame
    int n;
    float T[12];                     // its world pose
    float4* out4;                    // all-pairs job: the context's loop grid, (x, y, z, index) in index order
    float* out3;                     // cell-grid job: the world cloud the grid is built from; both null: check only
};
struct LoopHead {
    int done, status, iter, n_corr;
    float pose[12];
    unsigned kd_tie, inliers;
    float initial_cost, final_cost;
};

// transform_point_cloud (transform_pt's order) for every job's matched cloud, as k_cloud_world.  words: three per-slot
// arrays of gridDim.y words -- [0] raised by a non-finite world point, [1] receives the count (the device count the
// grid builder reads), [2] the grid builder's occupied-cell counter.
__global__ __launch_bounds__(kBlock) void k_cloud_world_b(const LoopCloud* __restrict__ jobs, uint32_t* __restrict__ words) {
    const LoopCloud& J = jobs[blockIdx.y];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) words[gridDim.y + blockIdx.y] = static_cast<uint32_t>(J.n);
    if (i >= J.n) return;
    float wx, wy, wz;
    transform_pt(J.T, J.in[3 * static_cast<size_t>(i)], J.in[3 * static_cast<size_t>(i) + 1],
                 J.in[3 * static_cast<size_t>(i) + 2], wx, wy, wz);
    if (!(isfinite(wx) && isfinite(wy) && isfinite(wz))) atomicOr(&words[blockIdx.y], 1u);
    if (J.out4) {
        J.out4[i] = make_float4(wx, wy, wz, __int_as_float(i));
    } else if (J.out3) {
        J.out3[3 * static_cast<size_t>(i)] = wx;
        J.out3[3 * static_cast<size_t>(i) + 1] = wy;
        J.out3[3 * static_cast<size_t>(i) + 2] = wz;
    }
}

// One thread per job: the head of its GN state.
__global__ __launch_bounds__(kWave) void k_loop_heads(const KParams* __restrict__ PB, int njobs, LoopHead* __restrict__ heads) {
    const int a = blockIdx.x * kWave + threadIdx.x;
    if (a >= njobs) return;
    const DevState* st = PB[a].st;
    LoopHead H;
    H.done = st->done; H.status = st->status; H.iter = st->iter; H.n_corr = st->n_corr;
    for (int k = 0; k < 12; ++k) H.pose[k] = st->pose[k];
    H.kd_tie = st->kd_tie; H.inliers = st->inliers;
    const int last = min(H.iter, LO_MAX_ITERS) - 1;
    H.initial_cost = H.iter > 0 ? st->logs[0].cost : 0.0f;
    H.final_cost = last >= 0 ? st->logs[last].cost : 0.0f;
    heads[a] = H;
}
// One wave per job: its executed iterations' logs to out + off[job] (off < 0: none wanted; the host sized the offsets
// from the heads it read after the last chunk, and nothing has run on the jobs' logs since).
__global__ __launch_bounds__(kWave) void k_loop_logs(const KParams* __restrict__ PB, const int* __restrict__ off,
                                                     lo_iter_log* __restrict__ out) {
    const int a = blockIdx.x;
    if (off[a] < 0) return;
    const DevState* st = PB[a].st;
    const int iters = min(max(st->iter, 0), LO_MAX_ITERS);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(st->logs);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out + off[a]);
    const int words = iters * static_cast<int>(sizeof(lo_iter_log) / sizeof(uint32_t));
    for (int w = threadIdx.x; w < words; w += kWave) dst[w] = src[w];
}

struct LoopBatch {
    int device = 0;
    DevBuf<KParams> d_P;
    PinnedBuf<KParams> h_P;
    DevBuf<float> d_T0;
    PinnedBuf<float> h_T0;
    DevBuf<LoopCloud> d_cl;
    PinnedBuf<LoopCloud> h_cl;
    DevBuf<uint32_t> d_words;        // 3 words per slot (k_cloud_world_b); later the selections / the log offsets
    PinnedBuf<uint32_t> h_words;
    DevBuf<LoopHead> d_head;
    PinnedBuf<LoopHead> h_head;
    DevBuf<lo_iter_log> d_logs;
    PinnedBuf<lo_iter_log> h_logs;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool attr = false;
};
static void lb_release(void* p) {
    LoopBatch* S = static_cast<LoopBatch*>(p);
    (void)hipSetDevice(S->device);
    if (S->ev0) (void)hipEventDestroy(S->ev0);
    if (S->ev1) (void)hipEventDestroy(S->ev1);
    delete S;
}
static size_t lb_all_lds(int m) { return static_cast<size_t>((std::max(m, 1) + 511) / 512 * 512) * sizeof(float4); }   // all_padded
static int lb_all_blocks(int n) { return (std::max(n, 1) + kAllThreads / kWave - 1) / (kAllThreads / kWave); }
static int lb_knn_blocks(int n) { return static_cast<int>((static_cast<long long>(n) * kKnnGroup + kBlock - 1) / kBlock); }

// a record from the solo entry's outputs (T_rel and the ratio were written in place)
static void lb_rec_from_stats(lo_loop_rec& R, int rc, const lo_stats& st) {
    R.status = rc;
    R.converged = st.converged;
    R.iterations = st.iterations;
    R.n_corr = st.n_corr;
    R.initial_cost = static_cast<float>(st.initial_cost);
    R.final_cost = static_cast<float>(st.final_cost);
}
}  // namespace lo

extern "C" int lo_batch_optimize_loop_dev(lo_batch* b, const lo_loop_job* jobs, int count, lo_loop_rec* out,
                                          lo_iter_log* logs, double* gpu_ms) {
    if (!b) return LO_ERR_ARG;
    struct Err { std::string err; lo_batch* b; ~Err() { if (!err.empty()) batch_set_error(b, err.c_str()); } } err_{{}, b}, *e = &err_;
    auto fail = [&](int rc, int i, const std::string& msg) {
        e->err = (i >= 0 ? "job " + std::to_string(jobs[i].job) + " (entry " + std::to_string(i) + "): " : std::string()) + msg;
        return rc;
    };
    if (count < 0) return fail(LO_ERR_ARG, -1, "negative job count");
    if (count > 0 && (!jobs || !out)) return fail(LO_ERR_ARG, -1, "null jobs or out array");
    const BatchView V = batch_view(b);
    if (V.pending) return fail(LO_ERR_STATE, -1, "batch in flight: call lo_batch_result first");
    if (gpu_ms) *gpu_ms = 0.0;
    if (count == 0) return LO_OK;
    {
        std::vector<char> seen(static_cast<size_t>(V.count), 0);
        for (int i = 0; i < count; ++i) {
            const lo_loop_job& J = jobs[i];
            if (J.job < 0 || J.job >= V.count) {
                e->err = "entry " + std::to_string(i) + ": job index " + std::to_string(J.job) + " out of range";
                return LO_ERR_ARG;
            }
            if (seen[J.job]) return fail(LO_ERR_ARG, i, "job listed twice");
            seen[J.job] = 1;
            if ((J.n_curr > 0 && !J.d_curr) || (J.n_matched > 0 && !J.d_matched))
                return fail(LO_ERR_ARG, i, "null cloud pointer with a non-zero count");
            if (J.n_matched > static_cast<size_t>(INT32_MAX / 2)) return fail(LO_ERR_CAPACITY, i, "too many map points");
        }
        for (int i = 0; i < count; ++i)
            if (jobs[i].n_curr > static_cast<size_t>(V.ctx[jobs[i].job]->cfg.max_points))
                return fail(LO_ERR_CAPACITY, i, "n_curr exceeds max_points");
    }
    LO_HIP(e, hipSetDevice(V.device));
    for (int i = 0; i < count; ++i) {                        // a queued single scan's pending hold first (scan overlap)
        lo_ctx* c = V.ctx[jobs[i].job];
        if (flush_hold(c) != LO_OK) return fail(LO_ERR_HIP, i, c->err);
    }
    void** slot = batch_loop_state(b, lb_release);
    if (!*slot) {
        LoopBatch* S = new LoopBatch();
        S->device = V.device;
        *slot = S;                                           // owned by the batch from here on
    }
    LoopBatch* S = static_cast<LoopBatch*>(*slot);
    hipStream_t bs = static_cast<hipStream_t>(V.stream);

    // the classes: empty jobs report at once; a large exact job runs lo_icp_optimize_loop_dev on its context; the rest
    // in lockstep, in the slot order above
    std::vector<int> cls[4], solo;                           // fast all-pairs, fast grid, exact grid, exact all-pairs
    for (int i = 0; i < count; ++i) {
        lo_loop_rec& R = out[i];
        R.status = LO_INSUFFICIENT;
        R.converged = R.iterations = R.n_corr = R.rerun = 0;
        R.initial_cost = R.final_cost = 0.0f;
        const lo_loop_job& J = jobs[i];
        if (J.n_curr == 0 || J.n_matched == 0) continue;             // empty clouds: 0 correspondences (:477-483)
        const lo_ctx* c = V.ctx[J.job];
        const bool grid = J.n_matched > static_cast<size_t>(kKnnAllMax);
        if (c->exact && J.n_curr > static_cast<size_t>(kExactMergeMax)) solo.push_back(i);
        else cls[c->exact ? (grid ? 2 : 3) : (grid ? 1 : 0)].push_back(i);
    }
    std::vector<int> lock;
    for (const auto& v : cls) lock.insert(lock.end(), v.begin(), v.end());
    const int nact = static_cast<int>(lock.size()), nsolo = static_cast<int>(solo.size()), nslot = nact + nsolo;
    const int nfast = static_cast<int>(cls[0].size() + cls[1].size()), nexl = nact - nfast;
    const int g0 = static_cast<int>(cls[0].size()), ngrid = static_cast<int>(cls[1].size() + cls[2].size());
    const int nall = nact - ngrid;
    if (nslot == 0) return LO_OK;
    const size_t A = static_cast<size_t>(nslot);

    if (!S->ev0) LO_HIP(e, hipEventCreate(&S->ev0));
    if (!S->ev1) LO_HIP(e, hipEventCreate(&S->ev1));
    if (!S->attr) {
        for (const void* f : {reinterpret_cast<const void*>(&k_knn_all_b), reinterpret_cast<const void*>(&k_inlier_all_b)})
            LO_HIP(e, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kKnnAllMax * sizeof(float4)));
        S->attr = true;
    }
    LO_HIP(e, S->d_P.reserve(A));
    LO_HIP(e, S->h_P.reserve(A));
    LO_HIP(e, S->d_T0.reserve(12 * A));
    LO_HIP(e, S->h_T0.reserve(12 * A));
    LO_HIP(e, S->d_cl.reserve(A));
    LO_HIP(e, S->h_cl.reserve(A));
    LO_HIP(e, S->d_words.reserve(3 * A));
    LO_HIP(e, S->h_words.reserve(3 * A));
    LO_HIP(e, S->d_head.reserve(A));
    LO_HIP(e, S->h_head.reserve(A));

    // ---- the local maps.  Per-context buffers first: the contexts are idle, as for every batch call; a buffer that
    // has to grow is the one case that waits for the context's stream (what it enqueued last may still read the old
    // block).  A large exact job's slot only checks its cloud here: a non-finite point of any job ends the call
    // before any GN launch.
    int max_m = 1, max_all_m = 1;
    for (int a = 0; a < nslot; ++a) {
        const int i = a < nact ? lock[a] : solo[a - nact];
        const lo_loop_job& J = jobs[i];
        lo_ctx* c = V.ctx[J.job];
        LoopCloud& L = S->h_cl[a];
        L.in = J.d_matched;
        L.n = static_cast<int>(J.n_matched);
        std::memcpy(L.T, J.T_matched, sizeof(L.T));
        L.out4 = nullptr;
        L.out3 = nullptr;
        max_m = std::max(max_m, L.n);
        if (a >= nact) continue;
        int rc = kd_alloc(c);
        if (rc == LO_OK) rc = ensure_acc_part(c);
        if (rc != LO_OK) return fail(rc, i, c->err);
        const bool grid = a >= g0 && a < g0 + ngrid;
        if (grid) {
            if (3 * J.n_matched > c->d_lworld.capacity()) {
                LO_HIP(e, hipStreamSynchronize(c->stream));
                LO_HIP(e, c->d_lworld.reserve(3 * J.n_matched));
            }
            L.out3 = c->d_lworld;
        } else {
            if (J.n_matched > c->lgrid.d_pts.capacity()) {
                LO_HIP(e, hipStreamSynchronize(c->stream));
                LO_HIP(e, c->lgrid.d_pts.reserve(J.n_matched));
            }
            L.out4 = c->lgrid.d_pts;
            max_all_m = std::max(max_all_m, L.n);
        }
    }
    LO_HIP(e, hipEventRecord(S->ev0, bs));
    LO_HIP(e, hipMemsetAsync(S->d_words, 0, sizeof(uint32_t) * 3 * A, bs));
    LO_HIP(e, hipMemcpyAsync(S->d_cl, S->h_cl, sizeof(LoopCloud) * A, hipMemcpyHostToDevice, bs));
    hipLaunchKernelGGL(k_cloud_world_b, dim3((max_m + kBlock - 1) / kBlock, nslot), dim3(kBlock), 0, bs, S->d_cl.get(),
                       S->d_words.get());
    LO_HIP(e, hipGetLastError());
    LO_HIP(e, hipMemcpyAsync(S->h_words, S->d_words, sizeof(uint32_t) * A, hipMemcpyDeviceToHost, bs));
    {
        // the cell-grid jobs' grids (with none: the synchronise and the test of the words alone)
        std::vector<LoopGridSrc> gs;
        for (int a = g0; a < g0 + ngrid; ++a) {
            const lo_loop_job& J = jobs[lock[a]];
            lo_ctx* c = V.ctx[J.job];
            gs.push_back(LoopGridSrc{c, c->d_lworld, reinterpret_cast<const int*>(S->d_words + A + a), S->d_words + 2 * A + a,
                                     J.n_matched, J.job});
        }
        int bad = -1;
        std::string gerr;
        const int rc = batch_loop_grids_from_device(b, gs.data(), ngrid, kLoopMinCell, S->h_words, nslot, &bad, &gerr);
        if (rc != LO_OK) return fail(rc, bad >= 0 ? (bad < nact ? lock[bad] : solo[bad - nact]) : -1, gerr);
    }

    if (nact > 0) {
        // ---- the jobs' parameters, exactly as loop_solve fills them
        int max_nb = 1, max_acc = 1, n_max_ex = 1, max_all = 1, max_knn = 1, pko_max = kPkoMaxWGs;
        for (int a = 0; a < nact; ++a) {
            const lo_loop_job& J = jobs[lock[a]];
            lo_ctx* c = V.ctx[J.job];
            PointGrid& G = c->lgrid;
            const bool grid = a >= g0 && a < g0 + ngrid;
            if (!grid) {                                      // (a cell-grid job's fields: grid_job_bind)
                G.m = static_cast<int>(J.n_matched);
                G.has_order = false;
                G.all = true;
            }
            if (J.d_curr != c->d_pts.get())                  // (the context's own scan buffer is used in place)
                LO_HIP(e, hipMemcpyAsync(c->d_pts, J.d_curr, J.n_curr * 3 * sizeof(float), hipMemcpyDeviceToDevice, bs));
            KParams P = make_params(c, c->d_pts, static_cast<int>(J.n_curr));
            set_kd_params(c, P, G);
            P.loop = 1;
            std::memcpy(P.Tm, J.T_matched, sizeof(float) * 12);
            // T_lw_last = T_wl_last.inverse() (:509): the rigid inverse [R^T | -R^T t], evaluated in fp64 and rounded
            for (int r = 0; r < 3; ++r) {
                double tr = 0.0;
                for (int k = 0; k < 3; ++k) {
                    P.Tlw[4 * r + k] = J.T_matched[4 * k + r];
                    tr -= static_cast<double>(J.T_matched[4 * k + r]) * static_cast<double>(J.T_matched[4 * k + 3]);
                }
                P.Tlw[4 * r + 3] = static_cast<float>(tr);
            }
            P.T0p = S->d_T0 + 12 * a;
            std::memcpy(S->h_T0 + 12 * a, J.T_curr, sizeof(float) * 12);
            if (a >= nfast) {                                 // the scale comes from k_exact_scale_cb (iteration 0)
                P.scale_given = 1;
                n_max_ex = std::max(n_max_ex, P.n);
            } else {
                max_acc = std::max(max_acc, P.nb_acc);
            }
            max_nb = std::max(max_nb, P.nb);
            if (grid) max_knn = std::max(max_knn, lb_knn_blocks(P.n));
            else max_all = std::max(max_all, lb_all_blocks(P.n));
            pko_max = std::min(pko_max, pko_grid(c->cfg));
            S->h_P[a] = P;
        }
        if (static_cast<long long>(max_knn) * std::max(ngrid, 1) > INT_MAX)
            return fail(LO_ERR_CAPACITY, -1, "the cell-grid jobs' search grid exceeds 2^31 workgroups");
        LO_HIP(e, hipMemcpyAsync(S->d_T0, S->h_T0, sizeof(float) * 12 * nact, hipMemcpyHostToDevice, bs));
        LO_HIP(e, hipMemcpyAsync(S->d_P, S->h_P, sizeof(KParams) * nact, hipMemcpyHostToDevice, bs));

        // ---- the GN iterations in lockstep, the heads of all jobs read once per chunk
        const size_t lds = lb_all_lds(max_all_m);
        const int pko_wgs = std::max(1, std::min(pko_max, kLoopPkoWGs / nact));
        const size_t pre_bytes = static_cast<size_t>(max_nb) * sizeof(int);
        const dim3 blk(kBlock);
        const int head_blocks = (nact + kWave - 1) / kWave;
        const int per = std::max(1, std::min(kLoopBrutePerJob, kLoopBruteWGs / std::max(ngrid, 1)));
        const int brute_wgs = static_cast<int>(std::min<long long>(kLoopBruteWGs, static_cast<long long>(ngrid) * per));
        const size_t NA = static_cast<size_t>(nact);
        for (int it = 0; it < kLoopIters;) {
            for (int k = 0; k < kLoopChunkB && it < kLoopIters; ++k, ++it) {
                const int first = it == 0 ? 1 : 0;
                if (nall > 0)
                    hipLaunchKernelGGL(k_knn_all_b, dim3(max_all, nact), dim3(kAllThreads), lds, bs, S->d_P.get(), first);
                if (ngrid > 0) {
                    hipLaunchKernelGGL(k_knn_b, dim3(max_knn, ngrid), blk, 0, bs, S->d_P + g0, first);
                    hipLaunchKernelGGL(k_knn_brute_b, dim3(brute_wgs), dim3(1024), 0, bs, S->d_P + g0, ngrid, per);
                }
                hipLaunchKernelGGL(k_plane_b, dim3(max_nb, nact), blk, 0, bs, S->d_P.get(), first);
                if (first && nexl > 0) {
                    launch_exact_scale_cb(S->d_P + nfast, nexl, n_max_ex, bs);
                    LO_HIP(e, hipGetLastError());
                }
                hipLaunchKernelGGL((k_pko_tb<4, false>), dim3(pko_wgs, nact), dim3(256), pre_bytes, bs, S->d_P.get(), it);
                if (nexl > 0)
                    hipLaunchKernelGGL(k_exact_acc_b, dim3(nexl), dim3(256), kXcLdsBytes, bs, S->d_P + nfast, it);
                if (nfast == 0) continue;
                if (max_acc <= kFuseMaxBlocks) {           // small jobs: one 8-wave workgroup accumulates + solves
                    if (nfast < kLoopSplitSolveMin) {
                        hipLaunchKernelGGL(k_accumulate_b1<true>, dim3(1, nfast), dim3(512), 0, bs, S->d_P.get(), it);
                    } else {
                        hipLaunchKernelGGL(k_accumulate_b1<false>, dim3(1, nfast), dim3(512), 0, bs, S->d_P.get(), it);
                        hipLaunchKernelGGL(k_solve_b1, dim3(nfast), blk, 0, bs, S->d_P.get(), it);
                    }
                } else {
                    hipLaunchKernelGGL(k_accumulate_b, dim3(max_acc, nfast), blk, 0, bs, S->d_P.get(), it);
                    hipLaunchKernelGGL(k_solve_b, dim3(nfast), dim3(kSolveThreads), 0, bs, S->d_P.get(), it);
                }
            }
            hipLaunchKernelGGL(k_loop_heads, dim3(head_blocks), dim3(kWave), 0, bs, S->d_P.get(), nact, S->d_head.get());
            LO_HIP(e, hipGetLastError());
            LO_HIP(e, hipMemcpyAsync(S->h_head, S->d_head, sizeof(LoopHead) * NA, hipMemcpyDeviceToHost, bs));
            LO_HIP(e, hipStreamSynchronize(bs));
            bool all_done = true;
            for (int a = 0; a < nact; ++a) all_done = all_done && S->h_head[a].done;
            if (all_done) break;                              // every job converged, or has too few correspondences
        }

        // ---- the inlier pass of the converged jobs (h_words: the all-pairs selection, then the cell-grid one), then
        // the final heads and (asked for) the logs, one copy each
        int nsel_all = 0, nsel_grid = 0, max_sel_all = 1, max_sel_m = 1, max_sel_nb = 1, nlogs = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int a = 0; a < nact; ++a) {
                const LoopHead& H = S->h_head[a];
                const bool grid = a >= g0 && a < g0 + ngrid;
                if (grid != (pass == 1) || H.kd_tie || !(H.done && H.status == LO_OK)) continue;   // (a tied job is run again below)
                S->h_words[nsel_all + nsel_grid] = static_cast<uint32_t>(a);
                if (grid) {
                    ++nsel_grid;
                    max_sel_nb = std::max(max_sel_nb, S->h_P[a].nb);
                } else {
                    ++nsel_all;
                    max_sel_all = std::max(max_sel_all, lb_all_blocks(S->h_P[a].n));
                    max_sel_m = std::max(max_sel_m, S->h_P[a].kd_m);
                }
            }
        if (nsel_all + nsel_grid > 0) {
            const int* d_sel = reinterpret_cast<const int*>(S->d_words.get());
            LO_HIP(e, hipMemcpyAsync(S->d_words, S->h_words, sizeof(uint32_t) * (nsel_all + nsel_grid), hipMemcpyHostToDevice, bs));
            if (nsel_all > 0)
                hipLaunchKernelGGL(k_inlier_all_b, dim3(max_sel_all, nsel_all), dim3(kAllThreads), lb_all_lds(max_sel_m), bs,
                                   S->d_P.get(), d_sel);
            if (nsel_grid > 0)
                hipLaunchKernelGGL(k_inlier_b, dim3(max_sel_nb, nsel_grid), blk, 0, bs, S->d_P.get(), d_sel + nsel_all);
            hipLaunchKernelGGL(k_loop_heads, dim3(head_blocks), dim3(kWave), 0, bs, S->d_P.get(), nact, S->d_head.get());
            LO_HIP(e, hipGetLastError());
            LO_HIP(e, hipMemcpyAsync(S->h_head, S->d_head, sizeof(LoopHead) * NA, hipMemcpyDeviceToHost, bs));
            LO_HIP(e, hipStreamSynchronize(bs));              // (h_words is free again; the heads carry the inliers)
        }
        std::vector<int> log_off(NA, -1);
        if (logs) {
            for (int a = 0; a < nact; ++a) {
                if (S->h_head[a].kd_tie) continue;           // (its logs come from the rerun)
                log_off[a] = nlogs;
                nlogs += std::min(std::max(S->h_head[a].iter, 0), LO_MAX_ITERS);
            }
        }
        if (nlogs > 0) {
            LO_HIP(e, S->d_logs.reserve(static_cast<size_t>(nlogs)));
            LO_HIP(e, S->h_logs.reserve(static_cast<size_t>(nlogs)));
            for (int a = 0; a < nact; ++a) S->h_words[a] = static_cast<uint32_t>(log_off[a]);
            LO_HIP(e, hipMemcpyAsync(S->d_words, S->h_words, sizeof(uint32_t) * NA, hipMemcpyHostToDevice, bs));
            hipLaunchKernelGGL(k_loop_logs, dim3(nact), dim3(kWave), 0, bs, S->d_P.get(),
                               reinterpret_cast<const int*>(S->d_words.get()), S->d_logs.get());
            LO_HIP(e, hipGetLastError());
            LO_HIP(e, hipMemcpyAsync(S->h_logs, S->d_logs, sizeof(lo_iter_log) * nlogs, hipMemcpyDeviceToHost, bs));
        }
        LO_HIP(e, hipEventRecord(S->ev1, bs));
        LO_HIP(e, hipStreamSynchronize(bs));
        if (gpu_ms) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, S->ev0, S->ev1) != hipSuccess) ms = -1.0f;
            *gpu_ms = ms;
        }

        // ---- the records, by loop_solve's own statements; a tied job again, alone, with the kd visit order
        for (int a = 0; a < nact; ++a) {
            const int i = lock[a];
            const lo_loop_job& J = jobs[i];
            lo_loop_rec& R = out[i];
            lo_ctx* c = V.ctx[J.job];
            const LoopHead& H = S->h_head[a];
            if (H.kd_tie) {
                lo_stats st{};
                const int rc = loop_rerun_with_order(c, J.d_curr, J.n_curr, J.T_curr, J.n_matched, J.T_matched, R.T_rel,
                                                     &R.inlier_ratio, logs ? logs + static_cast<size_t>(i) * LO_MAX_ITERS : nullptr,
                                                     &st);
                if (rc < 0) return fail(rc, i, "tie re-run: " + c->err);
                lb_rec_from_stats(R, rc, st);
                R.rerun = 1;
                continue;
            }
            const bool converged = H.done && H.status == LO_OK;
            bool success = false;
            if (converged) {
                // optimized_relative_transform = curr.pose^-1 * optimized_curr_pose (:240), set on convergence
                const lo::SE3f rel = lo::se3_mul(lo::se3_inv(lo::se3_from12(J.T_curr)), lo::se3_from12(H.pose));
                lo::se3_to12(rel, R.T_rel);
                R.inlier_ratio = static_cast<float>(static_cast<int>(H.inliers)) / static_cast<float>(static_cast<int>(J.n_curr));
                success = !(R.inlier_ratio < 0.5f);                           // :244-246
            }
            R.status = success ? LO_OK : LO_INSUFFICIENT;
            R.converged = converged ? 1 : 0;
            R.iterations = H.iter;
            R.n_corr = H.n_corr;
            R.initial_cost = H.initial_cost;
            R.final_cost = H.final_cost;
            if (logs) {
                const int iters = std::min(std::max(H.iter, 0), LO_MAX_ITERS);
                for (int q = 0; q < iters; ++q) logs[static_cast<size_t>(i) * LO_MAX_ITERS + q] = S->h_logs[log_off[a] + q];
            }
        }
    }

    // ---- the large exact jobs, each through the solo entry on its own context
    for (int i : solo) {
        const lo_loop_job& J = jobs[i];
        lo_ctx* c = V.ctx[J.job];
        lo_loop_rec& R = out[i];
        lo_stats st{};
        const long long before = lo_loop_reruns(c);
        const int rc = lo_icp_optimize_loop_dev(c, J.d_curr, J.n_curr, J.T_curr, J.d_matched, J.n_matched, J.T_matched, R.T_rel,
                                                &R.inlier_ratio, logs ? logs + static_cast<size_t>(i) * LO_MAX_ITERS : nullptr, &st);
        if (rc < 0) return fail(rc, i, c->err);
        lb_rec_from_stats(R, rc, st);
        R.rerun = lo_loop_reruns(c) != before ? 1 : 0;
    }
    return LO_OK;
}
