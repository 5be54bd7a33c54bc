// lo_optimize.hip — the optimize drivers: launch helpers, the reference-exact preparation, enqueue_optimize, the
// async / result / sync entry points, the loop-closure ICP and the raw-scan (device filter) path.
//
// lo_icp_optimize enqueues the whole Gauss-Newton loop (4 kernels x max_iterations) with no host synchronisation in
// between; the kernels read DevState::done and fall through once the scan has converged or failed.
#include <hipcub/hipcub.hpp>

#include "lo_ctx_def.h"

namespace lo {
void launch_pko(lo_ctx* c, const KParams& P, int it) {
    // dynamic LDS for the per-block prefix (nb ints; 64 KB only at the 4M-point maximum)
    const size_t pre_bytes = static_cast<size_t>(std::max(P.nb, 1)) * sizeof(int);
    // 4 waves: the EM runs one GMM component per wave (gmm_fit_split), up to 256 samples (4 per lane)
    const int G = pko_grid(c);
    hipLaunchKernelGGL(k_pko_t<4>, dim3(G), dim3(256), pre_bytes, c->stream, P, it, G);
}

// Small scans with PKO: the PKO launch also evaluates the normal equations for every alpha candidate
// (acc_candidate, lo_pko.hip, (NA + 1) x ceil(nb_acc / kSpecBlocksPerWG) extra workgroups); k_solve_pick then
// solves the selected one.
bool spec_ok(const KParams& P) { return P.use_pko && P.acc_part && P.nb_acc <= kFuseMaxBlocks; }

void launch_pko_spec(lo_ctx* c, const KParams& P, int it, hipStream_t s) {
    size_t pre_bytes = static_cast<size_t>(std::max(P.nb, 1)) * sizeof(int);
    const int G = pko_grid(c);
    int W = (P.nb_acc + kSpecBlocksPerWG - 1) / kSpecBlocksPerWG;
    if (P.exact_cand) {                                  // one workgroup per exact candidate, factor rows in LDS
        W = 1;
        pre_bytes = std::max(pre_bytes, kXcLdsBytes);
    }
    if (c->pko_solo) pre_bytes = std::max(pre_bytes, kPkoSoloBytes);
    if (P.exact_cand) hipLaunchKernelGGL(k_pko_tx, dim3(G + (P.NA + 1) * W), dim3(256), pre_bytes, s ? s : c->stream, P, it, G);
    else hipLaunchKernelGGL(k_pko_t<4>, dim3(G + (P.NA + 1) * W), dim3(256), pre_bytes, s ? s : c->stream, P, it, G);
}

// One GN iteration after the correspondence stage: PKO with the speculative normal equations + k_solve_pick
// (small scans), else PKO, then k_accumulate whose last block solves (small) or k_solve over 1024 threads (large).
static void launch_gn_tail(lo_ctx* c, const KParams& P, int it) {
    const dim3 blk(kBlock);
    if (spec_ok(P)) {
        launch_pko_spec(c, P, it);
        hipLaunchKernelGGL(k_solve_pick, dim3(1), blk, 0, c->stream, P, it);
        return;
    }
    launch_pko(c, P, it);
    if (P.nb_acc <= kFuseMaxBlocks) {
        hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), blk, 0, c->stream, P, it, 1);
    } else {
        hipLaunchKernelGGL(k_accumulate, dim3(P.nb_acc), blk, 0, c->stream, P, it, 0);
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(kSolveThreads), 0, c->stream, P, it, 0);
    }
}

// A small scan whose PKO launches pre-solve the candidates (k_pick* selects one): the launch sequence of the fast mode,
// in reference-exact mode with the one-workgroup sort.  enqueue_optimize computes this once, before the lanes are
// chosen, and every branch below tests it; the KParams it is later built into must agree (checked there).
static bool cand_scan(const lo_ctx* c, size_t n) {
    const lo_config& g = c->cfg;
    const size_t nb = (n + kBlock - 1) / kBlock;          // nb_acc = min(nb, kAccBlocks) <= kFuseMaxBlocks
    return n > 0 && g.use_adaptive_m_estimator && c->presolve && nb <= static_cast<size_t>(kFuseMaxBlocks) &&
           g.max_iterations <= LO_MAX_ITERS && (!c->exact || n <= static_cast<size_t>(kExactMaxPoints));
}

// ---------------------------------------------------------------- optimize
// Correspondence stage of one GN iteration: surfel lookup, or (KDTree variant) grid kNN + brute-force
// fallback + plane fit.  P0 carries init = 1 on a scan's first iteration.
static constexpr int kBruteBlocks = 64;      // k_knn_brute workgroups (grid-strided over the unresolved list)
static constexpr int kBruteWaveBlocks = 256; // k_knn_brute_w: 4 queries in flight per workgroup

// The unresolved queries: a wave per query (k_knn_brute_w) over a small grid without the kd visit order, else a
// 1024-thread workgroup per query (k_knn_brute, which also ranks deciding ties in the visit order when it is built).
void launch_brute(lo_ctx* c, const KParams& P) {
    if (brute_wave_form(P.kd_nodes, P.kd_m)) hipLaunchKernelGGL(k_knn_brute_w, dim3(kBruteWaveBlocks), dim3(kBlock), 0, c->stream, P);
    else hipLaunchKernelGGL(k_knn_brute, dim3(kBruteBlocks), dim3(1024), 0, c->stream, P);
}

static dim3 knn_grid(const KParams& P) { return dim3((static_cast<size_t>(P.n) * kKnnGroup + kBlock - 1) / kBlock); }
static size_t all_lds(const KParams& P) { return static_cast<size_t>((std::max(P.kd_m, 1) + 511) / 512 * 512) * sizeof(float4); }   // all_padded
static dim3 all_grid(const KParams& P) { return dim3((std::max(P.n, 1) + kAllThreads / 64 - 1) / (kAllThreads / 64)); }

void launch_correspond(lo_ctx* c, const KParams& P, int with_stats, bool kd) {
    const dim3 grid(P.nb), blk(kBlock);
    if (!kd) {
        hipLaunchKernelGGL(k_correspond, grid, blk, 0, c->stream, P, with_stats);
        return;
    }
    KParams Pn = P;
    Pn.init = 0;
    if (P.kd_all) {                                      // a small set searched whole from LDS: no fallback pass
        hipLaunchKernelGGL(k_knn_all, all_grid(P), dim3(kAllThreads), all_lds(P), c->stream, P);
        hipLaunchKernelGGL(k_plane, grid, blk, 0, c->stream, Pn, with_stats);
        return;
    }
    hipLaunchKernelGGL(k_knn, knn_grid(P), blk, 0, c->stream, P);
    launch_brute(c, Pn);
    hipLaunchKernelGGL(k_plane, grid, blk, 0, c->stream, Pn, with_stats);
}

// After a KDTree-variant PKO launch (small scans): the iteration's solve -- the selected candidate's record
// (k_pick_knn) or its partial sums solved in every block (k_solve_knn) -- fused with the kNN search of it + 1, then
// the unresolved queries and the plane stage.
static void launch_pick_knn(lo_ctx* c, const KParams& P, int it) {
    const dim3 knn = knn_grid(P), blk(kBlock);
    if (P.kd_all) {
        if (P.cand_rec) {
            hipLaunchKernelGGL(k_pick_knn_all, all_grid(P), dim3(kAllThreads), all_lds(P), c->stream, P, it);
        } else {
            hipLaunchKernelGGL(k_solve_pick, dim3(1), blk, 0, c->stream, P, it);
            hipLaunchKernelGGL(k_knn_all, all_grid(P), dim3(kAllThreads), all_lds(P), c->stream, P);
        }
        hipLaunchKernelGGL(k_plane, dim3(P.nb), blk, 0, c->stream, P, 0);
        return;
    }
    if (P.cand_rec) hipLaunchKernelGGL(k_pick_knn, knn, blk, 0, c->stream, P, it);
    else hipLaunchKernelGGL(k_solve_knn, knn, blk, 0, c->stream, P, it);
    launch_brute(c, P);
    hipLaunchKernelGGL(k_plane, dim3(P.nb), blk, 0, c->stream, P, 0);
}

// A scan's first correspondence launch, bracketed by HIP events on the context stream when stage timing is on
// (the kernel's in-step duration, as opposed to lo_bench_kernel's back-to-back launches).
void launch_correspond_first(lo_ctx* c, const KParams& P0, bool kd, int with_stats) {
    const bool timed = c->stage_timing && c->st_n < kStageEvents;
    if (timed) (void)hipEventRecord(c->st_ev[2 * c->st_n], c->stream);
    if (timed && !kd && c->d_span) {                     // and its own execution span (k_correspond, P.span)
        KParams Pt = P0;
        Pt.span = c->d_span + static_cast<size_t>(kSpanWords) * c->st_n;
        launch_correspond(c, Pt, with_stats, kd);
    } else {
        launch_correspond(c, P0, with_stats, kd);
    }
    if (timed) (void)hipEventRecord(c->st_ev[2 * c->st_n++ + 1], c->stream);
}

// Reference-exact mode (lo_exact.hip): device buffers on first use, then per GN iteration the correspondence stage,
// (iteration 0) the sorted-order scale, the PKO, the per-point terms and the sequential sums + fp32 solve.  Scans of
// at most kExactMaxPoints sort in one workgroup (*n2 = n: registers + LDS, lo_seqsum.h); larger scans (*n2 = 0)
// write their residuals out, sort them with hipCUB's radix sort and sum them across the chip (launch_mwm_scale).
static int exact_prepare(lo_ctx* c, KParams& P, size_t n, int* n2) {
    // the term buffer: row-major [point][43] up to kExactMaxPoints (k_exact_terms + k_exact_solve), term-major rows of
    // round_up(n, 64) beyond (the 14 factor rows)
    const size_t ex_need = std::max(static_cast<size_t>(kExactMaxPoints) * kExactTerms,
                                    kExactFactors * ((n + 63) & ~static_cast<size_t>(63)));
    LO_HIP(c, c->d_ex_terms.reserve(ex_need));
    LO_HIP(c, c->d_ex_rank.reserve(kExactMaxPoints));
    if (!c->ex_attr) {
        LO_HIP(c, exact_scale_rank_prepare());
        LO_HIP(c, exact_scale_c_prepare());
        c->ex_attr = true;
    }
    P.ex_terms = c->d_ex_terms;
    P.scale_given = 1;
    // up to kExactMaxPoints points one workgroup sorts and sums the iteration-0 residuals (a device-counted scan -- the
    // voxel filter's output -- picks its sort width from the count on the device, k_exact_scale_cd, instead of sizing
    // the sort by the bound ceil(n_raw / stride))
    c->ex_merge = n <= static_cast<size_t>(kExactMaxPoints);
    if (std::getenv("LO_EXACT_RANKSORT")) c->ex_merge = false;   // A/B: the chip-wide rank sort
    if (n > static_cast<size_t>(kExactMaxPoints)) {
        LO_HIP(c, c->d_ex_tot.reserve(64));
        if (c->mw_n < n) {                                   // the column sums' head records
            c->mw_n = 0;                                     //   (no layout until both buffers and the clear succeeded)
            c->d_mw.reset();
            LO_HIP(c, c->d_mw.reserve(mw_bytes(43, static_cast<int>(n))));
            c->mw = mw_layout(c->d_mw, 43, static_cast<int>(n));
            LO_HIP(c, mw_clear(c->mw, 43, c->stream));
            LO_HIP(c, hipStreamSynchronize(c->stream));
            c->d_mwm.reset();
            LO_HIP(c, c->d_mwm.reserve(mwm_bytes(static_cast<int>(n))));
            c->mwm = mwm_layout(c->d_mwm, static_cast<int>(n));
            c->mw_n = n;
        }
        P.ex_ld = static_cast<int>((n + 63) & ~static_cast<size_t>(63));   // term-major rows, 256-B aligned
        P.ex_tot = c->d_ex_tot;
        if (c->d_ex_sort_tmp.capacity() == 0 || c->d_ex_res.capacity() < n) {
            c->d_ex_sort_tmp.reset();                        // (set last: a failed grow is redone on the next scan)
            c->d_ex_res.reset();
            c->d_ex_sorted.reset();
            LO_HIP(c, c->d_ex_res.reserve(n));
            LO_HIP(c, c->d_ex_sorted.reserve(n));
            size_t tmp = 0;
            LO_HIP(c, hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, c->d_ex_res.get(), c->d_ex_sorted.get(),
                                                        static_cast<int>(n)));
            LO_HIP(c, c->d_ex_sort_tmp.reserve(std::max<size_t>(tmp, 1)));
        }
        *n2 = 0;
        return LO_OK;
    }
    *n2 = static_cast<int>(n);
    return LO_OK;
}
// the iteration-0 scale of reference-exact mode (between the scan's first correspondence launch and its first PKO)
void launch_exact_scale_any(lo_ctx* c, const KParams& P, int n2, hipStream_t s) {
    if (c->ex_merge) {
        launch_exact_scale_c(P, s);                          // counting sort + sums in one workgroup (<= 16384 points)
        return;
    }
    if (n2 > 0) {
        launch_exact_scale(P, n2, c->d_ex_rank, s);          // rank sort across the chip (A/B and diagnostics)
        return;
    }
    // beyond kExactMaxPoints: hipCUB sort + long mono sums
    const int n = P.n;                                       // the bound (a device-filtered scan counts on the device)
    hipLaunchKernelGGL(k_exact_resid, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, P, c->d_ex_res);
    size_t tmp = c->d_ex_sort_tmp.capacity();
    (void)hipcub::DeviceRadixSort::SortKeys(c->d_ex_sort_tmp, tmp, c->d_ex_res.get(), c->d_ex_sorted.get(), n, 0,
                                            static_cast<int>(sizeof(double) * 8), s);
    launch_mwm_scale(P, c->d_ex_sorted, c->mwm, s);
}
static void launch_exact_iteration(lo_ctx* c, const KParams& P, const KParams& P0, int it, int n2, bool kd) {
    if (it == 0) launch_correspond_first(c, P0, kd, 0);   // (stage timing: the scan's first correspondence launch)
    else launch_correspond(c, P, 0, kd);
    if (it == 0) launch_exact_scale_any(c, P, n2, c->stream);
    launch_pko(c, P, it);
    hipLaunchKernelGGL(k_exact_terms, dim3(P.nb), dim3(kBlock), 0, c->stream, P);
    if (P.ex_ld) {                                           // large scan: 43 parallel sequential-sum reproductions
        launch_mw_sums(P.ex_terms, P.ex_ld, 43, P.n, P.n_dev, P.st, c->mw, P.ex_tot, nullptr, c->stream, true);
        hipLaunchKernelGGL(k_exact_finish, dim3(1), dim3(64), 0, c->stream, P, it);
    } else {
        hipLaunchKernelGGL(k_exact_solve, dim3(1), dim3(512), 0, c->stream, P, it);   // kExactSolveThreads
    }
}

// The GN loop on the context stream alone.  fused (small scan with PKO): the solve of iteration it runs fused with the
// correspondence search of it + 1 (k_solve_correspond; KDTree: k_solve_knn, then k_knn_brute + k_plane), the last
// solve alone (k_solve_pick).
static void emit_single(lo_ctx* c, const KParams& P, const KParams& P0, int n2, bool fused) {
    const int iters = c->cfg.max_iterations;
    for (int it = 0; it < iters; ++it) {
        if (!fused) {
            if (it == 0) launch_correspond_first(c, P0, c->kd);
            else launch_correspond(c, P, 0, c->kd);
            launch_gn_tail(c, P, it);
            continue;
        }
        if (it == 0) {
            launch_correspond_first(c, P0, c->kd);
            if (c->exact) launch_exact_scale_any(c, P, n2, c->stream);
        }
        launch_pko_spec(c, P, it);
        if (it + 1 < iters && !c->kd) {
            if (P.cand_rec) hipLaunchKernelGGL(k_pick_correspond, dim3(P.nb), dim3(kBlock), 0, c->stream, P, it);
            else hipLaunchKernelGGL(k_solve_correspond, dim3(P.nb), dim3(kBlock), 0, c->stream, P, it);
        } else if (it + 1 < iters) {
            launch_pick_knn(c, P, it);
        } else if (P.cand_rec) {
            hipLaunchKernelGGL(k_pick, dim3(1), dim3(kBlock), 0, c->stream, P, it);
        } else {
            hipLaunchKernelGGL(k_solve_pick, dim3(1), dim3(kBlock), 0, c->stream, P, it);
        }
    }
}

// One scan: snapshot of the queue, plan (lo_scan_plan.h), the plan's flush / lane switch / holds, the scan's KParams,
// then its launches -- down the scan pipeline (emit_pipelined) or on the context stream alone.
int enqueue_optimize(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12], const int* n_dev) {
    std::memcpy(c->T_init, T_init, sizeof(float) * 12);
    c->last_n = n;
    c->last_pts = d_pts;
    c->last_ndev = n_dev;
    // Scan groups (lo_scan_group_plan.h): a groupable scan joins the open group and is launched with it; anything else
    // sends the open group out first (record order) and takes the ring path.  A scan that would leave at once as a
    // group of one (nothing of the context in flight) goes straight down the ring, as it always did.
    const GroupPlan gp = plan_group(group_snapshot(c, n, cand_scan(c, n), c->sync_call, n_dev != nullptr));
    if (gp.append && (gp.lockstep || !gp.emit)) {
        int rc = group_append(c, gp, d_pts, n, T_init);
        if (rc == LO_OK && gp.emit) rc = group_emit(c);
        if (rc != LO_OK) return rc;
        c->last_timed = false;
        c->pending = true;
        return LO_OK;
    }
    const int rcg = group_emit(c);
    if (rcg != LO_OK) return rcg;
    return enqueue_ring(c, d_pts, n, T_init, n_dev);
}

// The ring path of one scan (and of every scan of a group too small for lockstep, group_emit).
int enqueue_ring(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12], const int* n_dev) {
    const lo_config& g = c->cfg;
    leave_group_set(c);
    { const int rcj = group_join(c); if (rcj != LO_OK) return rcj; }   // behind the groups still running (record order)
    const unsigned ring_run = c->q.ring_n;                // the run of pipelined scans ends here unless this is one
    c->q.ring_n = 0;
    // HIP events only for synchronous calls (gpu_ms): a marker packet costs ~5-7 us of device time per scan
    const bool timed = c->sync_call;
    c->last_timed = timed;
    const bool cand = cand_scan(c, n);
    const ScanPlan plan = plan_scan(scan_snapshot(c, cand, timed, n_dev != nullptr));
    const int rcp = apply_plan(c, plan);
    if (rcp != LO_OK) return rcp;
    if (timed) LO_HIP(c, hipEventRecord(c->ev0, c->stream));
    if (n == 0) {
        // reset the GN state (pose by kernel argument: no host staging buffer, scans can queue back to back)
        Pose12 T0;
        std::memcpy(T0.v, T_init, sizeof(float) * 12);
        hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, c->stream, cur(c).d_st, T0, 1.0, g.robust_loss_delta);
    } else {
        const int rc = ensure_acc_part(c);
        if (rc != LO_OK) return rc;
        KParams P = make_params(c, d_pts, static_cast<int>(n));
        P.n_dev = n_dev;                                  // device-filtered scan: count read on the device
        std::memcpy(P.T0, T_init, sizeof(float) * 12);    // k_solve_correspond's pose before iteration 0
        KParams P0 = P;                                   // first k_correspond also resets the GN state
        P0.init = 1;
        const bool fused = spec_ok(P) && g.max_iterations <= LO_MAX_ITERS;
        if (cand != (fused && P.cand_rec != nullptr && (!c->exact || n <= static_cast<size_t>(kExactMaxPoints)))) {
            c->err = "enqueue_optimize: cand_scan disagrees with the scan's parameters";
            return LO_ERR_STATE;
        }
        int n2 = 0;
        if (c->exact) {
            const int rc3 = exact_prepare(c, P, n, &n2);
            if (rc3 != LO_OK) return rc3;
            P0.ex_terms = P.ex_terms;
            P0.scale_given = P.scale_given;
            // small scans with PKO: the same launch sequence as the default mode, with the sorted-order scale after the
            // first correspondence launch and the PKO launch's candidates forming the reference's sequential sums
            if (cand) P.exact_cand = P0.exact_cand = 1;
        }
        if (c->exact && !cand) {                          // (n2 > 0 exactly when n <= kExactMaxPoints)
            // reference-exact GN loop without candidates (lo_exact.hip): correspondences, (iteration 0) sorted-order
            // scale, PKO, per-point fp32 terms, sequential sums + fp32 LDLT + SVD-projected update
            for (int it = 0; it < g.max_iterations; ++it) launch_exact_iteration(c, P, P0, it, n2, c->kd);
        } else {
            if (c->q.flagged()) {                         // an earlier scan's wait timed out: one stream from now on
                const int rc4 = pipe_recover(c);
                if (rc4 != LO_OK) return rc4;
            }
            // (c->q.pipe as it is now: a recovery just above switched it off, whatever the plan saw)
            if (plan.pipelined && c->q.pipe) return emit_pipelined(c, plan, P, P0, n2, ring_run);
            const int rcf = flush_hold(c);                // (none pending unless the pipeline was just switched off)
            if (rcf != LO_OK) return rcf;
            emit_single(c, P, P0, n2, fused);
        }
        LO_HIP(c, hipGetLastError());
    }
    if (timed) LO_HIP(c, hipEventRecord(c->ev1, c->stream));
    c->pending = true;
    return LO_OK;
}
}  // namespace lo

extern "C" {

int lo_icp_optimize_async(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12]) {
    if (!c || !T_init || (n > 0 && !d_pts)) return LO_ERR_ARG;
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    c->last_dev_count = false;
    c->nf_valid = false;
    return enqueue_optimize(c, d_pts, n, T_init);
}

int lo_icp_result(lo_ctx* c, float T_out[12], lo_iter_log* logs, lo_stats* st) {
    if (!c) return LO_ERR_ARG;
    if (!c->pending) { c->err = "no optimize in flight"; return LO_ERR_STATE; }
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    // state header + the executed iterations' logs only
    const size_t bytes = offsetof(DevState, logs) + sizeof(lo_iter_log) * static_cast<size_t>(c->cfg.max_iterations);
    LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, bytes, hipMemcpyDeviceToHost, c->stream));
    // a device-filtered scan: its count comes back in the same sync (lo_filtered_points(ctx, NULL, 0) then reads it
    // without another round trip -- the frame loop asks for it every frame)
    c->nf_valid = c->last_dev_count && c->vf.n_out;
    if (c->nf_valid) LO_HIP(c, hipMemcpyAsync(c->h_nf, c->vf.n_out, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    c->pending = false;
    const DevState* hs = c->h_st;
    int status = c->last_n == 0 ? LO_INSUFFICIENT : hs->status;
    if (status == LO_ERR_PIPELINE) {
        // this scan's pipeline wait timed out: pipeline off, then the same scan again on one stream (its points are
        // still the caller's until this call returns)
        int rc = pipe_recover(c);
        if (rc != LO_OK) return rc;
        float T0[12];
        std::memcpy(T0, c->T_init, sizeof(T0));
        const bool timed = c->sync_call;
        rc = enqueue_optimize(c, c->last_pts, c->last_n, T0, c->last_ndev);
        c->sync_call = timed;
        if (rc == LO_OK) rc = flush_hold(c);
        if (rc != LO_OK) return rc;
        LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, bytes, hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        c->pending = false;
        ++c->q.pipe_reruns;
        status = hs->status;
    }
    if (c->kd && c->grid_dev && !c->grid.has_order && hs->kd_tie && c->last_n > 0) {
        // a deciding distance tie was ranked by index (a device-built grid has no kd visit order): the order built on
        // the host from the grid's own points, then the same scan again (its points are still the caller's)
        int rc = grid_add_order(c);
        if (rc != LO_OK) return rc;
        float T0[12];
        std::memcpy(T0, c->T_init, sizeof(T0));
        const bool timed = c->sync_call;
        rc = enqueue_optimize(c, c->last_pts, c->last_n, T0, c->last_ndev);
        c->sync_call = timed;
        if (rc == LO_OK) rc = flush_hold(c);
        if (rc != LO_OK) return rc;
        LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, bytes, hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        c->pending = false;
        ++c->kd_reruns;
        status = hs->status;
    }
    const int iters = hs->iter;
    if (T_out) {
        if (status == LO_OK) std::memcpy(T_out, hs->pose, sizeof(float) * 12);
        else std::memcpy(T_out, c->T_init, sizeof(float) * 12);   // optimized_transform = initial (:266, :301)
    }
    if (logs) for (int i = 0; i < iters && i < c->cfg.max_iterations; ++i) logs[i] = hs->logs[i];
    if (st) {
        st->iterations = iters;
        st->n_corr = hs->n_corr;
        st->status = status;
        st->converged = status == LO_OK ? 1 : 0;
        st->initial_cost = iters > 0 ? hs->logs[0].cost : 0.0;
        st->final_cost = iters > 0 ? hs->logs[iters - 1].cost : 0.0;
        float ms = -1.0f;                                  // -1: an async call (not timed)
        if (c->last_timed && hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) ms = -1.0f;
        st->gpu_ms = ms;
    }
    return status;
}

int lo_sync(lo_ctx* c) {
    if (!c) return LO_ERR_ARG;
    LO_HIP(c, sync_all(c));
    return LO_OK;
}

int lo_icp_optimize(lo_ctx* c, const float* pts, size_t n, const float T_init[12], float T_out[12],
                    lo_iter_log* logs, lo_stats* st) {
    if (!c || !T_init || !T_out || (n > 0 && !pts)) return LO_ERR_ARG;
    if (n > static_cast<size_t>(c->cfg.max_points)) { c->err = "n exceeds max_points"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (n > 0) LO_HIP(c, hipMemcpyAsync(c->d_pts, pts, n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    c->last_dev_count = false;
    c->nf_valid = false;
    c->sync_call = true;
    int rc = enqueue_optimize(c, c->d_pts, n, T_init);
    c->sync_call = false;
    if (rc != LO_OK) return rc;
    return lo_icp_result(c, T_out, logs, st);
}

// ---------------------------------------------------------------- loop-closure ICP
// IterativeClosestPointOptimizer::optimize_loop (:40-251) + find_correspondences_loop (:465-585): the KDTree
// correspondence kernels against the matched keyframe's local map (its own grid, so the context's odometry map
// is left alone), no distance gate, up to 100 GN iterations enqueued kLoopChunk at a time between convergence
// checks, then the 1-NN inlier ratio (k_inlier) once converged.
static constexpr int kLoopMaxIters = 100;                // :74
static constexpr int kLoopChunk = 4;
static constexpr int kLoopMinPerCell = 4;                // the matched cloud's grid: >= 4 points per occupied cell

// The solve shared by both entry points, after the matched cloud's local map sits in c->lgrid (built without the kd
// visit order).  curr: the current cloud, a host pointer or (curr_dev) a device pointer -- c->d_pts itself is used in
// place; lmap: the matched cloud in the world on the host, or null when it exists on the device only (a rerun with
// the visit order then brings the gridded points down, grid_add_order).
static int loop_solve(lo_ctx* c, const float* curr, bool curr_dev, size_t n_curr, const float T_curr[12], const float* lmap,
                      size_t n_matched, const float T_matched[12], float T_rel_out[12], float* inlier_ratio,
                      lo_iter_log* logs, lo_stats* st, bool with_order = false) {
    int rc = LO_OK;
    // all_pairs_upload has put a host cloud into c->d_pts already; every other case copies it below
    bool curr_staged = !curr_dev && c->lgrid.all;
retry:
    if (st) { std::memset(st, 0, sizeof(*st)); st->status = LO_INSUFFICIENT; }
    if (n_curr == 0 || n_matched == 0) return LO_INSUFFICIENT;       // empty clouds: 0 correspondences (:477-483)
    if ((rc = ensure_acc_part(c)) != LO_OK) return rc;
    if (!curr_staged && curr != c->d_pts.get())
        LO_HIP(c, hipMemcpyAsync(c->d_pts, curr, n_curr * 3 * sizeof(float),
                                 curr_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    curr_staged = false;                                 // (a rerun copies it again, as it always has)
    KParams P = make_params(c, c->d_pts, static_cast<int>(n_curr));
    set_kd_params(c, P, c->lgrid);
    P.loop = 1;
    std::memcpy(P.Tm, T_matched, sizeof(float) * 12);
    // T_lw_last = T_wl_last.inverse() (:509): the rigid inverse [R^T | -R^T t], evaluated in fp64 and rounded
    for (int r = 0; r < 3; ++r) {
        double tr = 0.0;
        for (int k = 0; k < 3; ++k) {
            P.Tlw[4 * r + k] = T_matched[4 * k + r];
            tr -= static_cast<double>(T_matched[4 * k + r]) * static_cast<double>(T_matched[4 * k + 3]);
        }
        P.Tlw[4 * r + 3] = static_cast<float>(tr);
    }
    int n2 = 0;
    if (c->exact && (rc = exact_prepare(c, P, n_curr, &n2)) != LO_OK) return rc;
    KParams P0 = P;
    P0.init = 1;
    std::memcpy(P0.T0, T_curr, sizeof(float) * 12);
    // small clouds with PKO: the odometry path's launch sequence (candidates solved in the PKO launch, k_pick_knn
    // taking the selected one fused with the next kNN search); reference-exact mode as there
    const bool cand = spec_ok(P) && P.cand_rec && (!c->exact || n2 > 0);
    if (cand && c->exact) { P.exact_cand = P0.exact_cand = 1; P0.ex_terms = P.ex_terms; }
    const dim3 blk(kBlock);
    LO_HIP(c, hipEventRecord(c->ev0, c->stream));
    const size_t head = offsetof(DevState, logs);
    for (int it = 0; it < kLoopMaxIters;) {
        for (int k = 0; k < kLoopChunk && it < kLoopMaxIters; ++k, ++it) {
            if (cand) {
                if (it == 0) {
                    launch_correspond(c, P0, 1, true);
                    if (c->exact) launch_exact_scale_any(c, P, n2, c->stream);
                }
                launch_pko_spec(c, P, it);
                if (it + 1 < kLoopMaxIters) launch_pick_knn(c, P, it);
                else hipLaunchKernelGGL(k_pick, dim3(1), blk, 0, c->stream, P, it);
                continue;
            }
            if (c->exact) {
                launch_exact_iteration(c, P, P0, it, n2, true);
                continue;
            }
            launch_correspond(c, it == 0 ? P0 : P, it == 0 ? 1 : 0, true);
            launch_gn_tail(c, P, it);
        }
        LO_HIP(c, hipGetLastError());
        LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, head, hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        if (c->h_st->done) break;                                 // converged, or too few correspondences
    }
    const bool converged = c->h_st->done && c->h_st->status == LO_OK;
    if (converged && P.kd_all) hipLaunchKernelGGL(k_inlier_all, all_grid(P), dim3(kAllThreads), all_lds(P), c->stream, P);
    else if (converged) hipLaunchKernelGGL(k_inlier, dim3(P.nb), blk, 0, c->stream, P);
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipEventRecord(c->ev1, c->stream));
    const size_t bytes = head + sizeof(lo_iter_log) * static_cast<size_t>(LO_MAX_ITERS);
    LO_HIP(c, hipMemcpyAsync(c->h_st, cur(c).d_st, bytes, hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    if (c->h_st->kd_tie && !with_order) {               // a deciding tie was ranked by index: redo with the order
        with_order = true;
        ++c->loop_reruns;
        rc = lmap ? grid_build(c, c->lgrid, lmap, n_matched, true, kLoopMinPerCell)
                  : grid_add_order(c, c->lgrid, kLoopMinPerCell);
        if (rc != LO_OK) return rc;
        goto retry;
    }
    const DevState* hs = c->h_st;
    bool success = false;
    if (converged) {
        // optimized_relative_transform = curr.pose^-1 * optimized_curr_pose (:240), set on convergence
        const lo::SE3f rel = lo::se3_mul(lo::se3_inv(lo::se3_from12(T_curr)), lo::se3_from12(hs->pose));
        lo::se3_to12(rel, T_rel_out);
        *inlier_ratio = static_cast<float>(static_cast<int>(hs->inliers)) / static_cast<float>(static_cast<int>(n_curr));
        success = !(*inlier_ratio < 0.5f);                            // :244-246
    }
    const int iters = hs->iter;
    if (logs) for (int i = 0; i < iters && i < LO_MAX_ITERS; ++i) logs[i] = hs->logs[i];
    const int status = success ? LO_OK : LO_INSUFFICIENT;
    if (st) {
        st->iterations = iters;
        st->n_corr = hs->n_corr;
        st->status = status;
        st->converged = converged ? 1 : 0;
        const int last = std::min(iters, LO_MAX_ITERS) - 1;
        st->initial_cost = iters > 0 ? hs->logs[0].cost : 0.0;
        st->final_cost = last >= 0 ? hs->logs[last].cost : 0.0;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) ms = -1.0f;
        st->gpu_ms = ms;
    }
    c->pending = false;
    return status;
}

int lo_icp_optimize_loop(lo_ctx* c, const float* curr, size_t n_curr, const float T_curr[12], const float* matched,
                         size_t n_matched, const float T_matched[12], float T_rel_out[12], float* inlier_ratio,
                         lo_iter_log* logs, lo_stats* st) {
    if (!c || !T_curr || !T_matched || !T_rel_out || !inlier_ratio || (n_curr > 0 && !curr) || (n_matched > 0 && !matched))
        return LO_ERR_ARG;
    if (n_curr > static_cast<size_t>(c->cfg.max_points)) { c->err = "n_curr exceeds max_points"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    int rc = flush_hold(c);
    if (rc == LO_OK) rc = kd_alloc(c);
    if (rc != LO_OK) return rc;
    // local map of the matched keyframe: its feature cloud in the world (transform_point_cloud, :60-64)
    const lo::SE3f Tm = lo::se3_from12(T_matched);
    std::vector<float> lmap(3 * std::max<size_t>(n_matched, 1));
    if (n_matched > 0) lo::transform_points(Tm, matched, n_matched, lmap.data());
    // the matched cloud's grid first without the kd visit order (building it is ~0.3 ms of host work per call and
    // it only ranks exact distance ties that decide a query's five neighbours or their order, which keyframe
    // centroids rarely produce); a solve that met one is rerun with the order (loop_solve)
    const bool all = n_matched <= static_cast<size_t>(kKnnAllMax);     // (the clouds' pinned upload, curr included)
    rc = all ? all_pairs_upload(c, c->lgrid, lmap.data(), n_matched, curr, n_curr)
             : grid_build(c, c->lgrid, lmap.data(), n_matched, false, kLoopMinPerCell);
    if (rc != LO_OK) return rc;
    return loop_solve(c, curr, false, n_curr, T_curr, lmap.data(), n_matched, T_matched, T_rel_out, inlier_ratio, logs, st);
}

// The same solve on device-resident clouds: the matched cloud goes to the world and into the local map's layout on
// the device (loop_map_from_device), the current cloud is copied device to device (or is c->d_pts already).
int lo_icp_optimize_loop_dev(lo_ctx* c, const float* d_curr, size_t n_curr, const float T_curr[12], const float* d_matched,
                             size_t n_matched, const float T_matched[12], float T_rel_out[12], float* inlier_ratio,
                             lo_iter_log* logs, lo_stats* st) {
    if (!c || !T_curr || !T_matched || !T_rel_out || !inlier_ratio || (n_curr > 0 && !d_curr) ||
        (n_matched > 0 && !d_matched))
        return LO_ERR_ARG;
    if (n_curr > static_cast<size_t>(c->cfg.max_points)) { c->err = "n_curr exceeds max_points"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    int rc = flush_hold(c);
    if (rc == LO_OK) rc = kd_alloc(c);
    if (rc != LO_OK) return rc;
    rc = loop_map_from_device(c, c->lgrid, d_matched, n_matched, T_matched, kLoopMinPerCell);
    if (rc != LO_OK) return rc;
    return loop_solve(c, d_curr, true, n_curr, T_curr, nullptr, n_matched, T_matched, T_rel_out, inlier_ratio, logs, st);
}

// ---------------------------------------------------------------- device preprocessing + optimize
static int stage_raw(lo_ctx* c, const float* raw, size_t n_raw) {
    LO_HIP(c, c->d_raw.reserve(n_raw * 3));
    if (n_raw > 0) LO_HIP(c, hipMemcpyAsync(c->d_raw, raw, n_raw * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return LO_OK;
}

static int check_raw_args(lo_ctx* c, size_t n_raw, int stride, float voxel) {
    if (stride < 1 || !(voxel > 0.0f)) { c->err = "stride must be >= 1 and voxel_size > 0"; return LO_ERR_ARG; }
    const size_t m = (n_raw + stride - 1) / stride;
    if (m > static_cast<size_t>(c->cfg.max_points)) { c->err = "ceil(n_raw / stride) exceeds max_points"; return LO_ERR_CAPACITY; }
    return LO_OK;
}

int lo_icp_optimize_raw_async(lo_ctx* c, const float* d_raw, size_t n_raw, int stride, float voxel_size,
                              const float T_init[12]) {
    if (!c || !T_init || (n_raw > 0 && !d_raw)) return LO_ERR_ARG;
    int rc = check_raw_args(c, n_raw, stride, voxel_size);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipSetDevice(c->device));
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    int m = 0;
    LO_HIP(c, vf_enqueue(c->vf, d_raw, n_raw, stride, voxel_size, c->d_pts, c->stream, m));
    c->last_dev_count = true;
    c->nf_valid = false;
    return enqueue_optimize(c, c->d_pts, static_cast<size_t>(m), T_init, c->vf.n_out);
}

void* lo_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 1), hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void lo_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

int lo_icp_optimize_raw(lo_ctx* c, const float* raw, size_t n_raw, int stride, float voxel_size, const float T_init[12],
                        float T_out[12], lo_iter_log* logs, lo_stats* st) {
    if (!c || !T_init || !T_out || (n_raw > 0 && !raw)) return LO_ERR_ARG;
    int rc = check_raw_args(c, n_raw, stride, voxel_size);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipSetDevice(c->device));
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    const float* src = n_raw > 0 ? pinned_alias(raw) : nullptr;
    if (!src) {                                          // pageable: stage the scan in device memory
        rc = stage_raw(c, raw, n_raw);
        if (rc != LO_OK) return rc;
        src = c->d_raw;
    }
    c->sync_call = true;
    rc = lo_icp_optimize_raw_async(c, src, n_raw, stride, voxel_size, T_init);
    c->sync_call = false;
    if (rc != LO_OK) return rc;
    return lo_icp_result(c, T_out, logs, st);
}

long long lo_filtered_points(lo_ctx* c, float* out, size_t cap) {
    if (!c) return LO_ERR_ARG;
    if (!c->last_dev_count || !c->vf.n_out) { c->err = "no device-filtered scan"; return LO_ERR_STATE; }
    if (!out && c->nf_valid && !c->pending) return *c->h_nf;   // read back with the scan's result (lo_icp_result)
    LO_HIP(c, hipSetDevice(c->device));
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    int n = 0;
    LO_HIP(c, hipMemcpyAsync(&n, c->vf.n_out, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    if (out && n > 0) {
        const size_t k = std::min<size_t>(static_cast<size_t>(n), cap);
        LO_HIP(c, hipMemcpy(out, c->d_pts, k * 3 * sizeof(float), hipMemcpyDeviceToHost));
    }
    return n;
}

long long lo_voxel_filter_gpu(lo_ctx* c, const float* raw, size_t n_raw, float voxel_size, int stride, float* out,
                              size_t out_cap) {
    if (!c || (n_raw > 0 && !raw)) return LO_ERR_ARG;
    int rc = check_raw_args(c, n_raw, stride, voxel_size);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipSetDevice(c->device));
    rc = flush_hold(c);
    if (rc == LO_OK) rc = stage_raw(c, raw, n_raw);
    if (rc != LO_OK) return rc;
    int m = 0;
    LO_HIP(c, vf_enqueue(c->vf, c->d_raw, n_raw, stride, voxel_size, c->d_pts, c->stream, m));
    c->last_dev_count = true;
    c->nf_valid = false;
    return lo_filtered_points(c, out, out_cap);
}

}  // extern "C"

namespace lo {
// The rerun of a loop solve that met a deciding distance tie, for a caller that ran the first pass itself (the batched
// loop ICP, lo_batch_loop.hip): what loop_solve does from its tie test on -- the rerun counted, the kd visit order
// built from the gridded points of c->lgrid, the solve again on the context stream.
int loop_rerun_with_order(lo_ctx* c, const float* d_curr, size_t n_curr, const float T_curr[12], size_t n_matched,
                          const float T_matched[12], float T_rel_out[12], float* inlier_ratio, lo_iter_log* logs,
                          lo_stats* st) {
    ++c->loop_reruns;
    const int rc = grid_add_order(c, c->lgrid, kLoopMinPerCell);
    if (rc != LO_OK) return rc;
    return loop_solve(c, d_curr, true, n_curr, T_curr, nullptr, n_matched, T_matched, T_rel_out, inlier_ratio, logs, st, true);
}
}  // namespace lo
