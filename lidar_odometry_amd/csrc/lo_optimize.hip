// lo_optimize.hip — the optimize drivers: launch helpers, the reference-exact preparation, enqueue_optimize, the
// async / result / sync entry points, the loop-closure ICP and the raw-scan (device filter) path.
//
// lo_icp_optimize enqueues the whole Gauss-Newton loop (4 kernels x max_iterations) with no host synchronisation in
// between; the kernels read DevState::done and fall through once the scan has converged or failed.
#include <hipcub/hipcub.hpp>

#include <atomic>

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

// Scan pipeline (first pipelined scan): the lanes' tail streams, their fence words, the record ring, the host flag.
static int pipe_alloc(lo_ctx* c) {
    if (c->d_hbroken) return LO_OK;                 // set last
    // (the first lane's tail stream; another lane's is made when a scan first runs there with two or more in flight)
    if (!c->s_tail[0]) LO_HIP(c, hipStreamCreateWithFlags(&c->s_tail[0], hipStreamNonBlocking));
    // (pipe_fail finds every group from any one: kMaxLanes x 16 bytes, aligned to that -- hipMalloc aligns to 256)
    LO_HIP(c, c->d_fin.reserve(kMaxLanes * kFinWords));
    LO_HIP(c, hipMemset(c->d_fin, 0, kMaxLanes * kFinWords * sizeof(uint32_t)));
    LO_HIP(c, c->d_ring.reserve(static_cast<size_t>(kRingRecords) * kRecWords));
    LO_HIP(c, hipMemset(c->d_ring, 0, static_cast<size_t>(kRingRecords) * kRecWords * sizeof(float)));
    LO_HIP(c, c->h_broken.reserve(1));
    *c->h_broken = 0;
    LO_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_hbroken), c->h_broken, 0));
    LO_HIP(c, hipDeviceSynchronize());              // zeroed before either stream's first poll
    return LO_OK;
}

// A pipeline wait timed out (the dispatcher ran the streams out of submission order): drain the context stream and every
// lane stream, switch the pipeline off for this context, clear the flag words.  Scans enqueued before this point report
// LO_ERR_PIPELINE (their tails left without touching anything); a synchronous call re-runs its scan on one stream
// (lo_icp_result).
static int pipe_recover(lo_ctx* c) {
    LO_HIP(c, sync_all(c));                         // (enqueues the pending holds of every lane first: they give up at once)
    c->pipe = false;
    ++c->pipe_timeouts;
    c->ring_n = 0;                                  // (the records of the scans that gave up were never written)
    c->err = "scan pipeline: a device-side wait timed out (the streams were not run concurrently, e.g. rocprofv3 "
             "counter collection); pipeline switched off for this context";
    LO_HIP(c, hipMemset(c->d_fin, 0, kMaxLanes * kFinWords * sizeof(uint32_t)));
    for (uint32_t& s : c->lane_seq) s = 0;          // (with the words they count in)
    LO_HIP(c, hipStreamSynchronize(nullptr));
    __atomic_store_n(c->h_broken.get(), 0u, __ATOMIC_RELEASE);
    return LO_OK;
}
static bool pipe_flagged(const lo_ctx* c) { return c->h_broken && __atomic_load_n(c->h_broken.get(), __ATOMIC_ACQUIRE) != 0u; }

// Contexts of this process with a hold pending, i.e. with queued scans in flight right now.
static std::atomic<int> g_holding{0};
// Scan overlap: the one place a pending hold leaves the host -- the oldest one, on the context stream.  The wait is
// k_wait_final's as before: bounded by pipe_bound, it gives up at once when the pipeline is broken, and a timeout marks
// the held scan's own DevState (its lane's) LO_ERR_PIPELINE.
static int pop_hold(lo_ctx* c) {
    const lo_ctx::Hold h = c->holds[0];
    for (int i = 1; i < c->n_hold; ++i) c->holds[i - 1] = c->holds[i];
    if (--c->n_hold == 0) g_holding.fetch_sub(1, std::memory_order_relaxed);
    LO_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_wait_final, dim3(1), dim3(kWave), 0, c->stream, c->d_fin + kFinWords * h.lane, h.seq, h.st,
                       c->d_hbroken, c->pipe_bound);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}
// All pending holds, oldest first.  Called at the top of every entry point that enqueues on the context stream, reads
// from it, or changes what a queued scan reads (and by sync_all); enqueue_optimize places the holds of a queue of scans
// itself (pop_hold).
int flush_hold(lo_ctx* c) {
    while (c->n_hold > 0) {
        const int rc = pop_hold(c);
        if (rc != LO_OK) return rc;
    }
    return LO_OK;
}

// Scans in flight for the scan being enqueued.  Two pay while the chip is half idle under one context's queue; when
// other contexts of the process are queueing scans too, their launches already fill it, and a second scan in flight per
// context only adds waits to the few hardware queues all their streams share (8 contexts: 24 streams on 4 queues ran
// 31 % slower in aggregate).  So unless lo_set_scan_depth / LO_OVERLAP_DEPTH chose, a context that is not alone in
// having scans in flight keeps one.
static int scan_depth(const lo_ctx* c) {
    if (!c->depth_auto) return c->depth;
    const int others = g_holding.load(std::memory_order_relaxed) - (c->n_hold > 0 ? 1 : 0);
    return others > 0 ? 1 : c->depth;
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
// ... that goes down the scan pipeline with the split pipe_main: the only path whose head may overlap the previous
// scan's tail
static bool pipelined_scan(const lo_ctx* c, bool cand, int pipe_main) {
    return cand && !c->kd && c->pipe && c->cfg.max_iterations > pipe_main;
}

// The context's members <-> a lane's set
static void lane_swap(lo_ctx* c, lo_ctx::ScanLane& A) {
    std::swap(A.d_slot, c->d_slot);
    std::swap(A.d_res_pko, c->d_res_pko);
    std::swap(A.d_wmask, c->d_wmask);
    std::swap(A.d_blk_cnt, c->d_blk_cnt);
    std::swap(A.d_blk_sum, c->d_blk_sum);
    std::swap(A.d_blk_m2, c->d_blk_m2);
    std::swap(A.d_blk_part, c->d_blk_part);
    std::swap(A.d_acc_part, c->d_acc_part);
    std::swap(A.d_cand_rec, c->d_cand_rec);
    std::swap(A.d_cand_cnt, c->d_cand_cnt);
    std::swap(A.d_js, c->d_js);
    std::swap(A.d_st, c->d_st);
}
// Lane `to` becomes the current one: a full set of the per-scan state on its first use (same sizes as ctx_alloc's and
// ensure_acc_part's), then the current set is parked in its own entry and lane `to`'s taken out of its entry.
// Depth 1: nothing of the lane swapped in is in flight, its last scan's hold was enqueued before the scan now pending
// started.  Depth >= 2: that hold may still be pending, and the caller enqueues it before anything touches the lane.
static int lane_switch(lo_ctx* c, int to) {
    lo_ctx::ScanLane& A = c->lanes[to];
    if (!c->lane_ready[to]) {
        const lo_config& g = c->cfg;
        const size_t NB = (static_cast<size_t>(g.max_points) + kBlock - 1) / kBlock;
        const size_t cand = static_cast<size_t>(g.num_alpha_segments) + 1;
        LO_HIP(c, A.d_slot.reserve(NB * kBlock));
        LO_HIP(c, A.d_res_pko.reserve(NB * kBlock));
        LO_HIP(c, A.d_wmask.reserve(NB * kWavesPerBlock));
        LO_HIP(c, A.d_blk_cnt.reserve(NB));
        LO_HIP(c, A.d_blk_sum.reserve(NB));
        LO_HIP(c, A.d_blk_m2.reserve(NB));
        LO_HIP(c, A.d_blk_part.reserve(NB * kNE));
        LO_HIP(c, A.d_js.reserve(kMaxAlpha + 1));
        LO_HIP(c, A.d_st.reserve(1));
        LO_HIP(c, hipMemsetAsync(A.d_st, 0, sizeof(DevState), c->stream));
        LO_HIP(c, A.d_cand_rec.reserve(cand * kCandWords));
        LO_HIP(c, A.d_cand_cnt.reserve(cand));
        // zeroed on the context stream: this scan's head follows there, and its tail starts only behind its main part
        LO_HIP(c, hipMemsetAsync(A.d_cand_cnt, 0, cand * sizeof(unsigned), c->stream));
        LO_HIP(c, A.d_acc_part.reserve(cand * kFuseMaxBlocks * kNE));
        c->lane_ready[to] = true;
    }
    lane_swap(c, c->lanes[c->lane]);                    // (that entry was empty: the members are now)
    lane_swap(c, A);
    c->lane = to;
    ++c->cfg_gen;                                       // a batch's cached device KParams name the other lane's buffers
    return LO_OK;
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
static void launch_correspond_first(lo_ctx* c, const KParams& P0, bool kd, int with_stats = 1) {
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
static void launch_exact_scale_any(lo_ctx* c, const KParams& P, int n2, hipStream_t s) {
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

int enqueue_optimize(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12], const int* n_dev) {
    const lo_config& g = c->cfg;
    std::memcpy(c->T_init, T_init, sizeof(float) * 12);
    c->last_n = n;
    c->last_pts = d_pts;
    c->last_ndev = n_dev;
    const unsigned ring_n0 = c->ring_n;                   // the run of pipelined scans ends here unless this is one
    c->ring_n = 0;
    // reset the GN state (pose by kernel argument: no host staging buffer, scans can queue back to back)
    Pose12 T0;
    std::memcpy(T0.v, T_init, sizeof(float) * 12);
    // HIP events only for synchronous calls (gpu_ms): a marker packet costs ~5-7 us of device time per scan
    const bool timed = c->sync_call;
    c->last_timed = timed;
    // scan overlap: a hold may be deferred (and a deferred one kept past this scan's head) only between two pipelined
    // scans that nothing times -- a synchronous call's HIP events and the stage timing bracket the whole scan -- and
    // whose points are the caller's: a device-filtered scan sits in the context's one point buffer, which the next
    // raw call's filter overwrites, so that call enqueues the hold first anyway
    const bool cand = cand_scan(c, n);
    const int depth = scan_depth(c);
    if (depth != c->depth_used) {                         // the holds pending were placed for the other order: all out first
        const int rcd = flush_hold(c);
        if (rcd != LO_OK) return rcd;
        c->depth_used = depth;
    }
    const bool may_defer = c->overlap && !timed && !c->stage_timing && !n_dev && !pipe_flagged(c);
    // this scan's head overlaps: a hold is pending and the scan is pipelined.  Only then does it take the queue's split
    // (pipe_main, 1 by default): the caller is queueing scans back to back, and the next head hides under a longer tail.
    // A scan behind a flushed hold (its caller read the previous result, or made any other call) keeps the split 2 a
    // scan always had unless one was chosen -- split 1 without overlap costs about 1 %.
    // Three or more in flight and no split chosen: the queue's split is 0 -- every GN iteration of an overlapping scan
    // runs on its lane's stream, and the context stream carries only the heads and the holds (DESIGN.md "Scan ring").
    const int queue_main = (c->pipe_main_auto && depth >= 3) ? 0 : c->pipe_main;
    const bool overlaps = c->n_hold != 0 && may_defer && pipelined_scan(c, cand, queue_main);
    const int pipe_main = (c->pipe_main_auto && !overlaps) ? 2 : queue_main;
    const bool defer = may_defer && pipelined_scan(c, cand, pipe_main);
    const int lane_before = c->lane;
    if (c->n_hold != 0) {
        if (!overlaps) {                                  // any other path: the context as it always was
            const int rcf = flush_hold(c);
            if (rcf != LO_OK) return rcf;
        } else {                                          // this scan's state goes to the next lane of the ring
            const int rcl = lane_switch(c, (c->lane + 1) % std::max(depth, 2));
            if (rcl != LO_OK) return rcl;
            // ... which scan k - depth used.  Two or more in flight: its hold may still be pending (with every older
            // one), and goes in front of this scan's head, which rewrites the state that scan's tail reads.
            // (Never more than `depth` in flight either, whatever lanes an earlier depth left the holds on.)
            int pops = c->n_hold - depth + 1;
            for (int i = 0; i < c->n_hold; ++i)
                if (c->holds[i].lane == c->lane) pops = std::max(pops, i + 1);
            for (int i = 0; depth > 1 && i < pops; ++i) {
                const int rch = pop_hold(c);
                if (rch != LO_OK) return rch;
            }
        }
    }
    if (c->lane != lane_before) c->prev_lane = lane_before;
    if (timed) LO_HIP(c, hipEventRecord(c->ev0, c->stream));
    if (n == 0) {
        hipLaunchKernelGGL(k_init, dim3(1), dim3(64), 0, c->stream, c->d_st, T0, 1.0, g.robust_loss_delta);
    } else {
        const int rc = ensure_acc_part(c);
        if (rc != LO_OK) return rc;
        KParams P = make_params(c, d_pts, static_cast<int>(n));
        P.n_dev = n_dev;                                  // device-filtered scan: count read on the device
        KParams P0 = P;                                   // first k_correspond also resets the GN state
        P0.init = 1;
        std::memcpy(P0.T0, T_init, sizeof(float) * 12);
        std::memcpy(P.T0, T_init, sizeof(float) * 12);   // k_solve_correspond's pose before iteration 0
        // small scan with PKO: the solve of iteration it runs fused with the correspondence search of it + 1
        // (k_solve_correspond; KDTree: k_solve_knn, then k_knn_brute + k_plane), the last solve alone (k_solve_pick)
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
            if (!cand) {                                  // (n2 > 0 exactly when n <= kExactMaxPoints)
                // reference-exact GN loop without candidates (lo_exact.hip): correspondences, (iteration 0) sorted-order
                // scale, PKO, per-point fp32 terms, sequential sums + fp32 LDLT + SVD-projected update
                for (int it = 0; it < g.max_iterations; ++it) launch_exact_iteration(c, P, P0, it, n2, c->kd);
                LO_HIP(c, hipGetLastError());
                if (timed) LO_HIP(c, hipEventRecord(c->ev1, c->stream));
                c->pending = true;
                return LO_OK;
            }
            // small scans with PKO: the same launch sequence as the default mode, with the sorted-order scale after the
            // first correspondence launch and the PKO launch's candidates forming the reference's sequential sums
            P.exact_cand = P0.exact_cand = 1;
        }
        if (pipe_flagged(c)) {                            // an earlier scan's wait timed out: one stream from now on
            const int rc4 = pipe_recover(c);
            if (rc4 != LO_OK) return rc4;
        }
        if (pipelined_scan(c, cand, pipe_main)) {         // (c->pipe as it is now: a recovery above switched it off)
            // scan pipeline: iterations < pipe_main on the context stream, the rest on the tail stream behind a
            // device-side wait for the main part; k_wait_final then holds the context stream until the scan's result
            // is final
            const int rc2 = pipe_alloc(c);
            if (rc2 != LO_OK) return rc2;
            if (++c->pipe_seq == 0) c->pipe_seq = 1;      // (the test hook's count: LO_PIPE_FAIL_AT is never 0)
            const bool fail = c->pipe_fail_at != 0 && c->pipe_seq == c->pipe_fail_at;
            const int lane = c->lane;
            if (++c->lane_seq[lane] == 0) c->lane_seq[lane] = 1;   // 0 is the fence word's reset value, never a scan's number
            const uint32_t seq = c->lane_seq[lane];
            uint32_t* const fin = c->d_fin + kFinWords * lane;
            // one scan in flight: both lanes' tails on the first tail stream, as before there were two -- tail(k) starts
            // behind tail(k - 1) anyway, and a third stream per context only crowds the hardware queues of a process
            // that runs many contexts
            const int tl = depth > 1 ? lane : 0;
            if (!c->s_tail[tl]) LO_HIP(c, hipStreamCreateWithFlags(&c->s_tail[tl], hipStreamNonBlocking));
            const hipStream_t s_tail = c->s_tail[tl];
            P.fin = P0.fin = fin;
            P.seq = P0.seq = seq;
            P.rec = P0.rec = c->d_ring + static_cast<size_t>(c->ring_pos % kRingRecords) * kRecWords;
            ++c->ring_pos;
            c->ring_n = std::min<unsigned>(ring_n0 + 1, kRingRecords);
            KParams Pt = P;                               // tail launches: leave once scan seq is final (the
            Pt.tail = 1;                                  // DevState may already be the next scan's)
            KParams Ph = P;                               // the main part's last pick signals the tail (signal_main)
            Ph.hold = 1;
            // host submission order of a queue of scans with d = depth >= 2 in flight, scan k on lane k % d:
            //   context stream:     k_wait_final(k - d) -> head(k) -> main(k)     (the wait was placed above)
            //   lane stream k % d:  k_wait_seq(k) -> tail(k)
            // and k_wait_final(k) is placed by scan k + d, or by flush_hold.  main(k) is the iterations below the split:
            // with split 0 (the queue's split from three in flight on) there is none, the context stream carries
            // k_wait_final(k - d) -> head(k) -> k_signal_main(k), and every iteration is tail(k).  With one scan in
            // flight (depth 1) the context stream carries head(k) -> k_wait_final(k - 1) -> main(k) instead.
            // Every device-side wait depends only on work submitted before it, on any stream: k_wait_final(j) polls
            // the lane's word that main(j) or tail(j) publishes, both submitted during scan j's own call, which
            // returned before any call that can place that wait; k_wait_seq(k) polls the lane's word that main(k)'s
            // last pick sets -- with split 0 the one k_signal_main(k) sets behind head(k) -- submitted just above it,
            // or the one main(k) publishes when it ends the scan.  Nothing waits for a later submission, so the order
            // is deadlock-free even if all the streams share one hardware queue (they then simply run in this order),
            // and every wait is bounded by pipe_bound besides.
            // head(k) rewrites the lane state of scan k - d: k_wait_final(k - d) precedes it on this stream, so that
            // scan is final, and what is left of its tail leaves on tail_gone before touching anything.  The lane's
            // words count the lane's own scans, which are final in order; between the lanes no order is assumed --
            // scan k may be final before scan k - 1.  main(k) and main(k - 1) follow each other on this stream; with
            // split 0 tail(k) and tail(k - 1) share nothing but the map and the tables, which neither writes.
            launch_correspond_first(c, P0, false);
            if (c->exact) launch_exact_scale_any(c, P, n2, c->stream);
            // split 0: no pick of a main part to say so -- "head done" is one more launch behind the head (the head's
            // stores are out when it starts; it releases and sets the lane's word).  The context stream is not the
            // bound once the iterations have left it.
            if (pipe_main == 0) hipLaunchKernelGGL(k_signal_main, dim3(1), dim3(kWave), 0, c->stream, fin, seq);
            if (overlaps) ++c->overlapped;                // its head went in front of the previous scan's hold
            if (c->n_hold != 0 && depth <= 1) {        // one scan in flight: that hold now, behind this scan's head
                const int rcf = flush_hold(c);
                if (rcf != LO_OK) return rcf;
            }
            for (int it = 0; it < g.max_iterations; ++it) {
                const bool tail = it >= pipe_main;
                if (it == pipe_main)                   // bound 0: the test hook's forced timeout
                    hipLaunchKernelGGL(k_wait_seq, dim3(1), dim3(kWave), 0, s_tail, fin, seq, c->d_st, c->d_hbroken,
                                       fail ? 0ull : c->pipe_bound);
                const hipStream_t s = tail ? s_tail : c->stream;
                const KParams& Pi = tail ? Pt : (it + 1 == pipe_main ? Ph : P);
                launch_pko_spec(c, Pi, it, s);
                if (it + 1 < g.max_iterations) hipLaunchKernelGGL(k_pick_correspond, dim3(P.nb), dim3(kBlock), 0, s, Pi, it);
                else hipLaunchKernelGGL(k_pick, dim3(1), dim3(kBlock), 0, s, Pi, it);
            }
            if (defer && c->n_hold < kMaxLanes) {         // enqueued by a later pipelined scan, or by flush_hold
                if (c->n_hold == 0) g_holding.fetch_add(1, std::memory_order_relaxed);
                c->holds[c->n_hold++] = lo_ctx::Hold{seq, lane, c->d_st};
            } else {
                const int rcf = flush_hold(c);            // (none pending: a scan that does not defer flushed them above)
                if (rcf != LO_OK) return rcf;
                hipLaunchKernelGGL(k_wait_final, dim3(1), dim3(kWave), 0, c->stream, fin, seq, c->d_st, c->d_hbroken,
                                   c->pipe_bound);
            }
            LO_HIP(c, hipGetLastError());
            if (timed) LO_HIP(c, hipEventRecord(c->ev1, c->stream));
            c->pending = true;
            return LO_OK;
        }
        const int rcf = flush_hold(c);                    // (none pending unless the pipeline was just switched off)
        if (rcf != LO_OK) return rcf;
        for (int it = 0; it < g.max_iterations; ++it) {
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
            if (it + 1 < g.max_iterations && !c->kd) {
                if (P.cand_rec) hipLaunchKernelGGL(k_pick_correspond, dim3(P.nb), dim3(kBlock), 0, c->stream, P, it);
                else hipLaunchKernelGGL(k_solve_correspond, dim3(P.nb), dim3(kBlock), 0, c->stream, P, it);
            } else if (it + 1 < g.max_iterations) {
                launch_pick_knn(c, P, it);
            } else if (P.cand_rec) {
                hipLaunchKernelGGL(k_pick, dim3(1), dim3(kBlock), 0, c->stream, P, it);
            } else {
                hipLaunchKernelGGL(k_solve_pick, dim3(1), dim3(kBlock), 0, c->stream, P, it);
            }
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
    LO_HIP(c, hipMemcpyAsync(c->h_st, c->d_st, bytes, hipMemcpyDeviceToHost, c->stream));
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
        LO_HIP(c, hipMemcpyAsync(c->h_st, c->d_st, bytes, hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        c->pending = false;
        ++c->pipe_reruns;
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
        LO_HIP(c, hipMemcpyAsync(c->h_st, c->d_st, bytes, hipMemcpyDeviceToHost, c->stream));
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

int lo_icp_flush(lo_ctx* c) {
    if (!c) return LO_ERR_ARG;
    return flush_hold(c);
}

int lo_icp_queue_records(lo_ctx* c, int n_last, float* out16xN) {
    if (!c || n_last < 0 || (n_last > 0 && !out16xN)) return LO_ERR_ARG;
    if (n_last > kRingRecords || static_cast<unsigned>(n_last) > c->ring_n) {
        c->err = "lo_icp_queue_records: n_last exceeds the ring, or the pipelined scans queued since the last other call";
        return LO_ERR_ARG;
    }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));                              // the holds, then every stream of the context
    if (pipe_flagged(c)) {                               // a wait timed out: those scans' records were never written
        const int rc = pipe_recover(c);
        return rc != LO_OK ? rc : LO_ERR_PIPELINE;
    }
    const unsigned long long first = c->ring_pos - static_cast<unsigned long long>(n_last);
    // oldest first: the run up to the ring's end, then the wrapped rest
    const size_t slot = static_cast<size_t>(first % kRingRecords);
    const size_t run = std::min<size_t>(static_cast<size_t>(n_last), kRingRecords - slot);
    if (run > 0)
        LO_HIP(c, hipMemcpy(out16xN, c->d_ring + slot * kRecWords, run * kRecWords * sizeof(float), hipMemcpyDeviceToHost));
    if (run < static_cast<size_t>(n_last))
        LO_HIP(c, hipMemcpy(out16xN + run * kRecWords, c->d_ring.get(), (n_last - run) * kRecWords * sizeof(float),
                            hipMemcpyDeviceToHost));
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
                      lo_iter_log* logs, lo_stats* st) {
    int rc = LO_OK;
    bool with_order = false;
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
        LO_HIP(c, hipMemcpyAsync(c->h_st, c->d_st, head, hipMemcpyDeviceToHost, c->stream));
        LO_HIP(c, hipStreamSynchronize(c->stream));
        if (c->h_st->done) break;                                 // converged, or too few correspondences
    }
    const bool converged = c->h_st->done && c->h_st->status == LO_OK;
    if (converged && P.kd_all) hipLaunchKernelGGL(k_inlier_all, all_grid(P), dim3(kAllThreads), all_lds(P), c->stream, P);
    else if (converged) hipLaunchKernelGGL(k_inlier, dim3(P.nb), blk, 0, c->stream, P);
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipEventRecord(c->ev1, c->stream));
    const size_t bytes = head + sizeof(lo_iter_log) * static_cast<size_t>(LO_MAX_ITERS);
    LO_HIP(c, hipMemcpyAsync(c->h_st, c->d_st, bytes, hipMemcpyDeviceToHost, c->stream));
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
