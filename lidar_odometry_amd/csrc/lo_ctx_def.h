// lo_ctx_def.h — the ICP context itself and the helpers its translation units share (lo_ctx, lo_surfel, lo_grid,
// lo_optimize, lo_scanq, lo_hooks, lo_batch .hip).  Nothing else includes this: lo_devmap, lo_iris, lo_gmap and
// lo_voxelmap reach a context through lo_ctx_internal.h.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "lo_buf.h"
#include "lo_ctx_internal.h"
#include "lo_device.h"
#include "lo_exact.h"
#include "lo_kdorder.h"
#include "lo_kernels_decl.h"
#include "lo_math.h"
#include "lo_pko_tables.h"
#include "lo_scanq.h"
#include "lo_seqsum.h"
#include "lo_vfilter.h"

using namespace lo;

// Dense uniform grid over a point set (the kd-tree's role): points sorted by cell, x fastest, index order
// inside a cell; start[cell] = first point, start[ncell] = m.
struct PointGrid {
    DevBuf<float4> d_pts;
    DevBuf<uint32_t> d_start;
    DevBuf<uint32_t> d_vpos;        // nanoflann visit order (lo_kdorder.h): vAcc_ position per original index
    DevBuf<KdNode> d_nodes;         //   and the tree's nodes (root = 0)
    bool has_order = false;         // d_vpos / d_nodes hold the visit order of the current points
    bool all = false;               // d_pts in index order, no cells (all_pairs_upload: k_knn_all / k_inlier_all)
    PinnedBuf<void> h_stage;        // pinned upload staging (grid_build)
    int m = 0;
    int org[3] = {0, 0, 0}, dim[3] = {1, 1, 1};
    float h = 1.0f;
};

// The device grid builder's scratch per context (lo_grid.hip; the solo and the batched form share it): the bounds
// readback, each point's cell / arrival number / slot (d_keys: 3 words per point), the cell counts, and the solo
// scan's chunk sums (a batch keeps its own for all jobs).
// d_bounds / h_bounds hold kGridWords 4-byte words: [0..5] the bounds, [6] the raw count, then
constexpr int kGridOcc = 7;        // occupied cells (the min_per_cell rule)
constexpr int kGridBad = 8;        // a non-finite world point (k_cloud_world)
constexpr int kGridCount = 9;      // a host-known count handed to the device builder
constexpr int kGridWords = 16;
struct DevGridScratch {
    DevBuf<float> d_bounds;
    PinnedBuf<float> h_bounds;
    DevBuf<uint32_t> d_keys;
    DevBuf<uint32_t> d_counts;
    DevBuf<uint32_t> d_bsum;
};

struct lo_ctx {
    lo_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;
    // scan buffers
    DevBuf<float> d_pts;
    ScanQueue q;                    // the scan queue, and the lanes of per-scan state (lo_scanq.h; cur(c) is the current)
    bool presolve = true;           // candidates solve inside the PKO launch (LO_PRESOLVE=0: k_solve_* instead)
    bool exact = true;              // lo_set_exact: the reference's own arithmetic order (lo_exact.hip) -- the default;
                                    //   lo_set_exact(ctx, 0) opts into the fast mode (fp64 tree sums, not parity-safe)
    uint64_t cfg_gen = 0;           // bumped by lo_update_config and by (re)allocations of the PKO / candidate buffers: a
                                    //   batch's cached device KParams of this context are stale once it changes
    DevBuf<float> d_ex_terms;
    DevBuf<float> d_ex_tot;         //   large scans: the 43 sums (launch_mw_sums -> k_exact_finish)
    DevBuf<double> d_ex_rank;       //   the iteration-0 residuals in sorted order (k_rank_sort, kExactMaxPoints)
    bool ex_merge = false;          //   this scan's exact scale runs in one launch (k_exact_scale_c: counting sort + sums)
    bool ex_attr = false;           //   the exact-scale kernels' dynamic-LDS attributes are set (per context)
    DevBuf<void> d_mw;              //   large scans: head records of the 43 column sums (lo_seqsum.h MwBuf)
    size_t mw_n = 0;                //   the scan size d_mw / d_mwm are laid out for (0: none)
    MwBuf mw{};
    DevBuf<void> d_mwm;             //   large scans: head records of the iteration-0 scale's two sums (MwmBuf)
    MwmBuf mwm{};
    DevBuf<double> d_ex_res;        //   scans beyond kExactMaxPoints: residuals, sorted residuals, hipCUB scratch
    DevBuf<double> d_ex_sorted;
    DevBuf<void> d_ex_sort_tmp;
    DevBuf<double> d_res;           // parity entry points (per-point residual / direct residual input)
    DevBuf<uint8_t> d_u8;
    PinnedBuf<DevState> h_st;
    PinnedBuf<int> h_nf;            // the device-filtered scan's count, read back with the result
    bool nf_valid = false;          //   h_nf holds the last device-filtered scan's count (lo_icp_result)
    // map
    DevBuf<Slot> d_tab;             // capacity: allocated slots
    uint32_t log2cap = 1;
    size_t n_surfels = 0;
    // in-place table patches (lo_map_patch_surfels): the keys resident on the device, tombstones left by erases,
    // a pinned staging buffer + device copy of the patch records, and the synced host map (lo_map_sync_voxelmap)
    std::unordered_set<uint64_t> resident;
    size_t n_tomb = 0;
    PinnedBuf<void> h_patch;
    DevBuf<void> d_patch;
    hipEvent_t ev_patch = nullptr;
    uint64_t map_src = 0, map_epoch = 0, map_pos = 0;
    uint64_t tab_gen = 0;           // bumped by every full upload (a pending fit's results no longer apply to it)
    uint64_t tab_edit = 0;          // bumped by every change of the table (uploads, patches, fits, a device map's claim)
    // lo_map_sync_surfels: the surfel set last synced through it (key -> normal, centroid), valid while the table has
    // not been changed by anything else since (mirror_edit == tab_edit)
    std::unordered_map<uint64_t, std::array<float, 6>> smirror;
    uint64_t mirror_edit = ~0ull;
    uint64_t devmap_gen = 0;        // the generation a device map (lo_devmap) reserved and maintains
    // deferred surfel fits of a synced host map (lo::ctx_fit_surfels): pinned in / out staging, device copies
    PinnedBuf<void> h_fit_in;
    DevBuf<void> d_fit_in;
    PinnedBuf<void> h_fit_out;      // FitResult records
    DevBuf<void> d_fit_out;
    hipEvent_t ev_fit = nullptr;
    uint64_t fit_ticket = 0;        // the launch whose results sit in h_fit_out (0: none)
    uint64_t fit_gen = 0;           //   and the table generation it patched
    std::vector<uint64_t> fit_keys; //   its packed keys, job order
    bool fit_reconciled = false;    //   its planarity failures already removed from `resident`
    float fit_thr = 0.0f;
    // KDTree variant: dense grid over the L0 centroids + per-point neighbour / plane / residual buffers
    bool kd = false;
    PointGrid grid;                 // the map's L0 centroids (lo_map_set_points, or ctx_grid_from_device)
    DevGridScratch gscr;
    bool grid_dev = false;          // the grid was built on the device (no kd visit order; ties re-run, lo_icp_result)
    int kd_reruns = 0;              //   scans re-run with the order after such a tie (lo_kd_reruns)
    PointGrid lgrid;                // loop closure: the matched keyframe's local map (lo_icp_optimize_loop)
    DevBuf<float> d_lworld;         //   a device-resident matched cloud in the world, before it is gridded (_loop_dev)
    uint64_t loop_reruns = 0;       //   solves rerun with the kd visit order (a deciding distance tie)
    DevBuf<int32_t> d_kd_nbr;
    DevBuf<int32_t> d_kd_unres;
    DevBuf<double> d_kd_res;
    DevBuf<Slot> d_kd_plane;
    // device preprocessing (FastVoxelFilter): raw staging for host input + filter work buffers
    DevBuf<float> d_raw;
    VfBuffers vf;
    bool last_dev_count = false;    // last optimize took its point count from the device filter
    // PKO tables
    PkoTables tables;
    DevBuf<double> d_alphas;
    DevBuf<double> d_Z;
    DevBuf<int32_t> d_tabs_i;       // small_off | small_perm | base | ev_off | ev_steps | km_draws
    size_t off_small_off = 0, off_small_perm = 0, off_base = 0, off_ev_off = 0, off_ev_steps = 0, off_km = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // in-step timing of each scan's first correspondence launch (lo_set_stage_timing / lo_stage_time)
    bool stage_timing = false;
    std::vector<hipEvent_t> st_ev;  // pairs: [2 i] before, [2 i + 1] after
    int st_n = 0;
    DevBuf<unsigned long long> d_span;      // in-kernel span stamps (kSpanWords per launch): stage-timed launch i at
                                            //   kSpanWords i; lo_bench_kernel 5 at kSpanWords kStageEvents
    float T_init[12];
    size_t last_n = 0;
    bool pending = false;
    int pko_groups = 0;             // EM workgroups per PKO launch (lo_set_pko_groups / LO_PKO_GROUPS; 0 = one per alpha)
    bool pko_solo = false;          // LO_PKO_SOLO=1 (A/B): the speculative PKO launch asks for enough LDS that one
                                    //   workgroup holds a CU alone (no other launch's waves on its SIMDs)
    const float* last_pts = nullptr;   // the scan in flight (a re-run after a pipeline timeout)
    const int* last_ndev = nullptr;
    bool sync_call = false;         // the optimize in flight is a synchronous call: HIP events time it (gpu_ms)
    bool last_timed = false;
};

namespace lo {
constexpr int kStageEvents = 1024;
constexpr int kExactMaxPoints = 16384;                // reference-exact mode: one-workgroup sort in LDS up to here

// lo_ctx.hip
hipError_t sync_all(lo_ctx* c);
int kd_alloc(lo_ctx* c);
extern std::mutex g_live_mu;
extern std::unordered_set<const lo_ctx*> g_live;
extern uint64_t g_ticket;
// lo_grid.hip
int grid_build(lo_ctx* c, PointGrid& G, const float* xyz, size_t m, bool with_order = true, int min_per_cell = 0);
int all_pairs_upload(lo_ctx* c, PointGrid& G, const float* xyz, size_t m, const float* q = nullptr, size_t nq = 0);
int grid_add_order(lo_ctx* c);
int grid_add_order(lo_ctx* c, PointGrid& G, int min_per_cell);
int grid_from_device(lo_ctx* c, PointGrid& G, const float* d_xyz, const int* d_count, size_t cap, int min_per_cell);
int loop_map_from_device(lo_ctx* c, PointGrid& G, const float* d_xyz, size_t m, const float T[12], int min_per_cell);
// lo_optimize.hip
void launch_pko(lo_ctx* c, const KParams& P, int it);
bool spec_ok(const KParams& P);
void launch_pko_spec(lo_ctx* c, const KParams& P, int it, hipStream_t s = nullptr);
void launch_brute(lo_ctx* c, const KParams& P);
void launch_correspond(lo_ctx* c, const KParams& P, int with_stats, bool kd);
void launch_correspond_first(lo_ctx* c, const KParams& P0, bool kd, int with_stats = 1);
void launch_exact_scale_any(lo_ctx* c, const KParams& P, int n2, hipStream_t s);
int enqueue_optimize(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12], const int* n_dev = nullptr);
int enqueue_ring(lo_ctx* c, const float* d_pts, size_t n, const float T_init[12], const int* n_dev);
int loop_rerun_with_order(lo_ctx* c, const float* d_curr, size_t n_curr, const float T_curr[12], size_t n_matched,
                          const float T_matched[12], float T_rel_out[12], float* inlier_ratio, lo_iter_log* logs,
                          lo_stats* st);
// lo_scanq.hip
// the per-scan state of the last enqueued scan: its lane's, or (a grouped scan) its set in the group's slot
inline ScanLane& cur(lo_ctx* c) { return c->q.grp.cur ? *c->q.grp.cur : c->q.lanes[c->q.lane]; }
// ... back on the ring's current lane: whatever builds KParams for a launch of its own (a ring scan, a batch job, the
// loop-closure solve, the parity entry points) does so on a lane, which has the candidate buffers
inline void leave_group_set(lo_ctx* c) {
    if (!c->q.grp.cur) return;
    c->q.grp.cur = c->q.grp.prev = nullptr;
    ++c->cfg_gen;
}
int lane_alloc_base(lo_ctx* c, ScanLane& L);    // everything but the candidate buffers, sized by max_points
int lane_alloc_cand(lo_ctx* c, ScanLane& L);    // the candidate buffers, sized by the alpha grid (d_acc_part last)
int flush_hold(lo_ctx* c);     // the pending holds of the last pipelined scans, enqueued on the context stream now
int pipe_recover(lo_ctx* c);
ScanPlanIn scan_snapshot(const lo_ctx* c, bool cand, bool timed, bool dev_count);
int apply_plan(lo_ctx* c, const ScanPlan& plan);
int emit_pipelined(lo_ctx* c, const ScanPlan& plan, KParams& P, KParams& P0, int n2, unsigned ring_run);
// scan groups (lo_scan_group_plan.h)
GroupPlanIn group_snapshot(const lo_ctx* c, size_t n, bool cand, bool timed, bool dev_count);
int group_append(lo_ctx* c, const GroupPlan& plan, const float* d_pts, size_t n, const float T_init[12]);
int group_emit(lo_ctx* c);     // the open group leaves (lockstep on its slot's stream, or scan by scan down the ring)
int group_flush(lo_ctx* c);    // ... and the context stream waits for every slot's last group (flush_hold calls this)
int group_join(lo_ctx* c);     // the context stream behind every slot's last group (flush_hold, every ring-path scan)
hipError_t group_sync(lo_ctx* c);
void group_release(lo_ctx* c);

// ---- per-scan helpers on the launch path of every optimize, single and batched: inline, as when one file held them
// PKO workgroups: one alpha of the JS grid per workgroup (each fits the GMM redundantly), capped at kPkoMaxWGs
inline int pko_grid(const lo_config& g) { return std::max(1, std::min(kPkoMaxWGs, g.num_alpha_segments)); }
// the context's EM workgroup count: pko_groups (lo_set_pko_groups; 0 = one alpha per workgroup, pko_grid)
inline int pko_grid(const lo_ctx* c) {
    const int full = pko_grid(c->cfg);
    return c->pko_groups > 0 ? std::min(full, c->pko_groups) : full;
}

constexpr size_t kPkoSoloBytes = 64 * 1024;   // + the ~22-27 KB static part: more than half of a CU's 160 KB
// the speculative normal equations and candidate records (first PKO optimize, and after lo_update_config dropped them)
inline int ensure_acc_part(lo_ctx* c) {
    leave_group_set(c);
    ScanLane& L = cur(c);
    if (L.d_acc_part || !c->cfg.use_adaptive_m_estimator) return LO_OK;    // (set last: "all three")
    const int rc = lane_alloc_cand(c, L);
    if (rc != LO_OK) return rc;
    LO_HIP(c, hipMemset(L.d_cand_cnt, 0, L.d_cand_cnt.capacity() * sizeof(unsigned)));
    ++c->cfg_gen;
    // the exact candidates' staging sits in the PKO launch's dynamic LDS (beyond the 64 KB default with the static part)
    LO_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_pko_tx), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(std::max(kXcLdsBytes + 16384, kPkoSoloBytes))));
    LO_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_pko_t<4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  static_cast<int>(kPkoSoloBytes)));
    return LO_OK;
}

// A host scan in pinned memory (lo_host_alloc, hipHostMalloc, hipHostRegister): the device address that aliases it,
// so the filter reads the sampled points over the bus directly instead of a staging copy of the whole scan.
inline const float* pinned_alias(const float* p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // pageable
    if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
    return reinterpret_cast<const float*>(static_cast<const char*>(a.devicePointer) +
                                          (reinterpret_cast<const char*>(p) - static_cast<const char*>(a.hostPointer)));
}

inline void set_kd_params(lo_ctx* c, KParams& P, const PointGrid& G) {
    P.tab = c->d_kd_plane;
    P.kd_pts = G.d_pts;
    P.kd_start = G.d_start;
    P.kd_vpos = G.has_order ? G.d_vpos : nullptr;
    P.kd_nodes = G.has_order ? G.d_nodes : nullptr;
    P.kd_m = G.m;
    for (int a = 0; a < 3; ++a) { P.kd_org[a] = G.org[a]; P.kd_dim[a] = G.dim[a]; }
    P.kd_h = G.h;
    P.kd_all = G.all ? 1 : 0;
    P.kd_nbr = c->d_kd_nbr;
    P.kd_unres = c->d_kd_unres;
    P.kd_res = c->d_kd_res;
    P.kd_plane = c->d_kd_plane;
}

inline KParams make_params(lo_ctx* c, const float* d_pts, int n) {
    KParams P{};
    const lo_config& g = c->cfg;
    P.pts = d_pts;
    P.n = n;
    P.nb = (n + kBlock - 1) / kBlock;
    P.nb_acc = P.nb < kAccBlocks ? (P.nb > 0 ? P.nb : 1) : kAccBlocks;
    P.tab = c->d_tab;
    P.log2cap = c->log2cap;
    P.l1scale = g.voxel_size * static_cast<float>(g.hierarchy_factor);   // PointToVoxelKey (VoxelMap.cpp:51-52)
    P.max_iters = g.max_iterations;
    P.tol_t = g.translation_tolerance;
    P.tol_r = g.rotation_tolerance;
    P.maxd = g.max_correspondence_distance;
    P.min_corr = g.min_correspondence_points;
    P.robust = g.use_robust_loss;
    P.robust_delta = g.robust_loss_delta;
    P.cauchy_loss = g.loss_cauchy;
    P.use_pko = g.use_adaptive_m_estimator;
    P.S = g.gmm_sample_size;
    P.K = g.gmm_components;
    P.NA = g.num_alpha_segments;
    P.pko_kernel = g.pko_kernel;
    P.min_scale = g.min_scale_factor;
    P.trunc = g.truncated_threshold;
    P.alphas = c->d_alphas;
    P.Z = c->d_Z;
    P.small_off = c->d_tabs_i + c->off_small_off;
    P.small_perm = c->d_tabs_i + c->off_small_perm;
    P.base = c->d_tabs_i + c->off_base;
    P.ev_off = c->d_tabs_i + c->off_ev_off;
    P.ev_steps = c->d_tabs_i + c->off_ev_steps;
    P.km_draws = c->d_tabs_i + c->off_km;
    const ScanLane& L = cur(c);
    P.slot = L.d_slot;
    P.wmask = L.d_wmask;
    P.blk_cnt = L.d_blk_cnt;
    P.blk_sum = L.d_blk_sum;
    P.blk_m2 = L.d_blk_m2;
    P.blk_part = L.d_blk_part;
    P.acc_part = L.d_acc_part;
    P.cand_rec = c->presolve ? L.d_cand_rec.get() : nullptr;   // candidates pre-solve (k_pick*, KDTree: k_pick_knn)
    P.cand_cnt = L.d_cand_cnt;
    P.js = L.d_js;
    P.res_dbg = nullptr;
    P.res_out = L.d_res_pko;
    P.direct_res = nullptr;
    P.st = L.d_st;
    P.em_stat = c->stage_timing ? reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(L.d_st.get()) +
                                                                        offsetof(DevState, em_stat))
                                : nullptr;                  // the lead PKO workgroup's EM clock (stage timing)
    if (c->kd) set_kd_params(c, P, c->grid);             // KDTree path: downstream kernels read per-point planes
    return P;
}
}  // namespace lo
